"""The one build recipe of the TEST-ONLY host harnesses (tests/*_host, tests/hostcore)."""
import glob
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "element-crush-gym_amd", "csrc")


def build(lib_path, source, opt_flags):
    """Compile `source` into the shared library `lib_path` unless that is newer than the source and every
    header of the device sources (a harness compiles whatever it includes from there)."""
    newest = max(os.path.getmtime(s) for s in [source] + glob.glob(os.path.join(CSRC, "*.hpp")))
    if os.path.exists(lib_path) and os.path.getmtime(lib_path) >= newest:
        return
    subprocess.run(["hipcc", "--offload-arch=gfx950", *opt_flags, "-std=c++17", "-fPIC", "-shared",
                    "-o", lib_path + ".tmp", source], check=True)
    os.replace(lib_path + ".tmp", lib_path)
