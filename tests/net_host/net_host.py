"""ctypes face of the TEST-ONLY host build of the policy/value network's core (net_host.hip)."""
import ctypes
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from hostbuild import build  # noqa: E402

LIB = os.path.join(HERE, "libnet_host.so")
_lib = None


def p(a):
    return ctypes.c_void_p(a.ctypes.data)


def lib():
    global _lib
    if _lib is None:
        build(LIB, os.path.join(HERE, "net_host.hip"), ["--offload-host-only", "-O1"])
        L = ctypes.CDLL(LIB)
        vp, i32, i64, f64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_double
        L.nt_features_ok.argtypes, L.nt_features_ok.restype = [i32], i32
        L.nt_bf16_round.argtypes, L.nt_bf16_round.restype = [vp, i64, vp], None
        L.nt_bf16_round_f64.argtypes, L.nt_bf16_round_f64.restype = [vp, i64, vp], None
        L.nt_bf16_widen.argtypes, L.nt_bf16_widen.restype = [vp, i64, vp], None
        L.nt_fold.argtypes, L.nt_fold.restype = [vp] * 6 + [f64, i64, i32, vp, vp, vp], None
        L.nt_pack_elems.argtypes, L.nt_pack_elems.restype = [i32], i64
        L.nt_pack_index.argtypes, L.nt_pack_index.restype = [i32, i64, i32], i64
        L.nt_pack.argtypes, L.nt_pack.restype = [i32, vp, vp], None
        L.nt_unpack.argtypes, L.nt_unpack.restype = [i32, vp, vp], None
        L.nt_tap_row.argtypes, L.nt_tap_row.restype = [i64, i64, i32, i32, i32], i64
        L.nt_acc_row.argtypes, L.nt_acc_row.restype = [i32, i32], i32
        L.nt_blob_len.argtypes, L.nt_blob_len.restype = [i32] * 5, i64
        L.nt_stem.argtypes, L.nt_stem.restype = [vp, i64, i32, i32, i32, i32, vp, vp, vp], None
        _lib = L
    return _lib
