// m3_inst.hip -- one board configuration's kernels + launchers (m3_kernels.hpp),
// compiled once per configuration: -DM3_INST=<id> (0 .. N_CONFIGS - 1).
// With -DM3_PART=<0..3> only one group of the configuration's launchers (and the kernels they
// launch) is instantiated here and the others are declared extern: the 32 x 32-frame
// configurations take ~20 minutes each in one translation unit, so the Makefile builds them
// in four (the same kernels, spread over the cores).
#include "m3_kernels.hpp"

#ifndef M3_INST
#error "compile with -DM3_INST=<configuration id>"
#endif
#define M3_CAT_(a, b) a##b
#define M3_CAT(a, b) M3_CAT_(a, b)

namespace m3k {
#ifndef M3_PART
M3_INSTANTIATE(template, M3_CAT(CF_, M3_INST))
#else
#ifdef M3_PHASE_PROF
#error "M3_PHASE_PROF keeps its counters per translation unit: build the configuration whole (no M3_PART)"
#endif
using CF_PART = M3_CAT(CF_, M3_INST);
M3_INSTANTIATE(extern template, CF_PART)
#if M3_PART == 0
template int launch_env_step<CF_PART>(m3_env*, const int32_t*);
#elif M3_PART == 1
template int launch_init<CF_PART>(hipStream_t, const InitArgs&, int64_t);
#elif M3_PART == 2
template int launch_apply<CF_PART>(m3_ctx*, const ApplyArgs&);
template int launch_legal<CF_PART>(m3_ctx*, int64_t, const int8_t*, uint32_t*);
template int fill_next_slots<CF_PART>(m3_env*);
template int rederive<CF_PART>(m3_env*);
template int launch_lookahead<CF_PART>(hipStream_t, const LookArgs&);
#elif M3_PART == 3
template int launch_rollouts<CF_PART>(m3_ctx*, const RolloutArgs&);
#else
#error "M3_PART is 0 .. 3"
#endif
#endif
}  // namespace m3k

#if defined(M3_PHASE_PROF) && !defined(M3_PART)
extern "C" int M3_CAT(m3_prof_read_, M3_INST)(uint64_t* out, int reset) { return m3_prof_read_tu(out, reset); }
#endif
