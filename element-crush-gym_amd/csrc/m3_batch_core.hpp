// m3_batch_core.hpp -- what the batched step, rollout and stateless apply paths do per board, without
// the kernels around it: the per-shape geometry and tunables (KS), the pool and record sizes, and the
// per-board cores of the stateless apply and the rollouts (apply_and_emit, rollout_one). Everything is
// M3_HD or constexpr and nothing here needs the HIP runtime, so the kernels (m3_kernels.hpp) and the host
// harnesses (tests/hostcore, tests/lookahead_host) compile the same text. The staging, the env step
// (env_step_one, env_fin_*, the kernels' own cascade calls) and the launchers stay in m3_kernels.hpp.
#pragma once

#include "m3_rules.hpp"

// launcher signatures name these structs: they need linkage (m3_inst.hip instantiates them)
namespace m3k {
struct ApplyArgs {
    m3::Shape shape;  // the board (frame kernels; the specialised ones ignore it)
    int64_t n;
    const int8_t* boards;
    const uint32_t* seeds;
    const int32_t* n_actions;
    const int32_t* actions;
    int8_t* out_boards;
    int32_t* reward;
    uint32_t* draws;
    uint32_t* flags;
    uint32_t* legal;       // nullable
    int32_t* next_action;  // nullable
    uint32_t* ovf_count;
    uint32_t* ovf_list;
    uint32_t* bad_cells;   // nullable: set to 1 if a cell value lies outside [0, 127]
    int clear_ovf;         // k_apply_fix (one block) zeroes *ovf_count when done (zero-copy calls)
};
struct RolloutArgs {
    m3::Shape shape;
    int64_t n;
    const int8_t* boards;
    const uint32_t* seeds;     // cfg.seed of each state
    const int32_t* n_actions;
    const uint32_t* rseeds;    // rollout seed (random.randint(0, 2**31 - 1) or state.seed)
    int32_t* gain;             // sum of the step rewards of the rollout
    int32_t* steps;            // apply_action calls
    uint32_t* draws;           // global-stream draws since its last seed when the rollout ends
    uint32_t* flags;           // OR of the steps' M3_FLAG_*
    int8_t* out_boards;        // nullable: terminal boards
    uint32_t* counters;        // [0] overflow count, [1] spill records taken, [2] waves with a bad cell
    uint32_t* ovf_list;
    uint32_t* spill;
    uint32_t spill_cap;
};
}  // namespace m3k

namespace m3 {

constexpr int BLOCK = 256;
constexpr int FIX_BLOCK = 64;
constexpr int FIX_GRID = 16;       // step fixup almost never has work: few blocks schedule fast
constexpr int INIT_FIX_BLOCK = 64;
constexpr int INIT_BLOCK = 64;
// active lanes of the one-board-per-lane fix / reset kernels (KS::BPW: one for the 32 x 32 frame)
template <class CF>
constexpr uint32_t lanes_for() { return CF::W > 8 ? 1u : 64u; }
// 9x9: k_init redoes its few > 624-draw resets in-wave (wave_reset); 16x16
// resets go straight to k_init_fix_lane (most need >= 624 draws)
template <class CF>
constexpr bool INIT_INLINE_FIX = CF::N <= 128;
// The M3_* macros of the device sources are of three kinds only: numeric tunings that `make variant
// XFLAGS=-D...` varies (the #ifndef-guarded numbers, from here on, in m3_kernels.hpp and M3_TW9 /
// M3_LEGAL_SLICED_W in m3_rules.hpp), M3_FAST_MATCH (m3_rules.hpp: the host test compares both sides),
// and build structure / diagnostic builds (M3_SPLIT_TU, M3_INST, M3_PART, M3_HEADLINE_ONLY,
// M3_NO_WIDE_FRAME; M3_PHASE_PROF, M3_TEST_NO_GATHER_WAIT, M3_DEBUG_NO_PREFETCH). On/off switches of
// variants that were measured and rejected are not kept: DESIGN.md has their numbers, git history
// their code.
// k_init's lockstep draw budget when it may defer (env prefetch): 9x9x6 resets
// past 454 draws (~4 %: the third chain level and the second block) go to
// k_init_coop, so a wave no longer runs to its slowest lane's ~600 draws
#ifndef M3_RESET_KCAP
#define M3_RESET_KCAP 454
#endif
constexpr uint32_t RESET_KCAP = M3_RESET_KCAP;
// A reset stops after this many rounds of BoardV2.__init__'s redraw loop (boardv2.py:23-27) and
// flags M3_FLAG_RESET_CAP: only two-colour boards get near it (a 16x16x2 reset can need more than
// 10,000 rounds; the reference keeps going), and a GPU lane must end.
constexpr uint32_t RESET_ROUND_CAP = 1u << 14;

// M3_NSLOT: episode slots per board (A/B knob; at most 5: the counter blocks of m3_kernels.hpp).
// Round 6 A/B of 5 slots -- one more step of slack for the synchronised end-of-episode reset
// bursts: equal speed.
#ifndef M3_NSLOT
#define M3_NSLOT 4
#endif
constexpr int NSLOT = M3_NSLOT;     // episode slots per board (see EnvArgs)
static_assert(NSLOT >= 2 && NSLOT <= 255, "slot index is a byte");

// Per-shape step-kernel geometry: boards (lanes) per workgroup and the
// match-group table capacity, sized so staging + table fit the 160 KB LDS.
// One wave per workgroup: the boards of a wave are staged through its own LDS
// slice, so a wave that finishes early never waits at a barrier for the
// workgroup's slowest wave (cascade depth varies a lot between boards) and its
// slot is refilled at once.
template <class CF>
struct KS {
    static constexpr int B = 64;
    static_assert(B == 64, "one-wave workgroups: lds_sync() orders a single wave's LDS accesses");
    // match groups in LDS per lane (more spill to a global pool): 9x9 6 (9 KB per wave, +0.8 %,
    // gpurun_out/r05aj), 16x16 4 (past the staging area a larger table costs occupancy)
    static constexpr int GCAP = CF::N <= 128 ? 6 : 4;
    // boards per wave: 64 (one per lane), but ONE for the 32 x 32 frame. Those kernels carry
    // ~2,500 SGPR spills through VGPR lanes, and with several lanes active some boards came out
    // wrong only in company (32x32x8 steps: 92 of 689; each exact alone) -- the lane interference
    // DESIGN.md §4 describes for the 16 x 16 frame. One active lane per wave has no divergence.
    static constexpr int BPW = CF::W > 8 ? 1 : B;
#ifndef M3_STEP_WPS
#define M3_STEP_WPS 4
#endif
    // k_env_step waves per SIMD the register allocation is bounded for (16x16:
    // 2, with 708 B of spill, +7 % over 1 once resets stopped binding)
#ifndef M3_STEP_WPS16
#define M3_STEP_WPS16 2
#endif
    // frame shapes (run-time board shape, FCfg): 1 wave/SIMD. Their uniform shape masks take
    // ~100 SGPRs and spill into VGPR lanes; at 2 waves/SIMD those VGPRs spilled to scratch in
    // turn and divergent lanes of a wave corrupted each other's results (rollouts at 10x8x9,
    // tools/dbg); with 512 registers per lane nothing reaches scratch.
#ifndef M3_STEP_WPS_FRAME
#define M3_STEP_WPS_FRAME 1
#endif
    static constexpr int STEP_WPS = CF::DYN ? M3_STEP_WPS_FRAME : (CF::N > 128 ? M3_STEP_WPS16 : M3_STEP_WPS);
    // k_env_cont: bounded like the step kernel it runs beside (a 2-waves/SIMD
    // build without spills measured 4 % slower overall: its waves take register
    // file the other shard's step waves need)
#ifndef M3_CONT_WPS
#define M3_CONT_WPS M3_STEP_WPS
#endif
    static constexpr int CONT_WPS = CF::N > 128 ? 1 : M3_CONT_WPS;
    // spill pool records per shard (32 x 32 frame: a record is 86 KB; fewer, the rest recompute)
    static constexpr uint32_t SPILL_RECORDS = CF::W > 8 ? 256 : 4096;
    // The env step's RNG is the register-only MT19937 chain from the board's
    // (seed, mt[397]) -- 4 B of per-board state (a per-board stream cache of
    // the first raw outputs, built by the reset, measured equal at 9x9 and 2x
    // slower at 16x16; removed in round 3).
    // 16x16: one chain level (draws < 227; a step needing more -- a near-full
    // board refill -- goes to k_env_fix), five fewer VGPRs live through the
    // cascade, +2.5 %. 9x9: the full three-level chain; the one-level build
    // came out 16 % slower (A/B gpurun_out/ab3), the register allocation of
    // the 3-waves/SIMD bound shifts with it.
    using Chain = std::conditional_t<(CF::N > 128), ChainMT1, ChainMT>;
    using Rng = Chain;
    static constexpr int CHAIN_LIMIT = CF::N > 128 ? 227 : 624;  // draws the chain reaches
    static_assert(std::is_same_v<Chain, ChainMTT<(uint32_t)CHAIN_LIMIT>>, "CHAIN_LIMIT is Chain's");
#ifndef M3_CASCADE_LIMIT
#define M3_CASCADE_LIMIT 2
#endif
    // k_env_step runs at most this many cascade iterations per step (-1: no
    // bound); longer steps are finished by k_env_cont (see there)
    // (16x16: off -- the continuation launch cost more than it saved:
    // 0.364 vs 0.337 G env-steps/s at 1 wave/SIMD, 0.391 vs 0.384 at 2)
#ifndef M3_CASCADE_LIMIT16
#define M3_CASCADE_LIMIT16 -1
#endif
    static constexpr int CASCADE_LIMIT = CF::N > 128 ? M3_CASCADE_LIMIT16 : M3_CASCADE_LIMIT;
};

// words of one spill-pool record: the groups LCAP..MAXG-1 of one board (LdsStore, m3_kernels.hpp)
template <class CF, int LCAP = KS<CF>::GCAP>
constexpr int SPILL_REC_WORDS = (CF::MAXG - LCAP) * 2 * CF::W;

// records of the rollout spill pool (a lane keeps one spill record for its whole rollout): one per
// 8 rollouts (at least 4096), within 256 MB (a lane that finds the pool empty is replayed exactly
// by k_rollout_fix)
inline int64_t rollout_spill_cap(int64_t n, size_t words) {
    const int64_t budget = (int64_t)((256ull << 20) / (words * 4ull));
    const int64_t want = n / 8 > 4096 ? n / 8 : 4096;
    const int64_t cap = want < budget ? want : budget;
    return cap > 1 ? cap : 1;
}

// ---------------------------------------------------------------------------
// stateless apply (BoardV2 facade): m3_apply_actions
// ---------------------------------------------------------------------------
template <class CF>
M3_HD void store_legal(uint32_t* out, const uint32_t* act, const typename CF::Dim& dm = typename CF::Dim{}) {
#pragma unroll
    for (int i = 0; i < CF::AW; ++i)
        if (i < dm.aw()) out[i] = act[i];
}

// one full apply_action + outputs for board b; returns false on RNG overflow
template <class CF, class RNG, class Store>
M3_HD bool apply_and_emit(typename CF::Bd* P, const m3k::ApplyArgs& a, int64_t b, RNG& rng, Store& st,
                          const typename CF::Dim& dm) {
    typename CF::Bd HL, VL;
    uint32_t f;
    const int r = apply_action<CF>(P, a.n_actions[b], a.actions[b], rng, f, HL, VL, st, dm);
    if (f & FLAG_RECOMPUTE) return false;
    const bool stepped = !(f & (FLAG_TERMINAL | FLAG_BAD_ACTION));
    a.reward[b] = r;
    a.draws[b] = stepped ? rng.draws() : 0u;
    uint32_t act[CF::AW];
    action_bits<CF>(HL, VL, act, dm);
    int na = -1;
    if (stepped) {
        na = random_action<CF>(act, rng);
        if (rng.overflow) return false;
        if (na < 0) f |= FLAG_NO_LEGAL;
    }
    mark<PH_NEXT>(st);
    a.flags[b] = f;
    if (a.next_action) a.next_action[b] = na;
    if (a.legal) store_legal<CF>(a.legal + b * dm.aw(), act, dm);
    return true;
}

// ---------------------------------------------------------------------------
// env step: result codes and the continuation record of a paused step
// ---------------------------------------------------------------------------
enum : int { ENV_STEP_DONE = 0, ENV_STEP_RECOMPUTE = 1, ENV_STEP_PAUSED = 2 };

// internal: a continuation record of a settled board with no legal move (the
// row shuffle comes next), as opposed to one paused before a cascade iteration
constexpr uint32_t FLAG_CONT_DEAD = 0x80u;

// Continuation records of paused steps (KS::CASCADE_LIMIT): word 0 the
// shard-local board index, words 1.. the Cont state, padded to CONT_REC words
// (9x9x6: 32 words, 128 B) so a lane writes and reads its record with 16-byte
// accesses -- 8 instructions each way instead of one per word (round 5 wrote them
// SoA, word w of record q at cont[w * n + q]: 31 stores per wave). Record q at
// cont[q * CONT_REC]; the step's counter block [CNT_CONT] counts them.
template <class CF>
using EnvCont = Cont<CF, typename KS<CF>::Rng>;
template <class CF>
constexpr int CONT_REC = (1 + EnvCont<CF>::WORDS + 3) & ~3;

// ---------------------------------------------------------------------------
// batched MCTS rollouts (mctslib/standard/mcts.py:14-19)
// ---------------------------------------------------------------------------
// One rollout per lane: np.random.seed(rseed); while n_actions >= 1:
// action = choice(legal_actions) from the global stream, state =
// apply_action(action). The first choice reads the stream of rseed; every
// later one reads the stream apply_action left behind (cfg.seed reseeded at
// boardv2.py:46, advanced by the step's draws), i.e. the same register chain
// the step just used. The match-group table is the env's LDS table + spill
// pool, and a lane keeps its spill record for the whole rollout; a rollout
// that overflows the chain (>= 624 draws in one step) or the pool is
// replayed from its first move by k_rollout_fix.
template <class CF, class RNG, class Store>
M3_HD bool rollout_one(typename CF::Bd* P, const m3k::RolloutArgs& a, int64_t b, RNG& first, RNG& rng, Store& st,
                       const typename CF::Dim& dm) {
    int n = a.n_actions[b];
    int gain = 0, steps = 0;
    uint32_t fl = 0u, dr = 0u;
    if (n >= 1) {                                               // mcts.py:16 while not is_terminal
        typename CF::Bd HL, VL;
        legal_masks<CF>(P, special_mask<CF, CF::NP>(P), HL, VL, dm);
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
        int x = random_action<CF>(act, first);                  // mcts.py:17, stream of the rollout seed
        dr = first.draws();
        for (;;) {
            if (x < 0) {                                        // np.random.choice([]) raises
                fl |= FLAG_NO_LEGAL;
                break;
            }
            uint32_t f;
            const int r = apply_action<CF>(P, n, x, rng, f, HL, VL, st, dm);  // mcts.py:18
            if (f & FLAG_RECOMPUTE) return false;
            fl |= f;
            gain += r;
            ++steps;
            --n;
            dr = rng.draws();
            if (n < 1) break;
            action_bits<CF>(HL, VL, act, dm);
            x = random_action<CF>(act, rng);                    // stream where apply_action left it
            if (rng.overflow) return false;
            dr = rng.draws();
        }
    }
    a.gain[b] = gain;
    a.steps[b] = steps;
    a.draws[b] = dr;
    a.flags[b] = fl;
    return true;
}

}  // namespace m3
