// TEST-ONLY host build of the device rule code (element-crush-gym_amd/csrc/m3_rules.hpp) and of the
// batched paths' per-board code (m3_batch_core.hpp). The same __host__ __device__ functions the HIP
// kernels run are called here on the CPU so their logic can be differential-tested against the
// oracle in a GPU-less container: the stateless step is k_apply's apply_and_emit, a rollout is
// k_rollout's rollout_one, and the table capacity, chain and record layout of the env step come from
// KS<CF> / EnvCont<CF> (hc_geometry reports them to the tests). The env kernels' own cascade calls
// and their wave-level epilogue (m3_kernels.hpp) are restated in step_paused. Not part of the
// product; the product library never contains or calls this file.
//
// Shapes: cfg 0 = Cfg<9,9,6>, cfg 1 = Cfg<16,16,8> (the specialised kernels'
// configs), cfg 2 = the frame (FCfg: 16 x 16, or 32 x 32 for a side > 16) for
// the board set by hc_set_frame(rows, columns, types) -- any shape, including
// 9x9x6 / 16x16x8.
// The other lanes of the wave, for the code that runs in lockstep with them (wave_any): on the GPU a
// lane whose own vote is false keeps going while any other lane of its wave still votes true. Here
// the stand-in neighbour outvotes the lane g_neighbour_votes times (0: the lane is alone, as in
// every entry point but the reset ones that set it) -- in init_board_tiles each vote is one more
// 64-draw chunk generated behind the tiles the lane has not read yet, which is how a reset comes
// to overrun its tile ring.
static long g_neighbour_votes = 0;
static inline bool hc_wave_any(bool p) {
    if (p || g_neighbour_votes <= 0) return p;
    --g_neighbour_votes;
    return true;
}
#define M3_HOST_WAVE_ANY(p) hc_wave_any(p)
#include "../../element-crush-gym_amd/csrc/m3_batch_core.hpp"

#include <stdlib.h>
#include <string.h>

using namespace m3;

static int g_T = 6;
static Shape g_shape = make_shape(9, 9, 6);

template <class CF>
static typename CF::Dim make_dim() {
    return typename CF::Dim(g_shape);
}

template <class CF>
static void load_planes(const int8_t* b, typename CF::Bd* P, const typename CF::Dim& dm) {
    if constexpr (CF::DYN) {
        frame_from_bytes<CF>(reinterpret_cast<const uint8_t*>(b), P, dm);
    } else {
        uint32_t cw[(CF::N + 3) / 4];
        memset(cw, 0, sizeof(cw));
        memcpy(cw, b, CF::N);
        planes_from_words<CF>(cw, P);
    }
}
template <class CF>
static void store_planes(const typename CF::Bd* P, int8_t* b, const typename CF::Dim& dm) {
    if constexpr (CF::DYN) {
        frame_to_bytes<CF>(P, reinterpret_cast<uint8_t*>(b), dm);
    } else {
        uint32_t cw[(CF::N + 3) / 4];
        words_from_planes<CF>(P, cw);
        memcpy(b, cw, CF::N);
    }
}

// The exact pass behind every fast path (k_apply_fix): board i again from its bytes, with the full
// generator and the full group table.
template <class CF>
static void step_exact(typename CF::Bd* P, const m3k::ApplyArgs& a, long i, int& recomputed,
                       const typename CF::Dim& dm) {
    recomputed++;
    FullMT* fm = new FullMT;
    ArrayStore<CF>* as = new ArrayStore<CF>;
    load_planes<CF>(a.boards + i * dm.cells(), P, dm);
    fm->init(a.seeds[i], 0);
    apply_and_emit<CF>(P, a, i, *fm, *as, dm);
    delete fm;
    delete as;
}

// One apply_action + next random action of board i as k_apply runs it: apply_and_emit on the fast
// path (Chain + the caller's group table), the exact pass when that gives up.
template <class CF, class Chain = ChainMT, class Store>
static void step_one(typename CF::Bd* P, const m3k::ApplyArgs& a, long i, Store& st, int& recomputed,
                     const typename CF::Dim& dm) {
    Chain rng;
    rng.init(a.seeds[i], mt_state397(a.seeds[i]));
    if (!apply_and_emit<CF>(P, a, i, rng, st, dm)) step_exact<CF>(P, a, i, recomputed, dm);
}

// The env kernels' bounded cascade, with KS<CF>'s chain: k_env_step stops before inner iteration
// pause + 1 or at a dead board (before the row shuffle, marked FLAG_CONT_DEAD) and hands the state
// over through the EnvCont words; k_env_cont_grid restores it into fresh variables and finishes the
// cascade, dead boards from the shuffle on. Then the step's draws and the next random action as
// env_fin_begin takes them; a step past the chain or the table goes to the exact pass.
// Returns whether the step paused.
template <class CF, class Store>
static bool step_paused(typename CF::Bd* P, const m3k::ApplyArgs& a, long i, Store& st, int& recomputed,
                        const typename CF::Dim& dm, int pause) {
    typename CF::Bd HL, VL;
    typename KS<CF>::Rng rng;
    rng.init(a.seeds[i], mt_state397(a.seeds[i]));
    int r;
    uint32_t f;
    bool paused = false;
    if (apply_begin<CF>(P, a.n_actions[i], a.actions[i], rng, f, HL, VL, st, r, dm)) {
        const int c = apply_cascade_ex<CF, CASX_STOP_DEAD>(P, rng, f, HL, VL, st, r, pause, false, dm);
        if ((c == CAS_PAUSED || c == CAS_DEAD) && !(f & FLAG_RECOMPUTE)) {
            if (c == CAS_DEAD) f |= FLAG_CONT_DEAD;
            uint32_t rec[EnvCont<CF>::WORDS];
            EnvCont<CF>::save(P, rng, r, f, [&](int k, uint32_t w) { rec[k] = w; });
            typename CF::Bd Q[CF::NP];  // (fresh variables: only what the record holds comes back)
            typename KS<CF>::Rng g2;
            int r2;
            uint32_t f2;
            EnvCont<CF>::load(Q, g2, r2, f2, [&](int k) { return rec[k]; });
            memcpy(P, Q, sizeof(Q));
            rng = g2;
            r = r2;
            f = f2;
            const bool dead = (f & FLAG_CONT_DEAD) != 0;
            f &= ~FLAG_CONT_DEAD;
            apply_cascade_ex<CF, 0>(P, rng, f, HL, VL, st, r, -1, dead, dm);
            paused = true;
        }
    }
    if (!(f & FLAG_RECOMPUTE)) {
        const bool stepped = !(f & (FLAG_TERMINAL | FLAG_BAD_ACTION));
        a.reward[i] = r;
        a.flags[i] = f;
        a.draws[i] = stepped ? rng.draws() : 0u;  // apply_action's draws, before the next choice
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
        a.next_action[i] = stepped ? random_action<CF>(act, rng) : -1;  // (may pass the chain's reach too)
        if (rng.overflow) f |= FLAG_RNG_OVERFLOW;
        if (a.legal) store_legal<CF>(a.legal + i * dm.aw(), act, dm);
    }
    if (f & FLAG_RECOMPUTE) step_exact<CF>(P, a, i, recomputed, dm);
    return paused;
}

static long g_paused = 0;  // steps that paused in the bounded-cascade mode (hc_paused)

template <class CF>
static int apply_n(long n, const int8_t* boards, const uint32_t* seeds, const int32_t* nact, const int32_t* acts,
                   int8_t* out, int32_t* rew, int32_t* draws, int32_t* flags, uint32_t* legal, int32_t* next_act,
                   int small) {
    const auto dm = make_dim<CF>();
    m3k::ApplyArgs a{};  // the rows are the caller's arrays
    a.n = n;
    a.boards = boards;
    a.seeds = seeds;
    a.n_actions = nact;
    a.actions = acts;
    a.reward = rew;
    a.draws = reinterpret_cast<uint32_t*>(draws);
    a.flags = reinterpret_cast<uint32_t*>(flags);
    a.legal = legal;
    a.next_action = next_act;
    int recomputed = 0;
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP];
        load_planes<CF>(boards + i * dm.cells(), P, dm);
        if (small >= 100 && small < 120) {  // bounded cascade, paused after small - 100 iterations and resumed
            SmallStore<CF, 4> ss;
            g_paused += step_paused<CF>(P, a, i, ss, recomputed, dm, small - 100);
        } else if (small == 32) {  // the env step's chain (16x16 / frame: one level, < 227 draws) + 4-group table
            SmallStore<CF, 4> ss;
            step_one<CF, typename KS<CF>::Chain>(P, a, i, ss, recomputed, dm);
        } else if (small == 8) {
            SmallStore<CF, 8> ss;
            step_one<CF>(P, a, i, ss, recomputed, dm);
        } else if (small == 4) {
            SmallStore<CF, 4> ss;
            step_one<CF>(P, a, i, ss, recomputed, dm);
        } else if (small) {
            SmallStore<CF, 1> ss;
            step_one<CF>(P, a, i, ss, recomputed, dm);
        } else {
            ArrayStore<CF>* as = new ArrayStore<CF>;
            step_one<CF>(P, a, i, *as, recomputed, dm);
            delete as;
        }
        // apply_action's flags: FLAG_NO_LEGAL is apply_and_emit's own, for the next action it could
        // not draw, which next_act = -1 reports here
        flags[i] &= ~(int32_t)(FLAG_RECOMPUTE | FLAG_NO_LEGAL);
        store_planes<CF>(P, out + i * dm.cells(), dm);
    }
    return recomputed;
}

// BoardV2.__init__ the way the kernels do it: 9x9 -- tile stream on the
// ChainMT (init_board_tiles), FullMT on overflow (k_init); frame -- FullMT
// rounds (k_init_fix_lane's fill_round_frame).
template <class CF>
static int init_n(long n, const uint32_t* seeds, int8_t* out, int32_t* draws, uint32_t* m397, int32_t* first_act) {
    const auto dm = make_dim<CF>();
    int recomputed = 0;
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP], HL, VL;
        m397[i] = mt_state397(seeds[i]);
        bool ok = false;
        if constexpr (!CF::DYN) {
            static uint32_t tm[CF::BITS * TileGen<CF>::TWMAX], pos[TileGen<CF>::MAXR];
            ChainMT cm;
            cm.init(seeds[i], m397[i]);
            uint32_t d = 0;
            ok = init_board_tiles<CF>(P, cm, tm, pos, 1, d, 0u, [](uint32_t, uint32_t) {}, [](uint32_t, uint32_t) {});
            draws[i] = (int32_t)d;
        }
        if (!ok) {
            if (!CF::DYN) recomputed++;
            FullMT* fm = new FullMT;
            fm->init(seeds[i], 0);
            if constexpr (CF::DYN) {
                for (int p = 0; p < CF::NP; ++p) P[p] = CF::Bd::zero();
                typename CF::Bd mask;
                fill_round_frame<CF>(P, *fm, nullptr, dm);
                while (get_match_mask<CF>(P, mask)) fill_round_frame<CF>(P, *fm, &mask, dm);
                recomputed += fm->k >= 624u;
            } else {
                { NoStore ns; init_board<CF>(P, *fm, ns, dm); }
            }
            draws[i] = (int32_t)fm->k;
            delete fm;
        }
        legal_masks<CF>(P, special_mask<CF, CF::NP>(P), HL, VL, dm);
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
        ChainMT rng;
        rng.init(seeds[i], m397[i]);
        first_act[i] = random_action<CF>(act, rng);
        store_planes<CF>(P, out + i * dm.cells(), dm);
    }
    return recomputed;
}

// BoardV2.__init__ through the scalar init_board (both forms), to cross-check the kernels' forms.
template <class CF>
static void init_scalar_n(long n, const uint32_t* seeds, int8_t* out, int32_t* draws) {
    const auto dm = make_dim<CF>();
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP];
        FullMT* fm = new FullMT;
        fm->init(seeds[i], 0);
        { NoStore ns; init_board<CF>(P, *fm, ns, dm); }
        draws[i] = (int32_t)fm->k;
        delete fm;
        store_planes<CF>(P, out + i * dm.cells(), dm);
    }
}

// init_board_tiles alone, one lane, draws capped at kcap (the env prefetch's deferral boundary,
// RESET_KCAP in k_init<CF, false>): ok[i] = what it returned; a reset it gave up (past kcap, or its
// unread tiles would overrun the ring) is redone on FullMT only with `fallback`, else left zero.
// neighbour: 64-draw chunks a busier lane of the same wave makes this one generate ahead (above).
// tm / pos are exactly the ring's size, so the sanitizer build sees any index past it.
template <class CF>
static int tiles_n(long n, const uint32_t* seeds, uint32_t kcap, int fallback, int neighbour, int8_t* out,
                   int32_t* draws, uint8_t* okv) {
    using C9B = Cfg<CF::R, CF::C, CF::T>;  // (same planes; CF may only differ in its TileGen)
    const auto dm = make_dim<C9B>();
    int gave_up = 0;
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP];
        uint32_t tm[CF::BITS * TileGen<CF>::TWMAX], pos[TileGen<CF>::MAXR];
        memset(tm, 0, sizeof(tm));
        memset(pos, 0, sizeof(pos));
        ChainMT cm;
        cm.init(seeds[i], mt_state397(seeds[i]));
        uint32_t d = 0;
        g_neighbour_votes = neighbour;
        const bool ok = init_board_tiles<CF>(P, cm, tm, pos, 1, d, 0u, [](uint32_t, uint32_t) {},
                                             [](uint32_t, uint32_t) {}, (NoStore*)nullptr, kcap);
        g_neighbour_votes = 0;
        okv[i] = (uint8_t)ok;
        draws[i] = ok ? (int32_t)d : 0;
        if (!ok) {
            gave_up++;
            for (int p = 0; p < CF::NP; ++p) P[p] = CF::Bd::zero();
            if (fallback) {
                FullMT* fm = new FullMT;
                fm->init(seeds[i], 0);
                { NoStore ns; init_board<C9B>(P, *fm, ns, dm); }
                draws[i] = (int32_t)fm->k;
                delete fm;
            }
        }
        store_planes<C9B>(P, out + i * dm.cells(), dm);
    }
    return gave_up;
}

template <class CF>
static void legal_n(long n, const int8_t* boards, uint32_t* out) {
    const auto dm = make_dim<CF>();
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP], HL, VL;
        load_planes<CF>(boards + i * dm.cells(), P, dm);
        legal_masks<CF>(P, special_mask<CF, CF::NP>(P), HL, VL, dm);
        uint32_t act[CF::AW];
        action_bits<CF>(HL, VL, act, dm);
        memcpy(out + i * dm.aw(), act, sizeof(uint32_t) * dm.aw());
    }
}

template <class CF>
static void matches_n(long n, const int8_t* tbs, uint8_t* mask, int32_t* spawn, int32_t* found) {
    const auto dm = make_dim<CF>();
    const int N = dm.cells();
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP], mk, sw[3];
        load_planes<CF>(tbs + i * N, P, dm);
        ArrayStore<CF>* as = new ArrayStore<CF>;
        found[i] = get_matches<CF>(P, mk, sw, *as);
        delete as;
        for (int x = 0; x < N; ++x) {
            const int fx = (x / dm.cols()) * CF::C + x % dm.cols();
            mask[i * N + x] = (uint8_t)mk.test(fx);
            int v = (int)sw[0].test(fx) * CF::H + (int)sw[1].test(fx) * CF::V + (int)sw[2].test(fx) * CF::M;
            if (sw[0].test(fx) && sw[1].test(fx)) v = CF::B;
            spawn[i * N + x] = v;
        }
    }
}

template <class CF>
static void roundtrip_n(long n, const int8_t* boards, int8_t* out) {
    const auto dm = make_dim<CF>();
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP];
        load_planes<CF>(boards + i * dm.cells(), P, dm);
        store_planes<CF>(P, out + i * dm.cells(), dm);
    }
}

// Phase counter (profiling hook of m3_rules.hpp): how many cascade rounds a step runs.
template <class CF>
struct CountStore : ArrayStore<CF> {
    static constexpr bool PROF = true;
    int rounds = 0;
    template <int K>
    void mark() {
        if (K == PH_REFILL) ++rounds;
    }
};

template <class CF>
static void rounds_n(long n, const int8_t* boards, const uint32_t* seeds, const int32_t* nact, const int32_t* acts,
                     int32_t* rounds) {
    const auto dm = make_dim<CF>();
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP], HL, VL;
        load_planes<CF>(boards + i * dm.cells(), P, dm);
        FullMT* fm = new FullMT;
        fm->init(seeds[i], 0);
        CountStore<CF>* cs = new CountStore<CF>;
        uint32_t f;
        apply_action<CF>(P, nact[i], acts[i], *fm, f, HL, VL, *cs, dm);
        rounds[i] = cs->rounds;
        delete fm;
        delete cs;
    }
}

// MCTS.rollout (mctslib/standard/mcts.py:14-19): k_rollout's rollout_one with k_rollout's chain
// (KS<CF>::Chain), one board at a time. Writes gain, steps, draws (global-stream position when the
// rollout ends), flags; -1 gain when the chain ran out (the kernel's k_rollout_fix replay). The group
// table is the full one (ArrayStore), so a board with many groups (tests/crafted.py) is played here
// and not given up.
template <class CF>
static void rollout_n(long n, const int8_t* boards, const uint32_t* seeds, const int32_t* nact, const uint32_t* rseeds,
                      int32_t* gain, int32_t* steps, uint32_t* draws, uint32_t* flags) {
    const auto dm = make_dim<CF>();
    m3k::RolloutArgs a{};
    a.n = n;
    a.n_actions = nact;
    a.gain = gain;
    a.steps = steps;
    a.draws = draws;
    a.flags = flags;
    ArrayStore<CF>* st = new ArrayStore<CF>;
    for (long i = 0; i < n; ++i) {
        typename CF::Bd P[CF::NP];
        load_planes<CF>(boards + i * dm.cells(), P, dm);
        typename KS<CF>::Chain first, rng;
        first.init(rseeds[i], mt_state397(rseeds[i]));
        rng.init(seeds[i], mt_state397(seeds[i]));
        gain[i] = steps[i] = 0;
        draws[i] = flags[i] = 0u;
        if (!rollout_one<CF>(P, a, i, first, rng, *st, dm)) gain[i] = -1;
    }
    delete st;
}

// what the kernels of a configuration are built with (hc_geometry)
enum { GEO_GCAP, GEO_CHAIN_LIMIT, GEO_SPILL_RECORDS, GEO_FIX_LANES, GEO_NSLOT, GEO_RESET_KCAP, GEO_BPW,
       GEO_CASCADE_LIMIT, GEO_SPILL_WORDS };
template <class CF>
static long geometry(int what) {
    using K = KS<CF>;
    switch (what) {
        case GEO_GCAP: return K::GCAP;
        case GEO_CHAIN_LIMIT: return K::CHAIN_LIMIT;
        case GEO_SPILL_RECORDS: return K::SPILL_RECORDS;
        case GEO_FIX_LANES: return FIX_GRID * (long)lanes_for<CF>();
        case GEO_NSLOT: return NSLOT;
        case GEO_RESET_KCAP: return RESET_KCAP;
        case GEO_BPW: return K::BPW;
        case GEO_CASCADE_LIMIT: return K::CASCADE_LIMIT;
        case GEO_SPILL_WORDS: return SPILL_REC_WORDS<CF>;
    }
    return -1000;
}

using C9 = Cfg<9, 9, 6>;
using C16 = Cfg<16, 16, 8>;
// 9x9x6 on a 7-word tile ring: 32 * (7 - W - 1) = 96 usable tiles, where the shipped 10 words give
// 192. Most single-lane resets then overrun the ring (a round's 81 tiles plus what the 64-draw chunk
// behind them accepted), so init_board_tiles' ring_full exit -- unreachable at test sizes with the
// shipped ring -- runs here, next to resets that complete on the small ring.
struct C9Ring7 : C9 {};
namespace m3 {
template <>
struct TileGen<C9Ring7> {
    static constexpr int TWMAX = 7;
    static constexpr int MAXR = TileGen<C9>::MAXR;
    static_assert(TWMAX > C9::W + 1, "a round's read window fits the ring");
    static M3_HD uint32_t slot(uint32_t q) { return q % (uint32_t)TWMAX; }
};
}  // namespace m3
// HC_NO_WIDE=1: no 32 x 32-frame instantiations (the MemorySanitizer build: with them its -O0
// compile needs ~40 GB and most of an hour)
#ifndef HC_NO_WIDE
#define HC_NO_WIDE 0
#endif
#define M3_F32(b) FCfg<b, 32>

#define DISPATCH(cfg, call)                        \
    do {                                           \
        if (cfg == 0) {                            \
            call(C9);                              \
        } else if (cfg == 1) {                     \
            call(C16);                             \
        } else {                                   \
            const int bits_ = bits_for_types(g_T); \
            const bool wide_ = g_shape.fs == 32;   \
            if (bits_ == 2 && !wide_) {            \
                call(FCfg<2>);                     \
            } else if (bits_ == 3 && !wide_) {     \
                call(FCfg<3>);                     \
            } else if (bits_ == 4 && !wide_) {     \
                call(FCfg<4>);                     \
            } else if (!wide_) {                   \
                call(FCfg<5>);                     \
            } else if (HC_NO_WIDE) {               \
                abort();                           \
            } else if (bits_ == 2) {               \
                call(M3_F32(2));                   \
            } else if (bits_ == 3) {               \
                call(M3_F32(3));                   \
            } else if (bits_ == 4) {               \
                call(M3_F32(4));                   \
            } else {                               \
                call(M3_F32(5));                   \
            }                                      \
        }                                          \
    } while (0)

// ArrayStore that records whether the scan touched it (get_matches' loop-free path never does)
template <class CF>
struct TrapStore : ArrayStore<CF> {
    bool used = false;
    bool put(int g, const typename CF::Bd& hh, const typename CF::Bd& vv) {
        used = true;
        return ArrayStore<CF>::put(g, hh, vv);
    }
};

extern "C" {
int hc_set_frame(int rows, int columns, int types) {
    if (rows < 3 || rows > MAX_FRAME || columns < 3 || columns > MAX_FRAME || types < 2 || types > 31) return -1;
    g_T = types;
    g_shape = make_shape(rows, columns, types);
    return 0;
}
int hc_apply(int cfg, long n, const int8_t* b, const uint32_t* s, const int32_t* na, const int32_t* a, int8_t* o,
             int32_t* r, int32_t* d, int32_t* f, uint32_t* legal, int32_t* next_act, int small) {
    int rc = 0;
#define CALL(CF) rc = apply_n<CF>(n, b, s, na, a, o, r, d, f, legal, next_act, small)
    DISPATCH(cfg, CALL);
#undef CALL
    return rc;
}
int hc_init(int cfg, long n, const uint32_t* s, int8_t* o, int32_t* d, uint32_t* m397, int32_t* fa) {
    int rc = 0;
#define CALL(CF) rc = init_n<CF>(n, s, o, d, m397, fa)
    DISPATCH(cfg, CALL);
#undef CALL
    return rc;
}
// 9x9x6 init_board_tiles with the draw cap of the caller's choice and no fallback behind it:
// ok[i] = its return value, board and draws only where ok (zero elsewhere). Returns the resets given up.
int hc_init9_kcap(long n, const uint32_t* s, uint32_t kcap, int neighbour, int8_t* o, int32_t* d, uint8_t* ok) {
    if (kcap > 624u || neighbour < 0) return -1;
    return tiles_n<C9>(n, s, kcap, 0, neighbour, o, d, ok);
}
// 9x9x6 resets on the 7-word ring (C9Ring7), the given-up ones redone exactly (FullMT) as the
// kernels do; ok[i] = init_board_tiles' own return value. Returns the resets that fell back.
int hc_init9_ring7(long n, const uint32_t* s, int neighbour, int8_t* o, int32_t* d, uint8_t* ok) {
    if (neighbour < 0) return -1;
    return tiles_n<C9Ring7>(n, s, 624u, 1, neighbour, o, d, ok);
}
int hc_init_scalar(int cfg, long n, const uint32_t* s, int8_t* o, int32_t* d) {
#define CALL(CF) init_scalar_n<CF>(n, s, o, d)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
int hc_legal(int cfg, long n, const int8_t* b, uint32_t* out) {
#define CALL(CF) legal_n<CF>(n, b, out)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
int hc_matches(int cfg, long n, const int8_t* b, uint8_t* m, int32_t* sp, int32_t* fd) {
#define CALL(CF) matches_n<CF>(n, b, m, sp, fd)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
int hc_roundtrip(int cfg, long n, const int8_t* b, int8_t* o) {
#define CALL(CF) roundtrip_n<CF>(n, b, o)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
int hc_rounds(int cfg, long n, const int8_t* b, const uint32_t* s, const int32_t* na, const int32_t* a, int32_t* r) {
#define CALL(CF) rounds_n<CF>(n, b, s, na, a, r)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
int hc_rollout(int cfg, long n, const int8_t* b, const uint32_t* s, const int32_t* na, const uint32_t* rs,
               int32_t* gain, int32_t* steps, uint32_t* draws, uint32_t* flags) {
#define CALL(CF) rollout_n<CF>(n, b, s, na, rs, gain, steps, draws, flags)
    DISPATCH(cfg, CALL);
#undef CALL
    return 0;
}
// one constant of the configuration's kernels (GEO_*); -1000: no such constant
long hc_geometry(int cfg, int what) {
    long rc = 0;
#define CALL(CF) rc = geometry<CF>(what)
    DISPATCH(cfg, CALL);
#undef CALL
    return rc;
}
// records of the spill pool of a launch of n rollouts
long hc_rollout_spill_cap(int cfg, long n) {
    long rc = 0;
#define CALL(CF) rc = (long)rollout_spill_cap(n, (size_t)SPILL_REC_WORDS<CF>)
    DISPATCH(cfg, CALL);
#undef CALL
    return rc;
}
long hc_paused(int reset) {
    const long v = g_paused;
    if (reset) g_paused = 0;
    return v;
}
// boards whose match mask differs between the fast path and the sequential scan
long hc_mask_mismatches(int cfg, long n, const int8_t* b) {
    long bad = 0;
#define CALL(CF)                                                                   \
    for (long i = 0; i < n; ++i) {                                                 \
        typename CF::Bd P[CF::NP], m1, m2;                                         \
        const typename CF::Dim dm_ = make_dim<CF>();                               \
        load_planes<CF>(b + i * dm_.cells(), P, dm_);                              \
        const bool a1 = get_match_mask<CF>(P, m1);                                 \
        const bool a2 = get_match_mask_scan<CF>(P, m2);                            \
        bool same = a1 == a2;                                                      \
        for (int w = 0; w < CF::W; ++w) same = same && m1.w[w] == m2.w[w];         \
        bad += !same;                                                              \
    }
    DISPATCH(cfg, CALL);
#undef CALL
    return bad;
}
// boards where get_matches (with its loop-free path, M3_FAST_MATCH) differs from the sequential
// scan in the mask, the spawn planes or the result; *fast counts the boards the loop-free path took
long hc_fast_match_mismatches(int cfg, long n, const int8_t* b, long* fast) {
    long bad = 0, nf = 0;
#define CALL(CF)                                                                           \
    for (long i = 0; i < n; ++i) {                                                         \
        using Bd_ = typename CF::Bd;                                                       \
        Bd_ P[CF::NP], m1, m2, s1[3], s2[3];                                               \
        const typename CF::Dim dm_ = make_dim<CF>();                                       \
        load_planes<CF>(b + i * dm_.cells(), P, dm_);                                      \
        TrapStore<CF>* ts = new TrapStore<CF>;                                             \
        ArrayStore<CF>* as = new ArrayStore<CF>;                                           \
        const int r1 = get_matches<CF>(P, m1, s1, *ts);                                    \
        const int r2 = match_scan<CF, true>(P, m2, s2, *as);                               \
        nf += r1 == MATCH_FOUND && !ts->used;                                              \
        delete as;                                                                         \
        delete ts;                                                                         \
        bool same = r1 == r2;                                                              \
        if (r1 == MATCH_FOUND)                                                             \
            for (int w = 0; w < CF::W; ++w)                                                \
                same = same && m1.w[w] == m2.w[w] && s1[0].w[w] == s2[0].w[w] &&           \
                       s1[1].w[w] == s2[1].w[w] && s1[2].w[w] == s2[2].w[w];               \
        bad += !same;                                                                      \
    }
    DISPATCH(cfg, CALL);
#undef CALL
    *fast = nf;
    return bad;
}
// first n raw outputs via ChainMT2 (the two-block register chain); -1 once it overflowed
int hc_chain2_raw(uint32_t seed, int n, uint32_t* out) {
    ChainMT2 g;
    g.init(seed, mt_state397(seed));
    for (int i = 0; i < n; ++i) out[i] = g.next32();
    return g.overflow ? -1 : 0;
}
uint32_t hc_chain_draw(uint32_t seed, int k) {  // k-th raw output (0-based) via ChainMT
    ChainMT g;
    g.init(seed, mt_state397(seed));
    uint32_t v = 0;
    for (int i = 0; i <= k; ++i) v = g.next32();
    return g.overflow ? 0xFFFFFFFFu : v;
}
}
