// TEST-ONLY host build of the 9x9x6 refill (element-crush-gym_amd/csrc/m3_rules.hpp): the two-part
// refill the kernels run (refill: generation loop + refill_place) next to the tile-by-tile
// refill_loop it replaced, on the same board, hole set and generator position. Also seeded episodes
// that record the size of every refill, for the share of refills that fall back to refill_loop.
// Not part of the product.
#include <stdint.h>

static uint32_t* g_need_out = nullptr;  // the sizes of one step's refills, in order
static int g_need_n = 0, g_need_cap = 0;
static inline void rf_hook(uint32_t need) {
    if (g_need_out && g_need_n < g_need_cap) g_need_out[g_need_n] = need;
    ++g_need_n;
}
#define M3_HOST_REFILL_HOOK(need) rf_hook(need)
#include "../../element-crush-gym_amd/csrc/m3_rules.hpp"

#include <string.h>

using namespace m3;
using C9 = Cfg<9, 9, 6>;

static uint32_t rf_lcg(uint32_t* s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

// a board around the holes: tiles 1..6, one cell in twelve a special (planes 3..5), holes 0
static void base_board(uint32_t s, const C9::Bd& em, C9::Bd* P) {
    for (int p = 0; p < C9::NP; ++p) P[p] = C9::Bd::zero();
    for (int x = 0; x < C9::N; ++x) {
        int v = 1 + (int)(rf_lcg(&s) % 6u);
        if (rf_lcg(&s) % 12u == 0u) v |= (int)(8u << (rf_lcg(&s) % 3u));
        if (!em.test(x)) set_cell<C9, C9::NP>(P, x, v);
    }
}

template <class Chain>
static void refill_one(int which, const uint32_t* em3, uint32_t seed, uint32_t k0, uint32_t* planes, uint32_t* k_out,
                       uint32_t* ovf_out) {
    C9::Bd em, P[C9::NP];
    for (int i = 0; i < C9::W; ++i) em.w[i] = em3[i];
    base_board(seed * 2654435761u + k0, em, P);
    Chain rng;
    rng.init(seed, mt_state397(seed));
    for (uint32_t i = 0; i < k0; ++i) rng.next32();
    if (which == 0) refill<C9>(P, em, rng);
    else refill_loop<C9>(P, em, rng);
    for (int p = 0; p < C9::NP; ++p)
        for (int i = 0; i < C9::W; ++i) planes[p * C9::W + i] = P[p].w[i];
    *k_out = rng.k;
    *ovf_out = rng.overflow;
}

extern "C" {

// which: 0 = refill, 1 = refill_loop; limit: 624 (ChainMT, the 9x9x6 kernels' generator) or 227 (ChainMT1).
// em: n x 3 words, top-aligned; planes: n x 7 x 3 words out.
int rf_refill(int which, int limit, long n, const uint32_t* em, const uint32_t* seeds, const uint32_t* k0,
              uint32_t* planes, uint32_t* k_out, uint32_t* ovf_out) {
    if (limit != 227 && limit != 624) return -1;
    for (long i = 0; i < n; ++i) {
        if (k0[i] > (uint32_t)limit) return -2;
        uint32_t* pl = planes + i * C9::NP * C9::W;
        if (limit == 227) refill_one<ChainMT1>(which, em + 3 * i, seeds[i], k0[i], pl, k_out + i, ovf_out + i);
        else refill_one<ChainMT>(which, em + 3 * i, seeds[i], k0[i], pl, k_out + i, ovf_out + i);
    }
    return 0;
}

// The tiles of the first `cap` refills of one step per board (boards: n x 81 cell values), 0 = no such refill.
int rf_step_refills(long n, const int8_t* boards, const uint32_t* seeds, const int32_t* actions, int cap,
                    uint32_t* need) {
    const C9::Dim dm;
    auto* as = new ArrayStore<C9>;
    memset(need, 0, sizeof(uint32_t) * (size_t)n * cap);
    for (long b = 0; b < n; ++b) {
        C9::Bd P[C9::NP], HL, VL;
        uint32_t cw[(C9::N + 3) / 4];
        memset(cw, 0, sizeof(cw));
        memcpy(cw, boards + b * C9::N, C9::N);
        planes_from_words<C9>(cw, P);
        ChainMT rng;
        rng.init(seeds[b], mt_state397(seeds[b]));
        uint32_t f = 0u;
        g_need_out = need + b * cap;
        g_need_n = 0;
        g_need_cap = cap;
        apply_action<C9>(P, 20, actions[b], rng, f, HL, VL, *as, dm);
        g_need_out = nullptr;
    }
    delete as;
    return 0;
}

// Seeded episodes the way the env runs them (BoardV2(seed), then `moves` seeded random actions, no
// autoreset): need[(b * moves + m) * cap + j] = the tiles of move m's j-th refill (0: no such refill).
// Returns the number of steps that left the chain's reach (their refills are not recorded).
long rf_episode_refills(long n, const uint32_t* seeds, int moves, int cap, uint32_t* need) {
    long redone = 0;
    const C9::Dim dm;
    auto* fm = new FullMT;
    auto* as = new ArrayStore<C9>;
    memset(need, 0, sizeof(uint32_t) * (size_t)n * moves * cap);
    for (long b = 0; b < n; ++b) {
        C9::Bd P[C9::NP], HL, VL;
        const uint32_t m397 = mt_state397(seeds[b]);
        fm->init(seeds[b], 0);
        { NoStore ns; init_board<C9>(P, *fm, ns, dm); }
        legal_masks<C9>(P, special_mask<C9, C9::NP>(P), HL, VL, dm);
        uint32_t act[C9::AW];
        action_bits<C9>(HL, VL, act, dm);
        ChainMT rng;
        rng.init(seeds[b], m397);
        int action = random_action<C9>(act, rng);
        for (int m = 0; m < moves && action >= 0; ++m) {
            C9::Bd Q[C9::NP];
            memcpy(Q, P, sizeof(Q));
            const int cur = action;
            uint32_t f = 0u;
            rng.init(seeds[b], m397);
            g_need_out = need + (b * moves + m) * cap;
            g_need_n = 0;
            g_need_cap = cap;
            apply_action<C9>(P, moves - m, cur, rng, f, HL, VL, *as, dm);
            g_need_out = nullptr;
            if (!(f & FLAG_RECOMPUTE)) {
                action_bits<C9>(HL, VL, act, dm);
                action = random_action<C9>(act, rng);
                if (rng.overflow) f |= FLAG_RNG_OVERFLOW;
            }
            if (f & FLAG_RECOMPUTE) {
                ++redone;
                memset(need + (b * moves + m) * cap, 0, sizeof(uint32_t) * cap);
                memcpy(P, Q, sizeof(Q));
                f = 0u;
                fm->init(seeds[b], 0);
                apply_action<C9>(P, moves - m, cur, *fm, f, HL, VL, *as, dm);
                action_bits<C9>(HL, VL, act, dm);
                action = random_action<C9>(act, *fm);
            }
            if (f & (FLAG_TERMINAL | FLAG_BAD_ACTION)) break;
        }
    }
    delete fm;
    delete as;
    return redone;
}

}  // extern "C"
