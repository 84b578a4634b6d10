// asan_main.hip -- TEST INFRASTRUCTURE ONLY: the two-part 9x9x6 refill's host build
// (refill_host.hip) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.
// The hazard of the bit code is a shift by 32 or more (a stream of exactly 32 tiles, a column
// offset of 32, row 8 of a late column): UBSan's shift check stops on any. The cases are those of
// tests/test_refill_cpu.py: random top-aligned hole sets at random generator positions, exactly
// 0 / 1 / 32 / 33 / 81 holes, one full column, refills that cross draw 227 and refills that reach
// the 624-draw limit; refill must equal refill_loop. Built and run by tests/test_refill_cpu.py.
#include "refill_host.hip"

#include <stdio.h>

static void heights_to_em(const int* h, uint32_t* em) {
    em[0] = em[1] = em[2] = 0u;
    for (int c = 0; c < 9; ++c)
        for (int r = 0; r < h[c]; ++r) {
            const int x = r * 9 + c;
            em[x >> 5] |= 1u << (x & 31);
        }
}

static long g_checks = 0, g_fallback = 0, g_overflow = 0;

static int check(const int* h, uint32_t seed, uint32_t k0, int limit) {
    uint32_t em[3], a[21], b[21], ka, kb, oa, ob;
    heights_to_em(h, em);
    if (rf_refill(0, limit, 1, em, &seed, &k0, a, &ka, &oa)) return 1;
    if (rf_refill(1, limit, 1, em, &seed, &k0, b, &kb, &ob)) return 1;
    int bad = ka != kb || oa != ob;
    if (!oa) bad |= memcmp(a, b, sizeof(a)) != 0;  // an overflowed step is recomputed from scratch
    if (bad) {
        fprintf(stderr, "mismatch: heights");
        for (int c = 0; c < 9; ++c) fprintf(stderr, " %d", h[c]);
        fprintf(stderr, " seed %u k0 %u limit %d: k %u/%u overflow %u/%u\n", seed, k0, limit, ka, kb, oa, ob);
        return 1;
    }
    int n = 0;
    for (int c = 0; c < 9; ++c) n += h[c];
    ++g_checks;
    g_fallback += n > 32;
    g_overflow += oa;
    return 0;
}

// n holes, spread left to right as evenly as the column height allows
static void spread(int n, int first, int* h) {
    for (int c = 0; c < 9; ++c) h[c] = 0;
    for (int c = first; n > 0; c = (c + 1) % 9)
        if (h[c] < 9) {
            ++h[c];
            --n;
        }
}

int main() {
    uint32_t rs = 2024u;
    int h[9];
    for (int i = 0; i < 20000; ++i) {
        for (int c = 0; c < 9; ++c) h[c] = (int)(rf_lcg(&rs) % 10u);
        if (i % 3 == 0)  // small refills, the common case on the GPU
            for (int c = 0; c < 9; ++c) h[c] = h[c] > 3 ? 0 : h[c];
        const uint32_t seed = rf_lcg(&rs) * 977u + 1u, k0 = rf_lcg(&rs) % 201u;
        if (check(h, seed, k0, (i & 1) ? 227 : 624)) return 1;
    }
    for (int limit : {227, 624})
        for (uint32_t seed = 1; seed <= 40u; ++seed) {
            for (int n : {0, 1, 31, 32, 33, 80, 81})
                for (int first : {0, 4, 8}) {
                    spread(n, first, h);
                    if (check(h, seed, seed % 7u, limit)) return 1;
                }
            for (int c = 0; c < 9; ++c) {  // one full column; and the columns from c on full (32 holes: off = 32)
                for (int d = 0; d < 9; ++d) h[d] = d == c ? 9 : 0;
                if (check(h, seed, 3u * seed, limit)) return 1;
                for (int d = 0; d < 9; ++d) h[d] = d >= c ? 9 : 0;
                if (check(h, seed, seed, limit)) return 1;
            }
            const int last_full[9] = {4, 4, 4, 4, 4, 3, 0, 0, 9};  // 32 holes, row 8 of the last column is tile 31
            if (check(last_full, seed, 0u, limit)) return 1;
            // across draw 227, and (three-level chain) into the 624-draw limit
            for (uint32_t k0 : {190u, 200u, 215u, 226u, 227u}) {
                spread(30, (int)(seed % 9u), h);
                if (check(h, seed, k0, limit)) return 1;
            }
            if (limit == 624)
                for (uint32_t k0 : {440u, 453u, 454u, 590u, 600u, 615u, 623u, 624u}) {
                    spread(24 + (int)(seed % 9u), (int)(seed % 9u), h);
                    if (check(h, seed, k0, limit)) return 1;
                }
        }
    if (!g_fallback || !g_overflow) return 2;
    printf("refill_host asan: %ld checks ok (%ld of more than 32 holes, %ld overflowed)\n", g_checks, g_fallback,
           g_overflow);
    return 0;
}
