// asan_main.hip -- TEST INFRASTRUCTURE ONLY: the lookahead core's host build (lookahead_host.hip)
// under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program. Seeded boards with
// sprinkled specials, terminal boards, every group size 1..64 on a ragged tail, the specialised
// shapes and frame shapes; the result must not depend on the boards per wave. Built and run by
// tests/test_lookahead_cpu.py; any sanitizer report exits non-zero.
#include "lookahead_host.hip"

#include <stdio.h>

static uint32_t lcg(uint32_t* s) {
    *s = *s * 1664525u + 1013904223u;
    return *s >> 8;
}

static int run(int cfg, int R, int C, int T, uint32_t& rs, long& checks) {
    const long n = 37;
    const int N = R * C, A = R * (C - 1) * 2;
    std::vector<int8_t> boards(n * N);
    std::vector<uint32_t> seeds(n), d1(n), d2(n), f1(n), f2(n);
    std::vector<int32_t> na(n), a1(n), a2(n), r1(n), r2(n), v1(n * A), v2(n * A);
    for (long i = 0; i < n; ++i) {
        seeds[i] = lcg(&rs) * 977u + 1u;
        na[i] = (int32_t)(lcg(&rs) % 6);  // includes terminal boards
        for (int x = 0; x < N; ++x) {
            const uint32_t u = lcg(&rs);
            int v = 1 + (int)(u % (uint32_t)T);
            if (lcg(&rs) % 100 < 4) v |= 1 << (32 - __builtin_clz((unsigned)T));  // a line special
            boards[i * N + x] = (int8_t)v;
        }
    }
    long st1[3], st2[3];
    if (lh_lookahead(cfg, 16, n, boards.data(), seeds.data(), na.data(), a1.data(), r1.data(), v1.data(), d1.data(),
                     f1.data(), st1))
        return 1;
    for (int bpw : {1, 5, 64}) {
        if (lh_lookahead(cfg, bpw, n, boards.data(), seeds.data(), na.data(), a2.data(), r2.data(), v2.data(),
                         d2.data(), f2.data(), st2))
            return 1;
        for (long i = 0; i < n; ++i)
            if (a1[i] != a2[i] || r1[i] != r2[i] || d1[i] != d2[i] || f1[i] != f2[i]) {
                fprintf(stderr, "mismatch: cfg %d bpw %d board %ld\n", cfg, bpw, i);
                return 1;
            }
        for (long i = 0; i < n * A; ++i)
            if (v1[i] != v2[i]) return 1;
        checks += n;
    }
    // every output nullable
    if (lh_lookahead(cfg, 16, n, boards.data(), seeds.data(), na.data(), nullptr, nullptr, nullptr, nullptr, nullptr,
                     st2))
        return 1;
    return 0;
}

int main() {
    uint32_t rs = 12345u;
    long checks = 0;
    if (run(0, 9, 9, 6, rs, checks)) return 1;
    if (run(1, 16, 16, 8, rs, checks)) return 1;
    const int frames[][3] = {{7, 7, 4}, {5, 5, 6}, {10, 8, 9}, {6, 5, 15}};
    for (auto& f : frames) {
        if (lh_set_frame(f[0], f[1], f[2])) return 1;
        if (run(2, f[0], f[1], f[2], rs, checks)) return 1;
    }
    // the key at its corners
    const int32_t rw[] = {-2147483647 - 1, -1, 0, 1, 2147483646, 2147483647};
    for (int32_t r : rw)
        for (int a : {0, 1, 479, 1 << 20}) {
            const unsigned long long k = lh_key(r, a);
            if (k == 0ull || lh_key_reward(k) != r || lh_key_action(k) != a) return 1;
            ++checks;
        }
    printf("lookahead_host asan: %ld checks ok\n", checks);
    return 0;
}
