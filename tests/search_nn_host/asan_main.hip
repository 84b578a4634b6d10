// asan_main.hip -- TEST INFRASTRUCTURE ONLY: the network-guided tree core's host build
// (search_nn_host.hip) under AddressSanitizer + UndefinedBehaviorSanitizer, as a stand-alone program.
// It replays a scenario that tests/test_search_nn_cpu.py recorded from its Python run -- the roots, then
// per round what the step and the evaluator returned -- through the core, and prints every search
// result; the test compares the text with its own. The scenario is a list of integers (floats as
// their bit patterns):
//   n cap N AW A
//   1 boards[n*N] n_actions[n] rewards[n] legal[n*AW]             roots
//   2 out_boards[n*N] reward[n] flags[n] legal[n*AW]              a round's step (select, attach)
//   3 backup values[n] logits[n*A]                                the evaluator's answer (commit)
//   4 k | 7 k   a run of k rounds fits | must be refused          5 result     6 actions[n] advance
// Any sanitizer report exits non-zero.
#include "search_nn_host.hip"

#include <stdio.h>
#include <stdlib.h>

static FILE* f;

template <class T>
static bool rd(std::vector<T>& v, size_t k) {
    v.resize(k);
    for (size_t i = 0; i < k; ++i) {
        long long x;
        if (fscanf(f, "%lld", &x) != 1) return false;
        v[i] = (T)x;
    }
    return true;
}

static unsigned fbits(float x) {
    unsigned u;
    memcpy(&u, &x, 4);
    return u;
}

int main(int argc, char** argv) {
    if (argc != 2 || !(f = fopen(argv[1], "r"))) return 2;
    std::vector<long long> hd;
    if (!rd(hd, 5)) return 2;
    const long n = (long)hd[0];
    const int cap = (int)hd[1], N = (int)hd[2], AW = (int)hd[3], A = (int)hd[4];
    NH* h = nh_create(n, cap, N, AW, A);
    std::vector<int8_t> boards, rows(n * N), ev(n * N);
    std::vector<uint8_t> need(n);
    std::vector<int32_t> na, rew, row_na(n), row_act(n), act, best(n), val(n), rv(n), nc(n), ca(n * A), cv(n * A);
    std::vector<float> cs(n * A), cp(n * A), values(n), logits((size_t)n * A);
    std::vector<uint32_t> legal, fl, vb, lb, gf(n);
    std::vector<long long> op;
    int results = 0, refused = 0;
    while (rd(op, 1)) switch (op[0]) {
            case 1:
                if (!rd(boards, n * N) || !rd(na, n) || !rd(rew, n) || !rd(legal, n * AW)) return 2;
                nh_set_roots(h, boards.data(), na.data(), rew.data(), legal.data(), ev.data(), need.data());
                break;
            case 2:
                if (!rd(boards, n * N) || !rd(rew, n) || !rd(fl, n) || !rd(legal, n * AW)) return 2;
                nh_select(h, rows.data(), row_na.data(), row_act.data());
                nh_attach(h, boards.data(), rew.data(), fl.data(), legal.data(), ev.data(), need.data());
                break;
            case 3: {
                if (!rd(op, 1)) return 2;
                const int backup = (int)op[0];
                if (!rd(vb, n) || !rd(lb, (size_t)n * A)) return 2;
                memcpy(values.data(), vb.data(), (size_t)n * 4);
                memcpy(logits.data(), lb.data(), (size_t)n * A * 4);
                nh_commit(h, values.data(), logits.data(), backup);
                break;
            }
            case 4:
            case 7: {
                if (!rd(op, 1)) return 2;
                const int rc = nh_fits(h, (int)op[0]);
                if (rc == -7) {
                    ++refused;
                    printf("refused %lld\n", op[0]);
                } else if (rc) {
                    return 3;
                }
                break;
            }
            case 5:
                nh_finish(h, best.data(), val.data(), rv.data(), nc.data(), ca.data(), cv.data(), cs.data(), cp.data(),
                          gf.data());
                for (long g = 0; g < n; ++g) {
                    printf("%ld %d %d %d %d %u", g, best[g], val[g], rv[g], nc[g], gf[g]);
                    for (int k = 0; k < nc[g]; ++k)
                        printf(" %d:%d:%u:%u", ca[g * A + k], cv[g * A + k], fbits(cs[g * A + k]), fbits(cp[g * A + k]));
                    printf("\n");
                }
                ++results;
                break;
            case 6:
                if (!rd(act, n)) return 2;
                if (nh_advance(h, act.data(), rows.data(), rew.data(), na.data())) return 4;
                break;
            default: return 2;
        }
    int used = 0;
    for (long g = 0; g < n; ++g) used = nh_nodes_used(h, g) > used ? nh_nodes_used(h, g) : used;
    printf("search_nn_host asan: %d results, %d refused, %d of %d nodes: checks ok\n", results, refused, used, cap);
    nh_destroy(h);
    fclose(f);
    return 0;
}
