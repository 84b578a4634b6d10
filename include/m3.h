/*
 * m3.h -- C ABI of libm3.so, the MI355X-native batched Match3 env step.
 *
 * Plain C types only (no torch, no HIP types): the reference is Python, and a
 * Python maintainer binds this with ctypes. Every entry
 * point names the reference interface it replaces (paths relative to the
 * ThorLL/Element-Crush-Gym checkout).
 *
 * Conventions
 *   - Return value: 0 (M3_OK) on success, a negative M3_ERR_* code otherwise;
 *     m3_last_error() then returns a thread-local message.
 *   - Boards are int8 row-major [n][rows][columns], cell values in [0, 127]
 *     (the reference stores int64; every value reachable from env play or
 *     dataset.py's type_switch fits).
 *   - Legal-action bitsets are uint32 words [n][ceil(A/32)], bit a = action a
 *     (A = rows*(columns-1)*2, ids as BoardConfig.decode, boardConfig.py:45-59).
 *   - "draws" = raw MT19937 outputs consumed since the last reseed, i.e. numpy's
 *     global RandomState after the call equals seed(cfg.seed) advanced by draws
 *     (boardv2.py:46, boardFunctions.py:17) -- the facade uses it to keep the
 *     reference's global-RNG side effect.
 *   - All calls on one context are serialised on that context's HIP stream;
 *     use one context per host thread. Host-buffer calls block until done.
 *   - No CPU fallback: on a machine without a usable gfx950 device, context
 *     creation fails with M3_ERR_NO_DEVICE.
 */
#ifndef M3_H
#define M3_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define M3_ABI_VERSION 1

#define M3_OK 0
#define M3_ERR_INVALID (-1)     /* bad argument */
#define M3_ERR_UNSUPPORTED (-2) /* board shape not compiled in */
#define M3_ERR_HIP (-3)         /* HIP runtime error */
#define M3_ERR_RCCL (-4)        /* RCCL error */
#define M3_ERR_NO_DEVICE (-5)   /* no usable GPU */
#define M3_ERR_STATE (-6)       /* call out of order (e.g. step before reset) */
#define M3_ERR_CAP (-7)         /* a safety cap stopped a reset the reference would keep running (see flags);
                                   m3_search_run: the simulations do not fit the trees' node_capacity */

/* Per-board flags (uint32 out_flags). */
#define M3_FLAG_TERMINAL 0x01u    /* n_actions < 1: board returned unchanged (boardv2.py:44-45) */
#define M3_FLAG_BAD_ACTION 0x02u  /* action id not in [0, A): reference raises KeyError (boardv2.py:48) */
#define M3_FLAG_SHUFFLE_CAP 0x04u /* dead-board shuffle cycled past the cap: reference hangs (boardv2.py:188-194) */
#define M3_FLAG_NO_LEGAL 0x08u    /* no legal action to sample: reference raises in np.random.choice */
#define M3_FLAG_SHUFFLED 0x10u    /* the dead-board shuffle ran */
#define M3_FLAG_CASCADE_CAP 0x100u /* cascade stopped after 65536 refills: the reference keeps going (types = 2 boards) */
#define M3_FLAG_RESET_CAP 0x200u   /* reset stopped after 16384 redraw rounds: the reference keeps going (large types = 2 boards) */

typedef struct m3_ctx m3_ctx;
typedef struct m3_env m3_env;
typedef struct m3_search m3_search;

int m3_abi_version(void);
const char *m3_last_error(void);
/* Number of visible HIP devices (0 when none). Never initialises a context. */
int m3_device_count(int *out_count);
/* 1 if kernels for BoardConfig(rows, columns, types) are compiled in, else 0. */
int m3_supported(int rows, int columns, int types);
/* Action-space size and bitset words for a shape (BoardConfig.action_space, boardConfig.py:27). */
int m3_action_space(int rows, int columns, int *out_actions, int *out_words);

/* One context per (device, board shape): owns a HIP stream and scratch. */
int m3_ctx_create(int device, int rows, int columns, int types, m3_ctx **out);
int m3_ctx_destroy(m3_ctx *ctx);
int m3_ctx_synchronize(m3_ctx *ctx);

/* Device memory on the context's device, through the HIP runtime libm3 itself
 * runs on (host tools and benches need no second runtime, e.g. torch, in the
 * process). m3_dev_copy blocks; kind 1 = host to device, 2 = device to host. */
int m3_dev_alloc(m3_ctx *ctx, int64_t bytes, void **out);
int m3_dev_free(m3_ctx *ctx, void *ptr);
int m3_dev_copy(m3_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind);

/* ---- stateless batch calls on host buffers (BoardV2 facade) ------------- */

/* BoardV2(n_actions, cfg) with array=None: seeded initial board (boardv2.py:17-27).
 * out_first_action: np.random.seed(cfg.seed); np.random.choice(legal_actions)
 * (samplerTasks.py:11-13), -1 if the board has no legal action. Nullable outs. */
int m3_init_boards(m3_ctx *ctx, int64_t n, const uint32_t *seeds, int8_t *out_boards,
                   uint32_t *out_draws, int32_t *out_first_action);
/* The same, with out_flags[i] (nullable): M3_FLAG_RESET_CAP when reset i stopped after 16384 redraw
 * rounds (large types = 2 boards; the reference keeps drawing), M3_FLAG_NO_LEGAL when it has no legal
 * action. m3_init_boards itself returns M3_ERR_CAP (outputs written) if any reset hit the cap. */
int m3_init_boards_ex(m3_ctx *ctx, int64_t n, const uint32_t *seeds, int8_t *out_boards,
                      uint32_t *out_draws, int32_t *out_first_action, uint32_t *out_flags);

/* BoardV2.apply_action (boardv2.py:43-207) for n independent (board, seed,
 * n_actions, action) tuples. out_next_action = choice(legal_actions(next))
 * drawn from the stream where apply_action left it (samplerTasks.py:12-13).
 * out_legal_bits / out_next_action are nullable. */
int m3_apply_actions(m3_ctx *ctx, int64_t n, const int8_t *boards, const uint32_t *seeds,
                     const int32_t *n_actions, const int32_t *actions, int8_t *out_boards,
                     int32_t *out_reward, uint32_t *out_draws, uint32_t *out_flags,
                     uint32_t *out_legal_bits, int32_t *out_next_action);

/* legal_actions(cfg, board) (boardFunctions.py:26-112) as bitsets. */
int m3_legal_actions(m3_ctx *ctx, int64_t n, const int8_t *boards, uint32_t *out_legal_bits);

/* ---- batched MCTS rollouts (mctslib/standard/mcts.py:14-19) ------------- */

/* MCTS.rollout(state) for n independent states (board, cfg.seed, n_actions):
 * np.random.seed(rollout_seeds[i]); while n_actions >= 1: action =
 * np.random.choice(legal_actions); state = state.apply_action(action).
 * The first choice reads rollout_seeds[i]'s stream, later ones the stream
 * apply_action left (cfg.seed + draws), exactly as the reference's global RNG.
 * out_gain = sum of the step rewards (rollout return = state.reward + gain),
 * out_steps = apply_action calls, out_draws = raw draws of the global stream
 * since its last seed at the end (seed = cfg.seed if out_steps > 0, else
 * rollout_seeds[i]), out_flags = OR of the steps' M3_FLAG_* (M3_FLAG_NO_LEGAL:
 * the reference raises in np.random.choice; the rollout stops there).
 * out_boards (nullable) = terminal boards. Host buffers; blocks until done. */
int m3_rollouts(m3_ctx *ctx, int64_t n, const int8_t *boards, const uint32_t *seeds,
                const int32_t *n_actions, const uint32_t *rollout_seeds, int32_t *out_gain,
                int32_t *out_steps, uint32_t *out_draws, uint32_t *out_flags, int8_t *out_boards);
/* Same on device buffers, enqueued on the context stream (no sync). Inputs
 * must stay valid until the stream reaches the launch. */
int m3_rollouts_device(m3_ctx *ctx, int64_t n, const int8_t *boards, const uint32_t *seeds,
                       const int32_t *n_actions, const uint32_t *rollout_seeds, int32_t *out_gain,
                       int32_t *out_steps, uint32_t *out_draws, uint32_t *out_flags, int8_t *out_boards);

/* ---- one-ply lookahead (BoardV2.greedy_action, boardv2.py:209-218) ------ */

/* For n independent states (board, cfg.seed, n_actions): the step reward of EVERY legal action,
 * i.e. apply_action(a).reward - state.reward for each a of legal_actions (boardv2.py:209-218,
 * samplers.greedy_actions), each on a private copy of the board with the stream reseeded from
 * cfg.seed, the dead-board shuffle and everything after it included.
 *   out_values [n][A]  the step reward of action a if legal, -1 otherwise
 *   out_best_action    the lowest legal id among the maxima (the reference's loop keeps the first
 *                      strict maximum of the ascending legal list); -1 without a legal action
 *   out_best_reward    that reward; -1 without a legal action
 *   out_last_draws     raw draws of the apply of the HIGHEST legal id -- where numpy's global
 *                      stream stands after the reference's loop; 0 if terminal or none legal
 *   out_flags          OR of the candidates' M3_FLAG_*, M3_FLAG_NO_LEGAL without a legal action,
 *                      M3_FLAG_TERMINAL for n_actions < 1 (every legal action is then worth 0)
 * Every out is nullable. Host buffers; blocks until done. Cells outside [0, 127]: M3_ERR_INVALID.
 * Boards with a side above 16 (the 32 x 32 frame): M3_ERR_UNSUPPORTED. */
int m3_lookahead(m3_ctx *ctx, int64_t n, const int8_t *boards, const uint32_t *seeds,
                 const int32_t *n_actions, int32_t *out_best_action, int32_t *out_best_reward,
                 int32_t *out_values, uint32_t *out_last_draws, uint32_t *out_flags);
/* Same on device buffers, enqueued on the context stream (no sync). Inputs must stay valid until
 * the stream reaches the launch. */
int m3_lookahead_device(m3_ctx *ctx, int64_t n, const int8_t *boards, const uint32_t *seeds,
                        const int32_t *n_actions, int32_t *out_best_action, int32_t *out_best_reward,
                        int32_t *out_values, uint32_t *out_last_draws, uint32_t *out_flags);

/* ---- device-resident MCTS trees (mctslib/abc/mcts.py:33-128, standard/mcts.py) ---------- */
/* n_games UCB1 search trees in device memory, searched in lockstep: one simulation round of every
 * game is a fixed sequence of launches on the context stream -- selection, the expansion's
 * apply_action, the attach, the rollout, the backup -- with no host round trip inside a search.
 * The search is the reference's, node for node: expansion pops the HIGHEST untried action
 * (untried_actions = list(legal), then pop(): abc/mcts.py:45,60), children keep their expansion
 * order, every maximum is the first one in that order, and UCB1 is evaluated bit for bit as CPython
 * evaluates it (doubles, every operation rounded on its own, log from a table filled by the host's
 * libm: csrc/m3_search_core.hpp). leaf_rollouts > 1 and deterministic=True (match3tile/mcts.py) are
 * not offered here.
 *
 * Memory: every game owns node_capacity node slots of 16 + 32 + 4 * ceil(A/32) + rows*columns bytes
 * (9x9x6: 149, 16x16x8: 368), never compacted: re-rooting keeps the slots of the dropped siblings.
 * A search of `simulations` rounds takes at most one slot per game and round;
 * 2 + moves * simulations slots hold a whole game of `moves` searches.
 *
 * A game freezes -- no expansion, no backup for the rest of its life, its flag word set -- where the
 * reference raises or never returns: a non-terminal node without a legal action (M3_FLAG_NO_LEGAL:
 * max() of no children, abc/mcts.py:96) and M3_FLAG_SHUFFLE_CAP / M3_FLAG_CASCADE_CAP of a step or a
 * rollout (an expansion's step gives its cap bits only: nothing is sampled after it; a rollout gives
 * its whole word, M3_FLAG_NO_LEGAL included where it went on past a cap to its next choice).
 * The other games go on. A frozen game's result is its root's children and visits as they
 * stood and its flag word (value: the root's reward, no part of the contract); m3_search_advance
 * leaves its root where it is and does not count it as a bad action.
 *
 * Every board shape the context takes is searched, the 32 x 32 frame (a side above 16) included:
 * unlike m3_lookahead, m3_search_create refuses none of them but rows < columns (M3_ERR_INVALID). */
int m3_search_create(m3_ctx *ctx, int64_t n_games, int32_t node_capacity, m3_search **out);
int m3_search_destroy(m3_search *s);
/* out[v - 1] = log(v) for v = 1..n: the table UCB1's log(parent.visits) is read from, std::log of
 * the host's libm, which CPython's math.log calls too (standard/mcts.py:36). Host only, needs no GPU. */
int m3_search_log_table(int32_t n, double *out);
/* MCTS.__init__ (abc/mcts.py:78-82) for every game: the root node of state (boards[i], cfg.seed =
 * seeds[i], n_actions[i], reward = rewards[i]) and the constructor's one expansion, without a
 * rollout. Drops the trees the object held: node slots, flag words and statistics start again.
 * Host buffers; blocks until done.
 * One departure from the reference, on purpose: a root with n_actions < 1. The reference's
 * constructor expands it all the same, apply_action of a terminal state returns the state itself,
 * and its search answers with an unplayable action and the policy [0.0]. Here such a root keeps no
 * child: m3_search_result reports best_action -1, n_children 0, value = rewards[i], flags 0, and
 * root_visits counts the simulations run. */
int m3_search_set_roots(m3_search *s, const int8_t *boards, const uint32_t *seeds, const int32_t *n_actions,
                        const int32_t *rewards);
/* `simulations` rounds of MCTS.__call__'s loop (abc/mcts.py:91-109) for every game. rollout_seeds:
 * host uint32 [simulations][n_games], round-major: the random.randint(0, 2**31 - 1) that
 * MCTS.rollout draws once per simulation, terminal leaf or not (standard/mcts.py:15), so the caller
 * pre-draws `simulations` seeds per game from that game's generator, in order. Returns once the seeds
 * are on their way and the rounds are enqueued; it does not wait for the kernels. M3_ERR_STATE before
 * m3_search_set_roots. M3_ERR_CAP, with nothing enqueued and the trees untouched, unless
 * used + simulations + 1 <= node_capacity, used = 1 + the simulations run since m3_search_set_roots. */
int m3_search_run(m3_search *s, int32_t simulations, const uint32_t *rollout_seeds);
/* What MCTS.__call__ returns (abc/mcts.py:113-120), without re-rooting: best_action = the action of
 * the FIRST most-visited root child in expansion order (-1 without a child), value = the reward of
 * the state where best_child(0) stops descending, root_visits, and the root's n_children children
 * in expansion order: child_action / child_visits / child_reward [n][A] (the policies are
 * child_visits / root_visits). flags: the game's M3_FLAG_* word, non-zero = frozen. Every out is
 * nullable. Host buffers; blocks until the runs before it are done. */
int m3_search_result(m3_search *s, int32_t *best_action, int32_t *value, int32_t *root_visits, int32_t *n_children,
                     int32_t *child_action, int32_t *child_visits, int64_t *child_reward, uint32_t *flags);
/* Re-root every game at the child its action leads to (abc/mcts.py:123-124); actions = NULL: at the
 * best_action of the last m3_search_result. The subtree keeps its visit counts and reward sums; the
 * new root has no parent. out_*: the new roots as states (board, reward, n_actions, legal bitset),
 * each nullable. M3_ERR_INVALID if an action has no expanded child (those games keep their root). */
int m3_search_advance(m3_search *s, const int32_t *actions, int8_t *out_boards, int32_t *out_rewards,
                      int32_t *out_n_actions, uint32_t *out_legal_bits);
/* Since m3_search_set_roots: out[0] node slots used (the maximum over the games, as of the last
 * m3_search_result), out[1] rounds run, out[2] / out[3] expansions / rollouts recomputed by the
 * exact pass of the apply / rollout kernels. Blocks. */
int m3_search_stats(m3_search *s, uint64_t out[4]);
/* Test hook: Node.ucb1 (standard/mcts.py:33-37) on the device for n independent (reward_sum, visits,
 * parent_visits >= 1, c) tuples, as the selection kernel evaluates it. Host buffers; blocks. */
int m3_search_ucb1(m3_ctx *ctx, int64_t n, const int64_t *reward_sum, const int32_t *visits,
                   const int32_t *parent_visits, const double *c, double *out);

/* ---- network-guided device MCTS trees (mctslib/nn/mcts.py: NNNode, NeuralNetworkMCTS) ---------- */
/* n_games prior-weighted search trees in device memory, searched in lockstep, with the evaluator
 * behind a split-phase call: a round runs up to an EVALUATION BATCH -- one board per game and a
 * `need` byte -- and goes on once the caller has fed (value: f32, logits: f32[A]) for every game.
 * The library keeps no ML framework in the process; an evaluator is anything that fills two device
 * (or host) arrays. Semantics (csrc/m3_search_nn_core.hpp has the arithmetic, DESIGN.md §4.9 the
 * reasons):
 *   - every node that is created and is not terminal is evaluated once; the logits stay raw (no
 *     softmax, they may be negative), entries of illegal actions are never read;
 *   - a child's prior is its parent's logit at the child's action, the root's prior is 1.0;
 *   - expansion pops the highest untried legal action, one expansion per game and round;
 *   - score of a child with v visits under a parent with pv visits and c = the parent state's
 *     n_actions: +inf if v == 0, else in float32, every operation rounded on its own,
 *         sum / (f32)v + ((f32)c * prior) * (f32)sqrt(log(pv) / (double)(1 + v))
 *     (the square root's argument in double, rounded to f32 once); first maximum in expansion order;
 *   - backup: the evaluator's value for a new non-terminal child, (f32)state reward for a terminal
 *     leaf or a terminal new child -- not reward plus value -- added in f32 from leaf to root (the
 *     reference keeps an all-integer sum as an int; here it is always f32, exact below 2^24).
 * The trees are pinned to the reference's own tree code. It is executed with numpy standing in for
 * `jax.numpy` and with integer rewards handed over as Python ints, so that numpy promotes as JAX does
 * with x64 off. JAX itself has still not been run.
 *
 * Memory: node_capacity slots per game of 16 + 32 + 4 * ceil(A/32) + rows*columns + 4 * A bytes
 * (9x9x6: 725, 16x16x8: 2,288), never compacted.
 *
 * A game freezes as in the UCB1 trees (M3_FLAG_NO_LEGAL, M3_FLAG_SHUFFLE_CAP / M3_FLAG_CASCADE_CAP of
 * an expansion's step) and in one more case: a needed row whose value, or any logit of a legal
 * action, is not finite gives M3_FLAG_BAD_EVAL; the node it was for is not linked, the tree stays as
 * it stood. The other games go on.
 *
 * The batch protocol. After m3_search_nn_set_roots the first two batches are the construction's
 * (abc/mcts.py:82): the roots themselves, then the child of each root's highest legal action; neither
 * backs anything up. Every later batch is one simulation round. The library tracks the phase.
 *   m3_search_nn_batch        enqueues the work up to the next batch and returns its device pointers:
 *                             boards int8 [n][N], need uint8 [n] (1: the game created a non-terminal
 *                             node this round; rows with need 0 are ignored when fed).
 *   m3_search_nn_feed_device  values f32 [n], logits f32 [n][A] in device memory: enqueues the rest of
 *   m3_search_nn_feed         the round. The host form stages the arrays and blocks until done.
 * Everything runs on the context stream. Ordering contract for an evaluator on a foreign runtime or
 * stream: m3_ctx_synchronize after m3_search_nn_batch and before reading the batch; the caller's own
 * stream finished before m3_search_nn_feed_device (the library does not wait for it).
 * M3_ERR_STATE: a feed without a pending batch, a second batch (or a result / advance / run_linear)
 * while one is pending, any call before m3_search_nn_set_roots. */
#define M3_FLAG_BAD_EVAL 0x400u /* search_nn: a needed evaluation (value or a legal logit) is not finite */
typedef struct m3_search_nn m3_search_nn;
int m3_search_nn_create(m3_ctx *ctx, int64_t n_games, int32_t node_capacity, m3_search_nn **out);
int m3_search_nn_destroy(m3_search_nn *s);
/* The root nodes, as m3_search_set_roots (a root with n_actions < 1 keeps no child and is never
 * evaluated). Drops the trees the object held and any pending batch. The next batch is the roots'. */
int m3_search_nn_set_roots(m3_search_nn *s, const int8_t *boards, const uint32_t *seeds, const int32_t *n_actions,
                           const int32_t *rewards);
/* remaining: the simulations the caller's run still has to go, this one included (ignored for the two
 * construction batches). M3_ERR_CAP, with nothing enqueued and the trees untouched, unless
 * used + remaining + 1 <= node_capacity, used = 1 + the simulation rounds fed since set_roots: passed
 * truthfully, a run that does not fit is refused at its first batch. Does not wait for the kernels. */
int m3_search_nn_batch(m3_search_nn *s, int32_t remaining, const int8_t **d_boards, const uint8_t **d_need);
int m3_search_nn_feed_device(m3_search_nn *s, const float *d_values, const float *d_logits);
int m3_search_nn_feed(m3_search_nn *s, const float *values, const float *logits);
/* The built-in baseline evaluator, and a whole run with no host round trip: any pending construction
 * batches and then `simulations` rounds, each batch evaluated on the device by a linear map of the
 * one-hot board. d_W: device f32 [N][CH][A + 1], CH = 2^(ceil(log2(types)) + 2) (the reference's
 * one-hot width, elementCrush.py:66, :92); a cell whose value is >= CH contributes nothing.
 *     out[j] = (((W[0][x0][j] + W[1][x1][j]) + W[2][x2][j]) + ...) over the cells in ascending order,
 * float32, no bias; logits = out[0 .. A), value = out[A]. M3_ERR_CAP as m3_search_nn_batch with
 * remaining = simulations. Does not wait for the kernels; d_W must stay valid until they are done. */
int m3_search_nn_run_linear(m3_search_nn *s, int32_t simulations, const float *d_W);
/* As m3_search_result, with child_value_sum (f32) in place of child_reward, and child_prior (f32).
 * value is still the integer state reward at the end of the greedy line (c = 0 in the score). */
int m3_search_nn_result(m3_search_nn *s, int32_t *best_action, int32_t *value, int32_t *root_visits,
                        int32_t *n_children, int32_t *child_action, int32_t *child_visits, float *child_value_sum,
                        float *child_prior, uint32_t *flags);
/* As m3_search_advance. */
int m3_search_nn_advance(m3_search_nn *s, const int32_t *actions, int8_t *out_boards, int32_t *out_rewards,
                         int32_t *out_n_actions, uint32_t *out_legal_bits);
/* Since m3_search_nn_set_roots: out[0] node slots used (the maximum over the games, as of the last
 * result), out[1] simulation rounds fed, out[2] expansions recomputed by the apply kernel's exact
 * pass, out[3] batches fed from host arrays, out[4] from device arrays, out[5] evaluated by the
 * built-in linear evaluator. Blocks. */
int m3_search_nn_stats(m3_search_nn *s, uint64_t out[6]);

/* ---- the policy/value network: the reference's ElementCrush (elementCrush.py:51-97,
 * elementGOModules.py) in inference form, on the device (csrc/m3_net.hip; DESIGN.md §4.4 has the
 * arithmetic model). For a context of rows x columns x types: P = rows * columns, A = the action
 * space, CH = 2^(ceil(log2(types)) + 2).
 *   one_hot(cell, CH): a cell < 0 or >= CH is the zero vector (any int8 is accepted)
 *   stem    3x3 SAME conv CH -> F with bias, BatchNorm, ReLU
 *   tower   `layers` x (conv, BN, ReLU, conv, BN, + residual, ReLU), 3x3 SAME F -> F with bias
 *   value   1x1 conv F -> 1, BN, ReLU, flatten, dense [P -> F], ReLU, dense [F -> 1], ReLU
 *   policy  1x1 conv F -> 2, BN, ReLU, flatten (NHWC: (r * columns + c) * 2 + ch), dense [2P -> A]:
 *           raw logits
 * BatchNorm uses the stored statistics, y = (x - mean) * scale / sqrt(var + bn_eps) + bias, folded
 * in float64 into the convolution before it. The tower runs on the bf16 matrix cores with float32
 * accumulation (weights rounded once to bf16, activations stored as bf16); stem and heads are float32.
 * A board's outputs do not depend on n, on its index in the batch or on the need mask.
 *
 * blob: the weights as float32, concatenated in this order (conv kernels [kh][kw][in][out], dense
 * kernels [in][out]; "bn" = scale, bias, mean, var, each [out]):
 *   stem kernel [3][3][CH][F], bias [F], bn;
 *   per residual layer: conv1 kernel [3][3][F][F], bias [F], bn1; conv2 kernel, bias, bn2;
 *   value: conv kernel [1][1][F][1], bias [1], bn; dense1 kernel [P][F], bias [F]; dense2 kernel
 *   [F][1], bias [1];
 *   policy: conv kernel [1][1][F][2], bias [2], bn; dense kernel [2P][A], bias [A].
 * features: a multiple of 32 in 32..512 (else M3_ERR_UNSUPPORTED); layers >= 0. rows, columns and
 * types must be the context's, blob_len the exact length (M3_ERR_INVALID). The workspace (two bf16
 * activation buffers of at most 64 MiB each) is allocated here; larger batches run in chunks of boards. */
typedef struct m3_net m3_net;
int m3_net_create(m3_ctx *ctx, int32_t rows, int32_t columns, int32_t types, int32_t layers, int32_t features,
                  double bn_eps, const float *blob, int64_t blob_len, m3_net **out);
int m3_net_destroy(m3_net *net);
/* Host arrays: boards int8 [n][P] -> values f32 [n], logits f32 [n][A]. Blocks. n = 0 is allowed. */
int m3_net_forward(m3_net *net, const int8_t *boards, int64_t n, float *values, float *logits);
/* The same on device arrays, enqueued on the context stream; does not wait. d_need (nullable,
 * uint8 [n]): rows with need == 0 are not written. */
int m3_net_forward_device(m3_net *net, const int8_t *d_boards, const uint8_t *d_need, int64_t n, float *d_values,
                          float *d_logits);
/* Feature extraction: the trunk's activations after the stem (upto = 0) or after residual layer
 * `upto` (1..layers), widened to float32, out [n][rows][columns][F] (host). Blocks. */
int m3_net_trunk(m3_net *net, const int8_t *boards, int64_t n, int32_t upto, float *out);
/* m3_search_nn_run_linear with the network as the evaluator: the pending construction batches and
 * `simulations` rounds with no host round trip (counted in m3_search_nn_stats out[4]). The state and
 * capacity errors are the same; M3_ERR_INVALID if the net was not made on the search's context (so
 * for another board shape). */
int m3_search_nn_run_net(m3_search_nn *s, int32_t simulations, m3_net *net);

/* ---- device-resident batched env: n x Match3Env (env.py:8-65) ----------- */

/* num_moves / env_goal as Match3Env(num_moves=20, env_goal=500) (env.py:15-16). */
int m3_env_create(m3_ctx *ctx, int64_t n, int num_moves, int env_goal, m3_env **out);
int m3_env_destroy(m3_env *env);

/* Match3Env.reset (env.py:58-65) for every board. seeds: host uint32[n], or
 * NULL for seeds seed_base + i. Draws each board's first seeded random action. */
int m3_env_reset(m3_env *env, const uint32_t *seeds, uint32_t seed_base);

/* Split the boards into nshards (1..8) contiguous shards, each stepped on its
 * own HIP stream (plus one prefetch stream per shard for the autoreset
 * launches). Results do not depend on it, and it may be called between any
 * two steps: the call waits for the env's work, the run goes on exactly as it
 * would have, and the m3_env_stats counters stay cumulative across it (a shard
 * that is no longer in use keeps what it counted). Default: 1. Each shard adds two
 * streams; with GPU_MAX_HW_QUEUES >= 8 in the process, 2 shards are fastest
 * (the shards' step kernels fill each other's tails); with HIP's default 4
 * queues, 1. */
int m3_env_set_shards(m3_env *env, int nshards);
/* Wait for all work of the env (every shard stream). */
int m3_env_synchronize(m3_env *env);

/* After a step, boards that are done are reset in place with seed += stride
 * (gymnasium vector-env autoreset; same-step semantics). Default: off. */
int m3_env_set_autoreset(m3_env *env, int enabled, uint32_t seed_stride);

/* Match3Env.step (env.py:48-56) on every board. actions: host int32[n], or
 * NULL to play each board's seeded env.board.random_action() (README.md:23,
 * samplerTasks.py:13) drawn on device at the end of the previous step.
 * Host actions are copied into pinned staging before the call returns (the
 * caller may reuse `actions` at once) and uploaded on a stream of their own;
 * the call blocks at most until the upload of two steps earlier is done. */
int m3_env_step(m3_env *env, const int32_t *actions);
/* Same with actions already in device memory (int32[n]); NULL = random. */
int m3_env_step_device(m3_env *env, const int32_t *d_actions);

/* The one-ply lookahead (m3_lookahead, boardv2.py:209-218) of the env's CURRENT boards, with their
 * current episode seeds and n_actions = num_moves - moves taken, as the next step would apply them.
 * Device buffers int32[n], int32[n], int32[n][A], each nullable. Enqueued per shard on the shard's
 * step stream, behind the previous step: the results are valid after m3_env_synchronize, or for
 * any later call on the env. M3_ERR_STATE before m3_env_reset. */
int m3_env_lookahead(m3_env *env, int32_t *d_best_action, int32_t *d_best_reward, int32_t *d_values);
/* Match3Env.step with every board playing BoardV2.greedy_action (boardv2.py:209-218, the policy of
 * samplerTasks.greedy_test): m3_env_lookahead into a buffer of the env, then m3_env_step_device on
 * it. A board without a legal action plays -1, as under the random policy (M3_FLAG_BAD_ACTION). */
int m3_env_step_greedy(m3_env *env);

/* What to copy out. */
#define M3_ENV_BOARDS 0      /* int8  [n][rows*columns]  observation (env.py:56) */
#define M3_ENV_REWARD 1      /* int32 [n]  reward of the last step           */
#define M3_ENV_DONE 2        /* uint8 [n]  done (env.py:54)                  */
#define M3_ENV_TRUNCATED 3   /* uint8 [n]  truncated: score >= env_goal (env.py:53) */
#define M3_ENV_SCORE 4       /* int32 [n]  episode score                      */
#define M3_ENV_MOVES 5       /* int32 [n]  moves taken in the episode         */
#define M3_ENV_FLAGS 6       /* uint32[n]  M3_FLAG_* of the last step         */
#define M3_ENV_NEXT_ACTION 7 /* int32 [n]  pre-drawn seeded random action     */
#define M3_ENV_LEGAL 8       /* uint32[n][words] legal bitset of the current board (derived: m3_env_get
                                computes it from the boards; after m3_env_device_ptr of this field every
                                step writes it, for device consumers) */
#define M3_ENV_SEEDS 9       /* uint32[n]  current episode seed               */
#define M3_ENV_DRAWS 10      /* uint32[n]  raw MT draws of the last step      */
#define M3_ENV_GATHERED 11   /* int32 [nranks][n] the env's all-gather buffer (after m3_env_comm_init) */
int m3_env_get(m3_env *env, int what, void *host_out);
int m3_env_device_ptr(m3_env *env, int what, void **out);

/* Checkpoint / resume of the batched env (the reference state is
 * (array, cfg.seed, n_actions, _reward), boardv2.py:12-16, plus Match3Env's
 * score and moves_taken, env.py:34). Overwrites one field of every board from
 * host memory laid out as m3_env_get returns it. Settable: M3_ENV_BOARDS,
 * SEEDS, SCORE, MOVES, NEXT_ACTION and the last step's REWARD, DONE,
 * TRUNCATED, FLAGS, DRAWS; LEGAL and GATHERED are derived (M3_ERR_INVALID).
 * The per-board state the env derives from these -- the legal set of the
 * board, the MT19937 chain word mt[397] of the seed, the queued autoreset
 * episodes -- is rebuilt before the next step / get / synchronize, so an env
 * loaded with another env's fields steps exactly as that env would have. A
 * freshly created env may be loaded instead of reset. */
int m3_env_set(m3_env *env, int what, const void *host_in);

/* ---- multi-GPU: RCCL over xGMI, one process per GPU --------------------- */
/* 128-byte ncclUniqueId; rank 0 creates it, the caller ships it to all ranks. */
int m3_comm_unique_id(uint8_t out_id[128]);
/* One communicator per env; a second call returns M3_ERR_STATE. */
int m3_env_comm_init(m3_env *env, const uint8_t id[128], int nranks, int rank);
/* Ranks of the env's communicator as RCCL reports them (ncclCommCount); 1 before m3_env_comm_init. */
int m3_env_comm_size(m3_env *env, int *out_nranks);
/* ncclAllGather of the last step's packed (reward << 2 | truncated << 1 | done)
 * int32 words of every board of every rank into the env's device buffer
 * M3_ENV_GATHERED ([nranks][n], rank-major); host_out (nullable, int32[nranks*n])
 * receives a copy and the call then blocks until it is there. The step kernel
 * writes the packed words only once a communicator exists, so gather the
 * outcomes of steps taken after m3_env_comm_init. No counterpart in the
 * reference (single host, no collectives): SURVEY.md §8(e). */
int m3_env_gather(m3_env *env, int32_t *host_out);
/* Same, into a caller-owned device buffer d_out (int32[nranks][n]; NULL = the
 * env's buffer), enqueued on the env's context stream without blocking. d_out
 * holds the step's outcomes once that stream reaches the gather: after
 * m3_env_synchronize, or for any later m3_env_get / m3_env_gather. Steps keep
 * running meanwhile (the packed words are double-buffered by step parity). */
int m3_env_gather_device(m3_env *env, int32_t *d_out);
/* Test hook: enqueue ~usec of idle GPU time on the env's context stream (the
 * stream the gathers run on), to hold a gather in flight while later steps run. */
int m3_env_debug_stall(m3_env *env, uint32_t usec);

/* Cumulative counters since the last m3_env_reset (m3_env_set_shards, m3_env_set_autoreset and
 * m3_env_set leave them counting): out[0] steps recomputed on
 * the exact fallback pass (>= 624 MT draws or more match groups than the LDS
 * table), out[1] resets recomputed by the wave-cooperative pass (9x9x6: a
 * reset of more than 624 MT draws -- exactly 624 still fits the register chain
 * -- or, when an autoreset's prefetch built it, of more than 454, or one whose
 * tile ring would have overrun; other shapes: the resets past what their
 * fast reset kernel covers, 624 draws or more on the explicit-reset path),
 * out[2] autoresets, out[3] number of shards. */
int m3_env_stats(m3_env *env, uint64_t out[4]);

/* ---- timing helpers for bench.py ---------------------------------------- */
/* Kernel-side timing: after m3_env_timing(env, cap), each of the next cap
 * shard-step launches records HIP events on its shard's stream before
 * k_env_step, after it, and after the pipeline's last kernel (k_env_cont_grid,
 * k_env_fix). m3_env_kernel_ms waits for them and returns the per-launch
 * durations of the whole pipeline in ms (out_n of them); m3_env_step_kernel_ms
 * the same for k_env_step alone (the dominant kernel, bench.py's roofline). */
/* Stopwatch on the context stream (HIP events): what = 0 marks the start; what = 1 marks the stop,
 * waits for it and returns in *out_ms the device time of everything enqueued on the context stream
 * between the two marks (the *_device calls; tools/lookahead_bench.py). */
int m3_ctx_timer(m3_ctx *ctx, int what, float *out_ms);
int m3_env_timing(m3_env *env, int capacity);
int m3_env_kernel_ms(m3_env *env, float *out_ms, int max_n, int *out_n);
int m3_env_step_kernel_ms(m3_env *env, float *out_ms, int max_n, int *out_n);

#ifdef __cplusplus
}
#endif
#endif /* M3_H */
