"""The evaluators of the network-guided search tests, importing numpy only: the golden generator
(tests/golden/gen_golden_search_nn.py) runs them under the reference's tree code, the model of
search_nn_ref.py and the device tests run the very same functions.

An evaluator of a case is ``ev(board[R, C], game, round) -> (value f32, logits f32[A])``.
"""
import math

import numpy as np

f32 = np.float32


def onehot_width(types):
    return 2 ** (int(math.ceil(math.log2(types))) + 2)


def weights(shape, k):
    """W [N][CH][A + 1] of the linear evaluator, from RandomState(k)."""
    R, C, T = shape
    A = R * (C - 1) * 2
    return np.random.RandomState(k).standard_normal((R * C, onehot_width(T), A + 1)).astype(np.float32)


def linear_eval(W, board):
    """out[j] = (((W[0][x0][j] + W[1][x1][j]) + ...): a sequential float32 loop over the cells, vectorised
    over j only. A cell >= CH contributes nothing. Returns (value, logits)."""
    CH, A = W.shape[1], W.shape[2] - 1
    acc = None
    with np.errstate(invalid="ignore"):  # (inf + -inf of poisoned weights is a NaN, on purpose)
        for i, x in enumerate(np.asarray(board).reshape(-1)):
            x = int(x)
            if 0 <= x < CH:
                acc = W[i, x].copy() if acc is None else (acc + W[i, x]).astype(np.float32)
    if acc is None:
        acc = np.zeros(A + 1, np.float32)
    return f32(acc[A]), acc[:A].copy()


def constant_ev(board, game, rnd):
    return f32(0.0), np.ones(2 * board.shape[0] * (board.shape[1] - 1), np.float32)


def negative_ev(board, game, rnd):
    """All logits negative, distinct per action; the value depends on the board."""
    A = 2 * board.shape[0] * (board.shape[1] - 1)
    return f32(int(np.asarray(board).sum()) % 7) * f32(0.25), (-(np.arange(A) % 5) - f32(0.5)).astype(np.float32)
