"""Brute-force reference and cases of the energy-score training head (the definition at ude_energy_forward in
include/ude_rk4.h), NumPy fp64, independent of the package.

Per window b and block C (joint: all (t, r); series: region r's times; field: time t's regions), over the
block's live coordinates (y != -1), with X (S, c) the samples' rows, D = S (fair: S - 1):
  ES_C = (1/S) sum_i |X_i - y| - (1/(2 S D)) sum_i sum_j |X_i - X_j|         (X[:, None] - X[None], every pair)
  loss = sum of ES_C / (B K);   d loss / d X_i = g / (B K) [ (X_i - y) / (S |X_i - y|) - (1/(S D)) sum_j
  (X_i - X_j) / |X_i - X_j| ], a term with norm 0 dropped; 0 at dropped coordinates.
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

BLOCKS = ("joint", "series", "field")
# (T, S, B, R)
CASES = {
    "odd_S": (3, 5, 4, 1),                # odd sample count
    "partial_tiles": (2, 33, 3, 10),      # two sample tiles plus one row
    "state_like": (9, 64, 2, 49),         # the training shape's T, S and R: 14 coordinate chunks per joint block
    "wide_R": (2, 17, 2, 70),             # more than 64 regions: a field block of three chunks, the last partial
    "max_S": (1, 128, 2, 3),              # the largest S the kernels must take: nine partners per thread
    "one_sample": (2, 1, 5, 2),           # S = 1: the pair term is exactly 0
    "one_coord": (1, 7, 3, 1),            # a block of one coordinate
    "ties": (3, 20, 3, 5),                # duplicated trajectories, ties in one series only, a sample on the target
    "masked_third": (3, 9, 3, 10),        # about a third of the targets -1
    "masked_block": (3, 9, 3, 10),        # a whole series and a whole time row of one window -1
    "masked_all": (2, 9, 3, 10),          # every target -1
}
COTANGENTS = (1.0, -3.5)


@dataclass(frozen=True)
class Case:
    name: str
    T: int
    S: int
    B: int
    R: int
    yhat: np.ndarray      # (T, S*B, R) fp32
    y: np.ndarray         # (B, T, R) fp32


@lru_cache(maxsize=None)
def make_case(name: str) -> Case:
    T, S, B, R = CASES[name]
    rng = np.random.default_rng(list(CASES).index(name) + 29)
    y = (2.0 + rng.random((B, T, R))).astype(np.float32)
    x = (y.transpose(1, 0, 2)[:, None] + 0.5 * rng.standard_normal((T, S, B, R))).astype(np.float32)   # (T, S, B, R)
    if name == "ties":
        x[:, 1] = x[:, 0]                       # whole trajectories duplicated, in every window: a pair
        x[:, 19] = x[:, 18] = x[:, 17]          # and a triple across the two sample tiles (17, 18 | 19 is in tile 1)
        x[:, 5, 1, 2] = x[:, 4, 1, 2]           # samples 4 and 5 of window 1 tied in region 2's series only
        x[:, 7, 2] = y[2]                       # sample 7 of window 2 on the target over the joint block
        x[1, 9, 0] = y[0, 1]                    # sample 9 of window 0 on the target over the field block t = 1
        x[:, 11, 0, 3] = y[0, :, 3]             # sample 11 of window 0 on the target over region 3's series
    if name == "masked_third":
        y[rng.random((B, T, R)) < 1.0 / 3.0] = -1.0
        assert 0 < (y == -1).sum() < y.size
    if name == "masked_block":
        y[1, :, 4] = -1.0                       # a whole series of window 1
        y[1, 2, :] = -1.0                       # and a whole time row
        y[0, 0, 0] = -1.0
    if name == "masked_all":
        y[...] = -1.0
    x.setflags(write=False)
    y.setflags(write=False)
    return Case(name, T, S, B, R, x.reshape(T, S * B, R), y)


def n_blocks(case: Case, block: str) -> int:
    return {"joint": 1, "series": case.R, "field": case.T}[block]


def block_coords(case: Case, block: str) -> int:
    """C: the coordinates of a block (before any is dropped)."""
    return {"joint": case.T * case.R, "series": case.T, "field": case.R}[block]


def _block_masks(T: int, R: int, block: str):
    if block == "joint":
        yield np.ones((T, R), dtype=bool)
    elif block == "series":
        for r in range(R):
            m = np.zeros((T, R), dtype=bool)
            m[:, r] = True
            yield m
    else:
        for t in range(T):
            m = np.zeros((T, R), dtype=bool)
            m[t] = True
            yield m


@dataclass(frozen=True)
class Reference:
    loss: float           # fp64
    es: np.ndarray        # (B, K) the blocks' scores
    grad: np.ndarray      # (T, S*B, R) fp64 d loss / d y_hat for the cotangent 1
    dropped: np.ndarray   # (T, S*B, R) bool: the coordinate's target is missing (gradient exactly 0)


@lru_cache(maxsize=None)
def reference(name: str, block: str, fair: bool) -> Reference:
    """Computed once per (case, block, fair) and shared; the arrays are read-only."""
    k = make_case(name)
    T, S, B, R = k.T, k.S, k.B, k.R
    D = S - 1 if fair else S
    assert D >= 1
    K = n_blocks(k, block)
    x = k.yhat.astype(np.float64).reshape(T, S, B, R)
    y = k.y.astype(np.float64)
    es = np.zeros((B, K))
    grad = np.zeros((T, S, B, R))
    with np.errstate(divide="ignore", invalid="ignore"):
        for b in range(B):
            xb = x[:, :, b].transpose(1, 0, 2)                          # (S, T, R)
            for q, m in enumerate(_block_masks(T, R, block)):
                m = m & (y[b] != -1.0)
                if not m.any():
                    continue                                            # no live coordinate: 0, counted in B K
                X, yv = xb[:, m], y[b][m]                               # (S, c), (c,)
                d = X[:, None] - X[None]                                # (S, S, c)
                n = np.sqrt((d * d).sum(-1))                            # (S, S)
                dy = X - yv
                ny = np.sqrt((dy * dy).sum(-1))                         # (S,)
                es[b, q] = ny.sum() / S - n.sum() / (2.0 * S * D)
                first = np.where(ny[:, None] > 0, dy / ny[:, None], 0.0) / S
                pairs = np.where(n[:, :, None] > 0, d / n[:, :, None], 0.0).sum(1) / (S * D)
                gb = np.zeros((S, T, R))
                gb[:, m] = first - pairs
                grad[:, :, b] += gb.transpose(1, 0, 2)
    grad /= B * K
    loss = float(es.sum() / (B * K))
    dropped = np.broadcast_to((k.y == -1.0).transpose(1, 0, 2)[:, None], (T, S, B, R)).reshape(T, S * B, R).copy()
    grad = grad.reshape(T, S * B, R)
    assert not grad[dropped].any()
    for a in (es, grad, dropped):
        a.setflags(write=False)
    return Reference(loss, es, grad, dropped)


def fair_values(name: str):
    return (False, True) if CASES[name][1] >= 2 else (False,)


CASE_BLOCK_FAIR = [(n, blk, f) for n in CASES for blk in BLOCKS for f in fair_values(n)]


def grad_bound(case: Case, block: str, ref_grad: np.ndarray, g: float) -> np.ndarray:
    """The kernels' bar per element of d y_hat: one fp32 rounding of the reference, plus the fp64 roundings of
    the bracket: each of its terms is at most 1 in magnitude, each norm carries at most C + 4 roundings, there
    are S terms."""
    C, K = block_coords(case, block), n_blocks(case, block)
    return 2.0 ** -23 * np.abs(ref_grad) + 2.0 * abs(g) / (case.B * K) * (C + case.S + 8) * 2.0 ** -52
