"""Brute-force reference and cases of the CRPS training head (the definition at ude_crps_forward in
include/ude_rk4.h), NumPy fp64, independent of the package.

Per group (t, b, r) with samples x_s = y_hat[t, s*B+b, r], target y = y[b, t, r], D = S (fair: S - 1):
  c = (1/S) sum_s |x_s - y| - (1/(2 S D)) sum_i sum_j |x_i - x_j|      (every pair, formed explicitly)
  num_s = D sgn(x_s - y) - (#{x_j < x_s} + #{x_j <= x_s} - S)          (counted directly)
  loss = sum of c over the groups with y != -1, / (B T R);  d loss / d x_s = g / (B T R) * num_s / (S D).
"""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

# (T, S, B, R) and how the inputs are made
CASES = {
    "odd_S": (3, 5, 4, 1),                # odd S, padding rows, fewer groups than a wave
    "dead_columns": (2, 128, 3, 49),      # dead columns in the last workgroup
    "ties": (2, 64, 7, 10),               # repeated samples, targets on a sample and on a tied pair
    "max_S": (1, 1024, 2, 3),             # the largest S, G = 4
    "one_sample": (2, 1, 5, 2),           # S = 1: the masked MAE
    "many_workgroups": (2, 2, 90, 49),    # more than 64 workgroups per time index; fair: D = 1
    "masked_third": (2, 9, 3, 10),        # about a third of the targets -1
    "masked_all": (2, 9, 3, 10),          # every target -1
    "odd_count": (1, 3, 43, 1),           # T S B R = 129 is odd: the workspace (256 + 2 * 129 = 514 bytes) is no
                                          # multiple of 4, and two bytes past a multiple of 512
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
    rng = np.random.default_rng(list(CASES).index(name) + 17)
    y = (2.0 + rng.random((B, T, R))).astype(np.float32)
    x = (y.transpose(1, 0, 2)[:, None] + 0.5 * rng.standard_normal((T, S, B, R))).astype(np.float32)   # (T, S, B, R)
    if name == "ties":
        x[:, 1::4] = x[:, 0::4]                 # every group: 16 tied pairs
        x[:, 10] = x[:, 9] = x[:, 8]            # and a triple
        y[0, 0, 0] = x[0, 6, 0, 0]              # a target exactly on a (single) sample
        y[1, 1, 2] = x[1, 0, 1, 2]              # a target on a tied pair (samples 0 and 1)
        assert x[1, 0, 1, 2] == x[1, 1, 1, 2]
    if name == "masked_third":
        y[rng.random((B, T, R)) < 1.0 / 3.0] = -1.0
        assert 0 < (y == -1).sum() < y.size
    if name == "masked_all":
        y[...] = -1.0
    x.setflags(write=False)
    y.setflags(write=False)
    return Case(name, T, S, B, R, x.reshape(T, S * B, R), y)


@dataclass(frozen=True)
class Reference:
    loss: float           # fp64
    c: np.ndarray         # (T, B, R) per-group value (before the mask)
    num: np.ndarray       # (T, S*B, R) int64 gradient numerators


@lru_cache(maxsize=None)
def reference(name: str, fair: bool) -> Reference:
    """Computed once per (case, fair) and shared; the arrays are read-only."""
    k = make_case(name)
    T, S, B, R = k.T, k.S, k.B, k.R
    D = S - 1 if fair else S
    assert D >= 1
    x = k.yhat.astype(np.float64).reshape(T, S, B, R)
    y = k.y.astype(np.float64).transpose(1, 0, 2)                     # (T, B, R)
    live = y != -1.0
    pair = np.zeros((T, B, R))
    n_lt = np.zeros((T, S, B, R), dtype=np.int64)
    n_le = np.zeros((T, S, B, R), dtype=np.int64)
    for i in range(S):                                               # the double loop over all pairs: i here,
        d = x[:, i:i + 1] - x                                        # j along axis 1
        pair += np.abs(d).sum(1)
        n_lt[:, i] = (d > 0).sum(1)                                  # x_j < x_i
        n_le[:, i] = (d >= 0).sum(1)                                 # x_j <= x_i (j = i included)
    c = np.abs(x - y[:, None]).sum(1) / S - pair / (2.0 * S * D)
    num = D * np.sign(x - y[:, None]).astype(np.int64) - (n_lt + n_le - S)
    num = num * live[:, None]
    loss = float((c * live).sum() / (B * T * R))
    num = num.reshape(T, S * B, R)
    c.setflags(write=False)
    num.setflags(write=False)
    return Reference(loss, c, num)


def reference_grad(name: str, fair: bool, g: float) -> np.ndarray:
    """d loss / d y_hat (T, S*B, R) fp64 for the upstream cotangent g."""
    k = make_case(name)
    D = k.S - 1 if fair else k.S
    return g / (k.B * k.T * k.R) * reference(name, fair).num / (k.S * D)


def fair_values(name: str):
    return (False, True) if CASES[name][1] >= 2 else (False,)


CASE_FAIR = [(n, f) for n in CASES for f in fair_values(n)]


def recovered_numerators(grad: np.ndarray, case: Case, fair: bool, g: float) -> np.ndarray:
    """The integers a gradient was formed from: grad * B T R * S D / g, rounded."""
    D = case.S - 1 if fair else case.S
    return np.rint(grad.astype(np.float64) * (case.B * case.T * case.R) * (case.S * D) / g).astype(np.int64)
