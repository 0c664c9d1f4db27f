"""csrc/ude_sir.h on the host: the one definition of the SIR right-hand side and its VJP that every
kernel calls, compiled with g++ (-ffp-contract=off, as the kernels are) and checked against the model's
equations in torch fp64 on the same fp32 inputs.

Bars (derived, not measured): every output is at most five fp32 roundings of a short sum, so
|got - ref| <= 8 * 2^-24 * m elementwise, m being the reference expression with every operand replaced
by its absolute value and every subtraction by an addition.  Mask decisions, the zeros of dead
(live = false) rows, dq at q = 0, beta / gamma and r_eff are exact."""
import numpy as np
import pytest
import torch

import sir_host_helpers as sh

KINDS = ("FaFp", "Fp", "Fa")
FA_W = float(np.float32(0.37))    # the fp32 value the library receives, so the fp64 reference sees the same input
EPS = 8.0 * 2.0 ** -24
N_RANDOM = 4096


def _inputs(kind):
    g = np.random.default_rng({"FaFp": 1, "Fp": 2, "Fa": 3}[kind])
    f32 = np.float32
    n = N_RANDOM
    Y = g.uniform(-1.6, 2.6, (n, 3)).astype(f32)          # a good share of every component masked
    q = g.standard_normal((n, 2)).astype(f32)
    fa = g.standard_normal((n, 3)).astype(f32)
    cot = g.standard_normal((n, 3)).astype(f32)
    er = g.standard_normal((n, 2)).astype(f32)
    ea = g.standard_normal((n, 3)).astype(f32)
    live = (g.uniform(size=n) < 0.9).astype(np.int32)
    # hand-placed rows: the mask's edges (2 and -1 are inside, one ulp beyond is outside), q = 0,
    # negative q, dead rows
    up, dn = np.nextafter(f32(2), f32(3)), np.nextafter(f32(-1), f32(-2))
    hy = [[2, 2, 2], [-1, -1, -1], [up, up, up], [dn, dn, dn], [2, up, -1], [dn, -1, 2], [up, 0.5, dn],
          [0.6, 0.1, 0.3], [0.6, 0.1, 0.3], [0.6, 0.1, 0.3], [0.6, 0.1, 0.3], [0.6, 0.1, 0.3], [2, -1, up]]
    hq = [[0.4, 0.2]] * 7 + [[0, 0.3], [0.3, 0], [0, 0], [-0.5, -0.25], [0.5, -0.25], [-0.0, 0.2]]
    hl = [1] * 11 + [0, 0]
    h = len(hy)
    Y = np.concatenate([Y, np.array(hy, f32)])
    q = np.concatenate([q, np.array(hq, f32)])
    live = np.concatenate([live, np.array(hl, np.int32)])
    fa = np.concatenate([fa, g.standard_normal((h, 3)).astype(f32)])
    cot = np.concatenate([cot, g.standard_normal((h, 3)).astype(f32)])
    er = np.concatenate([er, g.standard_normal((h, 2)).astype(f32)])
    ea = np.concatenate([ea, g.standard_normal((h, 3)).astype(f32)])
    return dict(Y=Y, q=q, fa=fa, cot=cot, er=er, ea=ea, live=live, n_hand=h)


def _ref_forward(kind, Y, q, fa, absval=False):
    """The model's right-hand side (unmasked) in the tensors' dtype; absval: the magnitude sum m."""
    b, gm = torch.abs(q[:, 0]), torch.abs(q[:, 1])
    S, I = Y[:, 0], Y[:, 1]
    if absval:
        S, I, fa = S.abs(), I.abs(), fa.abs()
    if kind == "Fa":
        return fa, b, gm
    plus = b * S * I
    minus = gm * I
    f = torch.stack([plus, plus + minus, minus] if absval else [-plus, plus - minus, minus], -1)
    if kind == "FaFp":
        f = f + FA_W * fa
    return f, b, gm


@pytest.fixture(scope="module", params=KINDS)
def case(request):
    kind = request.param
    x = _inputs(kind)
    f, rates, r_eff, masked = sh.rhs(kind, x["Y"], x["q"], x["fa"], FA_W)
    dres, dq, dyf, dfa = sh.vjp(kind, x["Y"], x["q"], x["cot"], x["live"], x["er"], x["ea"], FA_W)
    return dict(x, kind=kind, f=f, rates=rates, r_eff=r_eff, masked=masked, dres=dres, dq=dq, dyf=dyf, dfa=dfa)


def _close(got, ref, m, what):
    err = np.abs(got.astype(np.float64) - ref)
    bad = err > EPS * m
    assert not bad.any(), f"{what}: {int(bad.sum())} elements over the bar, worst {float((err / np.maximum(m, 1e-300)).max()) / 2.0 ** -24:.2f} x 2^-24 m"


def test_forward(case):
    kind, Y = case["kind"], case["Y"]
    mask = (Y > np.float32(2)) | (Y < np.float32(-1))
    assert np.array_equal(case["masked"] != 0, mask)
    h = case["n_hand"]
    assert mask[-h:][:4].tolist() == [[False] * 3, [False] * 3, [True] * 3, [True] * 3]
    assert np.all(case["f"][mask] == 0.0)
    t = lambda a: torch.from_numpy(a).double()
    ref, _, _ = _ref_forward(kind, t(Y), t(case["q"]), t(case["fa"]))
    m, _, _ = _ref_forward(kind, t(Y), t(case["q"]), t(case["fa"]), absval=True)
    keep = ~torch.from_numpy(mask)
    _close(case["f"], torch.where(keep, ref, torch.zeros_like(ref)).numpy(), m.numpy(), "f")
    if kind != "Fa":
        b, gm = np.abs(case["q"][:, 0]), np.abs(case["q"][:, 1])
        assert np.array_equal(case["rates"][:, 0], b) and np.array_equal(case["rates"][:, 1], gm)
        with np.errstate(divide="ignore", invalid="ignore"):
            want = (b * Y[:, 0]) / gm                     # fp32: one rounding per operation
        assert want.dtype == np.float32
        assert np.array_equal(case["r_eff"], want, equal_nan=True)   # gamma = 0 rows: inf / nan alike


def test_vjp(case):
    kind, Y, q = case["kind"], case["Y"], case["q"]
    live = case["live"] != 0
    mask = (Y > np.float32(2)) | (Y < np.float32(-1))
    dres_want = np.where(live[:, None] & ~mask, case["cot"], np.float32(0))
    assert np.array_equal(case["dres"], dres_want)
    t = lambda a: torch.from_numpy(a).double()
    # autograd through the fp64 forward: L = <cot, masked f> + <extra, rates> + <extra, Fa> over the live rows
    Yt, qt, fat = t(Y).requires_grad_(True), t(q).requires_grad_(True), t(case["fa"]).requires_grad_(True)
    f, b, gm = _ref_forward(kind, Yt, qt, fat)
    lv = torch.from_numpy(live).double()
    keep = (~torch.from_numpy(mask)).double() * lv[:, None]
    L = (f * keep * t(case["cot"])).sum()
    if kind != "Fa":
        L = L + (lv * (b * t(case["er"][:, 0]) + gm * t(case["er"][:, 1]))).sum()
    if kind != "Fp":
        L = L + (lv[:, None] * fat * t(case["ea"])).sum()
    gY, gq, gfa = torch.autograd.grad(L, [Yt, qt, fat], allow_unused=True)
    ad = np.abs(dres_want.astype(np.float64))
    aS, aI = np.abs(Y[:, 0].astype(np.float64)), np.abs(Y[:, 1].astype(np.float64))
    ab, ag = np.abs(q[:, 0].astype(np.float64)), np.abs(q[:, 1].astype(np.float64))
    if kind != "Fp":
        m = (FA_W if kind == "FaFp" else 1.0) * ad + np.abs(case["ea"].astype(np.float64))
        _close(case["dfa"], gfa.numpy(), m, "dfa")
        assert np.all(case["dfa"][~live] == 0.0)
    if kind != "Fa":
        dpl, dmi = ad[:, 1] + ad[:, 0], ad[:, 2] + ad[:, 1]
        er = np.abs(case["er"].astype(np.float64))
        m_dq = np.stack([dpl * aI * aS + er[:, 0], dmi * aI + er[:, 1]], -1)
        _close(case["dq"], gq.numpy(), m_dq, "dq")
        m_dy = np.stack([dpl * aI * ab, dpl * ab * aS + dmi * ag], -1)
        _close(case["dyf"], gY.numpy()[:, :2], m_dy, "dyf")
        assert np.all(case["dq"][~live] == 0.0) and np.all(case["dyf"][~live] == 0.0)
        assert np.all(case["dq"][q == 0] == 0.0)
        h = case["n_hand"]
        assert (q[-h:] == 0).sum() >= 4 and (q[-h:] < 0).sum() >= 3 and (~live[-h:]).sum() == 2
