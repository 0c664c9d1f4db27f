"""The model-configuration lattice, CPU side (tests/lattice_helpers.py; the GPU side is
tests/test_config_lattice_gpu.py).

* Trait coverage: every lattice case has the trait vector of csrc/ude_model.h it was chosen for (printed
  by the header itself through tests/native/ude_traits.cpp), and lattice + configs.PREBUILT together take
  both values of every boolean trait among deterministic models, every SLOTS 1..4 and every depth 2..5.
  A change that moves a threshold (ACT_A4 <= 512, WREG_MAX_Q, SLOTS_ == 1 ...) fails here instead of
  silently emptying a lattice cell.
* The checker is pinned where no golden fixture exists: at every deterministic case the kernel-order
  restatement (fp32, oracle/ude_korder.c) against OracleRHS in fp64 on latent, dy0 and every weight
  gradient, within the bars of test_kernel_order.test_korder_oracle_matches_golden: max(floor, 2 x the
  reference's own fp32-vs-fp64 distance), floor 1e-5 for latent and the statistics, 2e-5 for gradients.
* The fp64 oracle meets the margin condition (lattice_helpers.check_condition) at every case on both
  grids -- for the Bayesian cases at the weight samples of their test's draw stream.
* A configuration too large for the kernels is refused by library_for with the reason (UdeError)."""
import pytest
import torch

import lattice_helpers as lh
from helpers import normwise_rel
from oracle.ude_korder import KernelOrderOracle
from oracle.ude_oracle import OracleRHS


@pytest.mark.parametrize("case", list(lh.LATTICE))
def test_lattice_case_has_its_traits(case):
    tr = lh.traits(lh.LATTICE[case])
    bad = {k: (tr[k], v) for k, v in lh.EXPECTED[case].items() if tr[k] != v}
    assert not bad, f"{case}: ude_model.h no longer gives the traits this case stands for (got, expected): {bad}"


def test_lattice_and_prebuilt_cover_every_trait_value():
    from ude_amd import configs
    all_cfgs = list(dict.fromkeys(list(lh.LATTICE.values()) + list(configs.PREBUILT)))
    det = [lh.traits(c) for c in all_cfgs if not c[0].startswith("B")]
    for name in lh.BOOL_TRAITS:
        assert {tr[name] for tr in det} == {0, 1}, f"{name} takes one value only among deterministic models"
    assert {tr["SLOTS"] for tr in det} == {1, 2, 3, 4}
    assert {tr["D"] for tr in det} == {2, 3, 4, 5}
    # the combinations the lattice exists for
    combos = {(tr["STORE_ACT_D"], tr["SPLIT_BWD_L"], tr["WREG"], tr["FWD_RES"], tr["SPLITX0"], tr["DYF"]) for tr in det}
    assert any(c[:3] == (1, 1, 1) for c in combos)                    # large-record backward, resident weights
    assert any(c[:2] == (1, 1) and c[4:] == (1, 1) for c in combos)   # ... with the small-R paths
    assert any(c[0] == 0 and c[2:4] == (0, 1) for c in combos)        # small record without WREG
    assert any(c[0] == 1 and c[2:4] == (0, 0) for c in combos)        # large record, neither residency
    bay = [lh.traits(c) for c in all_cfgs if c[0].startswith("B")]
    assert {tr["GST"] for tr in bay} == {0, 1}
    assert any(tr["GST"] and tr["R"] not in (10, 49) and tr["R"] > 1 for tr in bay)
    assert any(tr["FULL0"] and tr["L"] != 8 for tr in bay)


@pytest.mark.parametrize("which", lh.GRIDS)
@pytest.mark.parametrize("case", lh.DET)
def test_oracle_meets_margin_condition(case, which):
    refs = lh.references(case, which)                     # asserts the condition
    unplanted = [i for i in range(lh.N_TRAJ) if i not in lh.PLANTED]
    print(f"{case} {which}: min margin {float(refs.margin.min()):.3f}, unplanted "
          f"{float(refs.margin[unplanted].min()):.3f}, smallest |rate before |.|| "
          f"{'-' if refs.kink is None else format(float(refs.kink.min()), '.1e')}")


@pytest.mark.parametrize("which", lh.GRIDS)
@pytest.mark.parametrize("case", lh.BAYES)
def test_bayes_oracle_meets_margin_condition(case, which):
    margin, masks = lh.bayes_condition(case, which)
    lh.check_condition(margin, masks, (case, which))


@pytest.mark.parametrize("case", lh.DET)
def test_korder_oracle_matches_fp64_oracle(pkg, case):
    refs = lh.references(case, "full")
    inp, ref = refs.inp, refs.ref
    kind = refs.cfg[0]
    mod = lh.module_for(pkg, refs.cfg)
    ko = KernelOrderOracle(OracleRHS.from_module(mod, torch.float32))
    out = ko.solve(inp.y0, inp.t, inp.h, threads=4)
    tol = lambda key, floor=1e-5: max(floor, 2.0 * refs.ref32.get(key, 0.0))
    errs = {"latent": normwise_rel(out["latent"], ref.latent)}
    assert errs["latent"] <= tol("latent")
    for key in ("mean", "std", "fa_norm"):
        if getattr(ref, key) is not None:
            errs[key] = normwise_rel(out[key], getattr(ref, key))
            assert errs[key] <= tol(key), (key, errs[key])
    dm, ds, dn = lh._cots(kind)
    dy0, gr, _ = ko.vjp(inp.y0, inp.t, inp.h, inp.dl, dm, ds, dn, stats=out, threads=4)
    errs["y0"] = normwise_rel(dy0, ref.grads["y0"])
    assert errs["y0"] <= tol("y0", 2e-5), errs["y0"]
    for nm in ko.names:
        errs[nm] = normwise_rel(gr[nm], ref.grads[nm])
        assert errs[nm] <= tol(nm, 2e-5), (nm, errs[nm])
    print(f"{case}: kernel-order restatement vs fp64: latent {errs['latent']:.1e}, dy0 {errs['y0']:.1e}, "
          f"weights <= {max(errs[n] for n in ko.names):.1e}")


def test_too_large_configuration_is_refused_with_the_reason():
    """FaFp R = 64 [128, 128, 128] / [128, 128]: the backward record needs more than the 160 KiB LDS
    (ude_model.h's static_assert).  The product refuses it when the library is asked for -- UdeError with
    the reason -- not at launch."""
    from ude_amd import _native
    cfg = lh.TOO_LARGE
    with pytest.raises(lh.TraitError, match="does not fit the 160 KiB LDS"):
        lh.traits(cfg)
    with pytest.raises(_native.UdeError, match="does not fit the 160 KiB LDS"):
        _native.library_for(cfg)
    assert not _native.config_supported(cfg)
