"""The row-gather case table checked on its own, without a GPU (tests/row_gather_cases.py): every launch regime of
csrc/row_gather.h is reached by a case that says so, the committed oracle and the float32 NumPy restatement agree bit for bit
on every forward and gather-gradient case, and the scatter bound holds for float32 sums of the same addends in any order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import row_gather_cases as rc  # noqa: E402


def test_case_names_are_unique():
    for table in (rc.FORWARD_CASES, rc.GATHER_GRAD_CASES, rc.SCATTER_CASES):
        names = [c["name"] for c in table]
        assert len(set(names)) == len(names)


def test_every_forward_regime_and_edge_is_reached():
    seen = set()
    for c in rc.FORWARD_CASES:
        regime, grid, strided = rc.forward_regime(c)
        assert regime == c["regime"], c["name"]
        assert strided == c["name"].endswith("_many"), (c["name"], grid)
        seen.add((c["nsrc"], regime, strided))
        if c["entry"] == "group_point_into":
            assert regime != "pow2"
    for nsrc in (1, 3):
        assert {(nsrc, "pow2", False), (nsrc, "pow2", True), (nsrc, "vec4", False), (nsrc, "vec4", True), (nsrc, "scalar", False)} <= seen
    pow2_cv = {c["c"] // 4 for c in rc.FORWARD_CASES if c["regime"] == "pow2"}
    assert {4, 256} <= pow2_cv                                   # both ends of the pow2 range
    for c in rc.FORWARD_CASES:                                   # odd row counts: a tail in the last workgroup / the pow2 clamp
        assert c["b"] % 8 != 0 and ((c["m"] * c["k"]) % 2 == 1)


def test_every_gather_gradient_block_shape_is_reached():
    seen = set()
    for c in rc.GATHER_GRAD_CASES:
        vec4, cv, block = rc.gather_grad_block(c)
        assert vec4 == c["vec4"], c["name"]
        seen.add((c["nsrc"], vec4, block > 256, c["ld"] > c["c"]))
        assert block % 64 == 0 and block >= cv
    for nsrc in (1, 3):
        for vec4 in (True, False):
            assert (nsrc, vec4, False, False) in seen and (nsrc, vec4, False, True) in seen
        assert (nsrc, False, True, False) in seen               # c = 300 scalar: 320 lanes
    assert any(c["col"] > 0 and c["ld"] > c["c"] for c in rc.GATHER_GRAD_CASES if c["nsrc"] == 1)


@pytest.mark.parametrize("c", rc.FORWARD_CASES, ids=rc.case_id)
def test_forward_oracle_equals_restatement(oracle_mod, c):
    points, idx, weight = rc.forward_inputs(c)
    want = rc.forward_restated(points, idx, weight)
    got = rc.forward_oracle(oracle_mod, c, points, idx, weight)
    assert want.dtype == np.float32 and np.array_equal(rc.bits(got), rc.bits(want))
    if c["nsrc"] == 1:
        assert np.isnan(points).any() and (rc.bits(points) == np.int32(-2 ** 31)).any()      # NaN payloads and -0.0 are in play


@pytest.mark.parametrize("c", rc.GATHER_GRAD_CASES, ids=rc.case_id)
def test_gather_gradient_oracle_equals_restatement(oracle_mod, c):
    idx, weight, wide = rc.grad_inputs(c)
    want = rc.grad_sequential(c, idx, weight, wide)
    assert np.array_equal(rc.bits(rc.grad_oracle(oracle_mod, c, idx, weight, wide)), rc.bits(want))
    assert not want[:, c["n"] - 1].any() and np.isfinite(want).all()            # the unreferenced target; no NaN column was read
    assert (idx[:, :, 0] == 7).all()                                            # the hub


@pytest.mark.parametrize("c", rc.SCATTER_CASES, ids=rc.case_id)
def test_scatter_bound_holds_for_any_order(c):
    idx, weight, wide = rc.grad_inputs(c)
    ref, bound = rc.scatter_reference(c, idx, weight, wide)
    for seed in range(3):
        got = rc.scatter_shuffled(c, idx, weight, wide, seed)
        assert (np.abs(got.astype(np.float64) - ref) <= bound).all()
    seq = rc.grad_sequential(c, idx, weight, wide)
    assert (np.abs(seq.astype(np.float64) - ref) <= bound).all()
    assert not bound[:, c["n"] - 1].any() and not ref[:, c["n"] - 1].any()      # unreferenced targets: exactly zero
    # the bound is tight enough to catch one dropped or doubled addend of typical size on the hub row
    assert np.median(bound[:, 7]) < 1e-2 * np.median(np.abs(wide[np.isfinite(wide)]))
