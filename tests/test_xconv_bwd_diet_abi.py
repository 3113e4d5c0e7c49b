"""The X-Conv backward kernels through the C ABI at the shapes where the reworked gradient of X (xc_bwd_x_body of
csrc/xconv_common.h: Wd staged in LDS, scalar row bases, the next trip's loads in flight, accumulators started from the first trip, the
halving exchange across the lanes) can go wrong, on all four entries: hf_xconv_depthwise_grad, hf_xconv_depthwise_gather_grad with and
without a workspace, hf_xconv_depthwise_gather_bn_grad.  References, inputs and bounds are those of tests/xconv_cases.py.

EXACT family (integers in [-2, 2]): every output equals fp64 bit for bit.  On the folded entry z1 is drawn from {1, 2} with gamma = invstd
= 1 and mean = beta = 0, so that F_delta = 1 * (elu(z1) - 0) + 0 = z1 exactly and the same fp64 reference holds.
ROUND family (seeded normals): within n u M of fp64, n from the new add order:
  grad_x   dF_X: M roundings on its longest path (M products, M - 1 adds); its product with F: 1; a lane's ceil(c / 64) trips, the first
           one starting the sum: ceil(c / 64) - 1; the halving exchange over the 64 lanes: 6                      n = M + ceil(c / 64) + 6
which is asserted not to exceed xconv_cases.roundings' M + ceil(c / 64) + 17; the other outputs keep xconv_cases' counts.  On the
folded entry F_delta is the library's own hf_bn_relu_fwd_eval of z1 (the bits the folded kernels rebuild), every output is held to the
bits of the two-launch route, and grad_x to fp64 on top.

Shapes (the smallest at which each path of the new code is taken):
  second_row   8195 rows: grid_for caps at 2048 blocks of 4 waves, so waves 0 .. 2 of block 0 walk a second row: accumulators, the
               prefetched indices and the staged Wd carried from one row into the next; K K = 16, 64, 144 for the exchange
  c_edge       c = 1, 63, 64, 65, 129, 200 (dense); c0 + c1 = 64 + 1, 128 + 1, 192 + 8 (gather, folded): dead lanes in the last trip, one
               trip, a trip on each side of the split at 64 / 128 / 192
  staging      K M ceil(c / 64) = 64 and 72 slots (K = 8, M = 1: c = 512 and 513): either side of kXcWdSlots
  row_edge     1 row; 5 rows with rows_per_cloud = 1 (every row its own cloud); 33 rows in 3 clouds of 11 (a cloud boundary inside a
               block's chunk, the last block of xconv_dw_bwd_fw_kernel holds one row); 131 rows (blocks of 33: an odd chunk, the last 32)
  options      M = 1, 2, 3, 4 dense; M = 1, 2, 4 folded; each of grad_x, grad_f, grad_wd, grad_fts alone and all together
Every gather and folded case is called twice: the same bits."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402
import xconv_runs as xa  # noqa: E402

pytestmark = pytest.mark.gpu

FOLDED_KM = ((8, 1), (8, 2), (8, 4))


def _c(family, regime, k, m, gather, b, p, n, c0, c1, **kw):
    return xc._fused("bwd", family, regime, k, m, gather, b, p, n, c0, c1, **kw)


def _cases():
    out = []
    # second row of a wave
    for fam in ("exact", "round"):
        out.append(_c(fam, "second_row", 8, 1, True, 5, 1639, 9, 64, 6))
    for k, m in ((4, 1), (12, 1)):
        for ch in (3, 70):
            out.append(_c("exact", "second_row", k, m, False, 5, 1639, 9, 0, ch))
    out.append(_c("round", "second_row", 12, 2, False, 5, 1639, 9, 0, 70))
    out.append(_c("exact", "second_row", 4, 4, True, 5, 1639, 9, 64, 6))
    out.append(_c("exact", "second_row", 12, 2, True, 5, 1639, 9, 64, 6))
    # channel edges and the staging threshold
    for fam in ("exact", "round"):
        for ch in (1, 63, 64, 65, 129, 200, 512, 513):
            out.append(_c(fam, "staging" if ch >= 512 else "c_edge", 8, 1, False, 3, 7, 13, 0, ch))
        for c0, c1 in ((64, 1), (128, 1), (192, 8), (64, 448), (64, 449)):
            out.append(_c(fam, "staging" if c1 >= 448 else "c_edge", 8, 1, True, 3, 7, 13, c0, c1))
    for k, m, ch in ((4, 4, 65), (12, 2, 129), (8, 4, 128), (8, 4, 129), (12, 1, 200)):   # 8, 4: 64 and 96 slots
        out.append(_c("exact", "c_edge", k, m, False, 3, 7, 13, 0, ch))
    # row edges
    for k, m in ((8, 1), (8, 4)):
        for b, p, n in ((1, 1, 3), (5, 1, 3), (3, 11, 4), (1, 131, 20)):
            out.append(_c("exact", "row_edge", k, m, True, b, p, n, 64, 36))
    out.append(_c("round", "row_edge", 8, 1, True, 3, 11, 4, 64, 36))
    out.append(_c("exact", "row_edge", 12, 1, False, 5, 1, 3, 0, 70))
    # options
    for m in (1, 2, 3, 4):
        for want in xc.SUBSETS[:3] + (xc.ALL4[:3],):
            out.append(_c("exact", "options", 8, m, False, 3, 7, 13, 64, 36, want=want))
        for want in xc.SUBSETS:
            out.append(_c("exact", "options", 8, m, True, 3, 7, 13, 64, 36, want=want, ws=True))
    return out


CASES = _cases()
FOLDED = [c for c in CASES if c["gather"] and (c["k"], c["m"]) in FOLDED_KM]


@pytest.mark.parametrize("c", CASES, ids=xc.case_id)
def test_backward_entries(c):
    """hf_xconv_depthwise_grad, or hf_xconv_depthwise_gather_grad with a workspace and without one (the same bits in every output but
    grad_wd, which without a workspace is summed by atomics)"""
    t = xc.make_inputs(c)
    got, _ = xa.run_bwd(c, t)
    assert set(got) == set(c["want"])
    xa.check_bwd_short_x(c, t, got, "hf_xconv_depthwise%s_grad" % ("_gather" if c["gather"] else ""))
    if not c["gather"]:
        return
    again, _ = xa.run_bwd(c, t)
    for name in got:
        assert torch.equal(got[name], again[name]), "grad_%s differs between two calls" % name
    other, _ = xa.run_bwd(c, t, ws=not c["ws"])
    xa.check_bwd_short_x(dict(c, ws=not c["ws"]), t, other, "hf_xconv_depthwise_gather_grad")
    for name in got:
        if name != "wd":
            assert torch.equal(got[name], other[name]), "grad_%s differs with and without a workspace" % name


# ------------------------------------------------------------------------------------------------------- the folded entry
@pytest.mark.parametrize("c", FOLDED, ids=xc.case_id)
def test_folded_entry(c):
    t = xa.folded_inputs(c)
    new, old, f = xa.run_folded(c, t)
    assert set(new) == set(c["want"])
    for name in new:
        assert torch.equal(new[name], old[name]), "grad_%s: %d of %d elements are not the bits of the two-launch route" % (
            name, int((new[name] != old[name]).sum()), new[name].numel())
    t["fd"] = f.cpu().numpy().reshape(t["fd"].shape)
    if xa.is_exact(c):
        assert np.array_equal(t["fd"], t["z1"])
    xa.check_bwd_short_x(c, t, new, "hf_xconv_depthwise_gather_bn_grad")
    again, _, _ = xa.run_folded(c, t)
    for name in new:
        assert torch.equal(new[name], again[name]), "grad_%s differs between two calls" % name


def test_the_cases_reach_both_sides_of_the_staging_threshold_and_a_second_row():
    slots = {(xc.cdiv(c["c0"] + c["c1"], 64) * c["k"] * c["m"]) for c in CASES}
    assert 64 in slots and any(s > 64 for s in slots) and any(s < 64 for s in slots)
    assert any(xc.rows_of(c) > 4 * xc.MAX_BLOCKS for c in CASES) and any(xc.rows_of(c) > 4 * xc.MAX_BLOCKS for c in FOLDED)
    assert {c["k"] for c in CASES if xc.rows_of(c) > 4 * xc.MAX_BLOCKS} == {4, 8, 12}
    assert {c["m"] for c in FOLDED} == {1, 2, 4}
