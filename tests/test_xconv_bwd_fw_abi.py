"""The F / Wd gradient kernel (xconv_dw_bwd_fw_kernel of csrc/xconv_common.h) through the C ABI at the shapes where its row loop can go
wrong: a row's X staged in the wave's LDS slot (twice: interleaved by pairs of k, and as it is), two rows of a wave per batch (one where
the registers hold no more: K M >= 24), rows past the block's end clamped and not stored, the cloud's table base carried along the
ascending rows, wave-uniform row bases with 32-bit lane offsets, packed products on pairs of k, and at (8, 4) the depthwise weights read
from the block's reduction buffer.  All four gradient entries: hf_xconv_depthwise_grad, hf_xconv_depthwise_gather_grad with and without
a workspace, hf_xconv_depthwise_gather_bn_grad.  References, inputs, `roundings` and bounds are those of tests/xconv_cases.py; the folded
entry's inputs and runner are those of tests/test_xconv_bwd_diet_abi.py.

EXACT family (integers in [-2, 2]; folded: z1 in {1, 2}, gamma = invstd = 1, mean = beta = 0): every output equals fp64 bit for bit.
ROUND family (seeded normals): within xconv_cases' n u M; the kernel's add order is the one those counts were taken from (every output
element keeps its sequence of multiplies and adds; packing runs across pairs of k or j, never along a sum), so no new count is needed.
The folded entry is also held to the bits of the two-launch route.  Every gather and folded case is called twice: the same bits.
Sentinels surround every output (abi_harness.Arena).

Shapes (the smallest at which each path is taken):
  rows      1 row (three waves have none, the batch has one live row); 5 rows with rows_per_cloud = 1 (every row its own cloud); 33 rows
            in 3 clouds of 11 (a cloud boundary inside a block's chunk and inside a two-row batch, the last block holds one row); 131
            rows (blocks of 32, the last one of 3: an odd chunk); 8195 rows (blocks of 9 rows at c <= 64, of 32 past it: a wave walks a second batch, the
            sums and the table base carried across batches)
  channels  dense c = 1, 63, 64, 65; gather c0 + c1 = 64 + 1 (one live lane in the gathered column), 128 + 1, 192 + 8
  options   (K, M) = (8, 1), (8, 2), (8, 4), (4, 1), (4, 4), (12, 1), (12, 2); folded at (8, 1), (8, 2), (8, 4); each of grad_f, grad_wd,
            grad_fts alone and all together (a gathered column that is asked for nothing returns early), with and without a workspace;
            the staged route (the gathered block's gradient written to the workspace) and the table route"""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402
import xconv_runs as xa  # noqa: E402

pytestmark = pytest.mark.gpu

KM = ((8, 1), (8, 2), (8, 4), (4, 1), (4, 4), (12, 1), (12, 2))
FOLDED_KM = ((8, 1), (8, 2), (8, 4))
ROWS = ((1, 1, 3), (5, 1, 3), (3, 11, 4), (1, 131, 20))     # (clouds, rows per cloud, table rows per cloud)
MANY = (5, 1639, 9)                                         # 8195 rows
G3, D2 = ("f", "wd", "fts"), ("f", "wd")


def _c(family, regime, k, m, gather, bpn, c0, c1, **kw):
    kw.setdefault("want", G3 if gather else D2)
    return xc._fused("bwd", family, regime, k, m, gather, bpn[0], bpn[1], bpn[2], c0, c1, **kw)


def _cases():
    out = []
    for k, m in KM:
        for bpn in ROWS:
            out.append(_c("exact", "row_edge", k, m, True, bpn, 64, 36))
        out.append(_c("exact", "row_edge", k, m, False, ROWS[2], 0, 100))
        out.append(_c("exact", "second_batch", k, m, True, MANY, 64, 6))
    for k, m in ((8, 1), (12, 2)):
        out.append(_c("round", "row_edge", k, m, True, ROWS[2], 64, 36))
        out.append(_c("round", "second_batch", k, m, True, MANY, 64, 6))
    out.append(_c("round", "row_edge", 8, 4, True, ROWS[3], 64, 36))
    out.append(_c("exact", "second_batch", 4, 1, False, MANY, 0, 3))
    out.append(_c("exact", "second_batch", 12, 1, False, MANY, 0, 70))
    out.append(_c("round", "second_batch", 8, 4, False, MANY, 0, 70))
    for ch in (1, 63, 64, 65):
        for fam in ("exact", "round"):
            out.append(_c(fam, "c_edge", 8, 1, False, ROWS[2], 0, ch))
        out.append(_c("exact", "c_edge", 8, 4, False, ROWS[2], 0, ch))
    for k, m in ((4, 4), (12, 2), (8, 2)):
        out.append(_c("exact", "c_edge", k, m, False, ROWS[2], 0, 65))
    for c0, c1 in ((64, 1), (128, 1), (192, 8)):
        for fam in ("exact", "round"):
            out.append(_c(fam, "c_edge", 8, 1, True, ROWS[2], c0, c1))
        for k, m in ((8, 2), (8, 4), (4, 1), (12, 1)):
            out.append(_c("exact", "c_edge", k, m, True, ROWS[2], c0, c1))
    for k, m in ((8, 1), (8, 4), (12, 2)):
        for want in (("f",), ("wd",), ("fts",), xc.ALL4):
            for ws in (True, False):
                out.append(_c("exact", "options", k, m, True, ROWS[2], 64, 36, want=want, ws=ws))
        for want in (("f",), ("wd",), xc.ALL4[:3]):
            out.append(_c("exact", "options", k, m, False, ROWS[2], 0, 100, want=want))
    # the staged route: past 8 MiB of gathered gradient, lists shorter than 8 (xdw_fts_direct false); grad_gathered is written
    for k, m in ((8, 1), (8, 4)):
        out.append(_c("exact", "staged", k, m, True, (4, 1024, 1100), 64, 68, want=G3, ws=True))
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
        if name != "wd" or c["ws"]:
            assert torch.equal(got[name], again[name]), "grad_%s differs between two calls" % name
    other, _ = xa.run_bwd(c, t, ws=not c["ws"])
    xa.check_bwd_short_x(dict(c, ws=not c["ws"]), t, other, "hf_xconv_depthwise_gather_grad")
    for name in got:
        if name != "wd":
            assert torch.equal(got[name], other[name]), "grad_%s differs with and without a workspace" % name


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
        assert (t["fd"] == t["z1"]).all()
    xa.check_bwd_short_x(c, t, new, "hf_xconv_depthwise_gather_bn_grad")
    again, _, _ = xa.run_folded(c, t)
    for name in new:
        assert torch.equal(new[name], again[name]), "grad_%s differs between two calls" % name


def test_the_cases_reach_what_the_row_loop_can_get_wrong():
    bwd = [c for c in CASES]
    assert {(c["k"], c["m"]) for c in bwd} == set(KM) and {(c["k"], c["m"]) for c in FOLDED} == set(FOLDED_KM)
    for k, m in KM:
        mine = [c for c in bwd if (c["k"], c["m"]) == (k, m) and c["gather"]]
        assert {(c["b"], c["p"]) for c in mine} >= {(b, p) for b, p, _ in ROWS} | {MANY[:2]}
    # a second batch: more rows per wave of a block than the batch holds
    for c in bwd:
        if c["regime"] == "second_batch":
            _, _, rpb = xc.xdw_bwd_grid(xc.rows_of(c), c["c0"] + c["c1"])
            assert xc.cdiv(rpb, xc.WAVES) > xc.XC_ROWS
    # 33 rows: two blocks, the last of one row; the cloud boundaries (rows 11, 22) fall inside wave 0's batch of rows 8 and 12 and wave
    # 0's batch of rows 16 and 20 | 24: inside the chunk and inside a batch
    assert xc.xdw_bwd_grid(33, 100) == (2, 2, 32) and xc.xdw_bwd_grid(131, 100) == (5, 2, 32)
    assert {c["c0"] + c["c1"] for c in bwd if not c["gather"]} >= {1, 63, 64, 65}
    assert {(c["c0"], c["c1"]) for c in bwd if c["gather"]} >= {(64, 1), (128, 1), (192, 8)}
    staged = [c for c in bwd if c["regime"] == "staged"]
    assert staged and all(not xc.xdw_fts_direct(xc.rows_of(c), c["n"], c["p"], c["k"], c["c1"], c["m"]) for c in staged)
    assert all(xc.xdw_fts_direct(xc.rows_of(c), c["n"], c["p"], c["k"], c["c1"], c["m"]) for c in bwd if c["regime"] != "staged")
