"""hf_proposal_stats and hf_argmax_accuracy (csrc/eval_stats.hip) on the GPU, through _lib.lib() and ctypes with no Python routing in
between, against the two entry points whose values they must reproduce bit for bit (hf_box3d_iou_matrix, hf_compute_bev_iou), the
NumPy reductions of those matrices (tests/eval_stats_cases.py) and the fp64 clip of tests/sampler_cases.py.

Every output is pre-filled with a sentinel (NaN for floats, -7 for ints) and none may survive; the workspace is exactly the size
hf_proposal_stats_workspace reports, between guard bytes that must be intact after the call."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_stats_cases as ec  # noqa: E402
from abi_harness import Workspace, abi, dev, filled, host, same_array  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def written(got, what, c):
    got = host(got)
    if got.dtype.kind == "f":
        assert not np.isnan(got).any(), "%s of %s: %d elements never written" % (what, ec.case_id(c), int(np.isnan(got).sum()))
    else:
        assert not (got == ec.SENT_I).any(), "%s of %s: %d elements never written" % (what, ec.case_id(c), int((got == ec.SENT_I).sum()))
    return got


def same(got, want, what, c):
    same_array(got, want, what, ec.case_id(c), unwritten=ec.SENT_I)


def _call(L, _lib, c, ins, with_matrices):
    b, m, g = c["b"], c["m"], c["g"]
    props, pc, gt, gc = ins
    out = {"best_iou3d": filled(DEV, (b, m), torch.float32, ec.SENT_I), "best_iou2d": filled(DEV, (b, m), torch.float32, ec.SENT_I),
           "best_gt": filled(DEV, (b, m), torch.int32, ec.SENT_I),
           "counts": filled(DEV, (b, 4), torch.int32, ec.SENT_I), "sums": filled(DEV, (b, 3), torch.float64, ec.SENT_I)}
    if with_matrices:
        out["iou3d"], out["iou2d"] = filled(DEV, (b, m, g), torch.float32, ec.SENT_I), filled(DEV, (b, m, g), torch.float32, ec.SENT_I)
    nbytes = L.hf_proposal_stats_workspace(b, m, g)
    pad = lambda v: (v + 255) & ~255
    assert nbytes == 2 * pad(4 * b * m * g)
    ws = Workspace(DEV, nbytes)
    _lib.check(L.hf_proposal_stats(b, m, g, _lib.ptr(props), _lib.ptr(pc), _lib.ptr(gt) if g > 0 else None, _lib.ptr(gc),
                                   _lib.ptr(out.get("iou3d")), _lib.ptr(out.get("iou2d")), _lib.ptr(out["best_iou3d"]),
                                   _lib.ptr(out["best_iou2d"]), _lib.ptr(out["best_gt"]), _lib.ptr(out["counts"]), _lib.ptr(out["sums"]),
                                   ws.p if nbytes else None, nbytes, _lib.stream_ptr()), "proposal_stats")
    ws.check("hf_proposal_stats")
    return out


def _existing_matrices(t, c):
    """(b, m, g) float32: hf_box3d_iou_matrix, and hf_compute_bev_iou of the boxes3d_to_bev rows per frame (zeros in the padding)"""
    from heterofusionrcnn_amd import modules
    from heterofusionrcnn_amd.bev_iou import compute_bev_iou
    from heterofusionrcnn_amd.rcnn_data import box3d_iou_matrix
    b, m, g = c["b"], c["m"], c["g"]
    iou3 = np.zeros((b, m, g), np.float32)
    iou2 = np.zeros((b, m, g), np.float32)
    if g == 0:
        return iou3, iou2
    props, gt = dev(DEV, t["proposals"]), dev(DEV, t["gt"])
    iou3 = host(box3d_iou_matrix(props, dev(DEV, t["proposal_count"]), gt, dev(DEV, t["gt_count"])))
    for f, fr in enumerate(c["frames"]):
        n, ng = fr["n"], fr["ng"]
        if n and ng:
            iou2[f, :n, :ng] = host(compute_bev_iou(modules.boxes3d_to_bev(props[f, :n]).contiguous(),
                                                    modules.boxes3d_to_bev(gt[f, :ng, :7]).contiguous())[1])
    return iou3, iou2


@pytest.mark.parametrize("c", ec.PROPOSAL_CASES, ids=ec.case_id)
def test_proposal_stats(c):
    _lib, L = abi()
    t = ec.make_proposal_inputs(c)
    b, m, g = c["b"], c["m"], c["g"]
    ins = [dev(DEV, t[k]) for k in ("proposals", "proposal_count", "gt", "gt_count")]
    out = _call(L, _lib, c, ins, True)
    iou3, iou2 = _existing_matrices(t, c)
    same(out["iou3d"], iou3, "iou3d against hf_box3d_iou_matrix", c)
    same(out["iou2d"], iou2, "iou2d against hf_compute_bev_iou", c)
    if any(fr["n"] and fr["ng"] for fr in c["frames"]) and m >= 3:
        assert (iou2 > iou3 + 0.1).any(), "no pair whose BEV IoU is well above its 3D IoU"
    best3, best2, best_gt, counts, sums, mags = ec.ref_proposal_stats(iou3, iou2, t["proposals"], t["proposal_count"], t["gt"], t["gt_count"])
    same(out["best_iou3d"], best3, "best_iou3d", c)
    same(out["best_iou2d"], best2, "best_iou2d", c)
    same(out["best_gt"], best_gt, "best_gt", c)
    same(out["counts"], counts, "counts", c)
    # ... and the counts of the fp64 clip: the margin condition makes the two equal
    for f, (labels, r50, r70) in enumerate(t["recalls"]):
        assert counts[f, 1:].tolist() == [labels, r50, r70], (f, counts[f].tolist(), t["recalls"][f])
    got = written(out["sums"], "sums", c)
    err, bound = np.abs(got - sums), ec.sum_bound(m, mags)
    print("\n%s: sums %s, |error| %s, bound %s" % (ec.case_id(c), got.tolist(), err.tolist(), bound.tolist()))
    assert (err <= bound).all(), (got.tolist(), sums.tolist(), bound.tolist())
    for f, fr in enumerate(c["frames"]):
        if fr["ng"] == 0 or fr["n"] == 0:
            assert got[f].tolist() == [0.0, 0.0, 0.0]
    # NULL matrices: the same remaining outputs; a second call: the same bytes
    for again, with_matrices in ((_call(L, _lib, c, ins, False), False), (_call(L, _lib, c, ins, True), True)):
        for k in out:
            if k in again:
                assert host(out[k]).tobytes() == host(again[k]).tobytes(), "%s of %s differs (matrices %s)" % (k, ec.case_id(c), with_matrices)


def test_proposal_stats_wrapper_writes_table_rows():
    """validate.proposal_stats into rows of a larger table equals the forced call"""
    from heterofusionrcnn_amd import validate
    _lib, L = abi()
    c = next(x for x in ec.PROPOSAL_CASES if x["name"] == "m63_g3_empty_frame_between")
    t = ec.make_proposal_inputs(c)
    ins = [dev(DEV, t[k]) for k in ("proposals", "proposal_count", "gt", "gt_count")]
    want = _call(L, _lib, c, ins, True)
    counts, sums = filled(DEV, (7, 4), torch.int32, ec.SENT_I), filled(DEV, (7, 3), torch.float64, ec.SENT_I)
    got = validate.proposal_stats(*ins, counts=counts[2:5], sums=sums[2:5], matrices=True)
    for k in want:
        assert host(want[k]).tobytes() == host(got[k]).tobytes(), k
    assert torch.equal(counts[2:5], want["counts"]) and (counts[:2] == ec.SENT_I).all() and (counts[5:] == ec.SENT_I).all()
    assert torch.equal(sums[2:5], want["sums"]) and sums[:2].isnan().all() and sums[5:].isnan().all()


@pytest.mark.parametrize("case", ec.ACCURACY_CASES, ids=ec.case_id)
def test_argmax_accuracy(case):
    from heterofusionrcnn_amd import validate
    _lib, L = abi()
    rpg, groups, c = case
    logits, target = ec.make_accuracy_inputs(case)
    want = ec.ref_argmax_accuracy(logits, target, groups)
    lg, tg = dev(DEV, logits), dev(DEV, target)
    table = filled(DEV, (groups + 2,), torch.int32, ec.SENT_I)
    out = table[1:1 + groups]
    _lib.check(L.hf_argmax_accuracy(rpg * groups, c, groups, _lib.ptr(lg), _lib.ptr(tg), ctypes.c_void_p(out.data_ptr()), _lib.stream_ptr()),
               "argmax_accuracy")
    same(out, want, "correct", case)
    assert int(table[0]) == ec.SENT_I and int(table[-1]) == ec.SENT_I, "written outside correct[0 .. groups)"
    same(validate.argmax_accuracy(lg, tg, groups), want, "correct (wrapper)", case)
    if groups == 3:
        assert want[0] == rpg and want[1] == 0
    # one group over all rows: the sum
    same(validate.argmax_accuracy(lg, tg, 1), np.array([want.sum()], np.int32), "correct (one group)", case)
