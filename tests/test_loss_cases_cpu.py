"""tests/loss_cases.py checked on any machine: the fp64 references against the package's float64 torch forms and their autograd
gradients, the case table against the launch edges it is there for, the restated configuration values, every generator's own assertions
and the sensitivity of the forward bound."""
import dataclasses
import os
import sys
import types

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loss_cases as lc  # noqa: E402

CASES = lc.all_cases()
SMALL = [c for c in CASES if 0 < c["rows"] <= 300]


def test_case_ids_are_unique_and_counted():
    ids = [lc.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    assert len(ids) == 35, "a case was added or removed: update this number when you add a case"


# ------------------------------------------------------------------------------------------------- the restated facts
def test_launch_rule_restated_from_the_entry_points():
    assert [lc.fwd_blocks(r) for r in (0, 1, 255, 256, 257)] == [1, 1, 1, 1, 2]
    assert lc.fwd_blocks(lc.FWD_STRIDE) == 1024 == lc.fwd_blocks(10 ** 7) and lc.fwd_blocks(lc.FWD_STRIDE - 256) == 1023
    assert [lc.fwd_trips(r) for r in (0, 1, 257, 262144, 262145, 524288, 524365, 1048577)] == [0, 1, 1, 1, 2, 2, 3, 5]
    assert [lc.bwd_blocks(r) for r in (1, 256, 257, 1048576, 1048577)] == [1, 1, 2, 4096, 4096]
    assert [lc.bwd_trips(r) for r in (0, 1, 257, 1048576, 1048577)] == [0, 1, 1, 1, 2]
    assert lc.head_width(12, 12) == 76 and lc.head_width(2, 2) == 16 and lc.head_width(32, 1) == 134
    assert lc.head_groups(5, 32) == ((0, 5), (10, 5), (20, 32)) and lc.head_tail(5, 32) == 84 == lc.head_width(5, 32) - 4
    assert lc.limits_ok(7, 32, 32) and lc.limits_ok(1, 1, 1)
    assert not any(lc.limits_ok(*s) for s in ((0, 1, 1), (8, 1, 1), (1, 0, 1), (1, 33, 1), (1, 1, 0), (1, 1, 33)))


def test_configuration_values_restated():
    from heterofusionrcnn_amd import rcnn, rcnn_train, rpn
    a = rpn.rpn_stack_config2()
    b = rpn.rpn_multiclass_heads(a)
    r = rcnn.RcnnConfig()
    t = rcnn_train.RcnnTrainConfig()
    assert lc.CONFIG_SHAPES == {"rpn_stack_config2": (a.num_classes, a.num_bin_xz, a.theta_bin_num),
                                "rpn_multiclass_heads": (b.num_classes, b.num_bin_xz, b.theta_bin_num),
                                "rcnn": (r.num_classes, r.num_bin_xz, r.num_bin_theta)}
    assert lc.RCNN_THRESHOLDS == (t.cls_neg_iou_range[1], t.cls_pos_iou_range[0], t.reg_pos_iou_range[0])
    assert lc.RPN_WEIGHTS == (a.seg_loss_weight, a.cls_loss_weight, a.reg_loss_weight) and (t.cls_loss_weight, t.reg_loss_weight) == (1.0, 1.0)
    assert a.head_width == lc.head_width(*lc.CONFIG_SHAPES["rpn_stack_config2"][1:]) and r.head_width == lc.head_width(*lc.CONFIG_SHAPES["rcnn"][1:])


def test_workspace_sizes_restated():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    assert L.hf_rpn_loss_workspace() == lc.rpn_workspace() == 16384 and L.hf_rcnn_loss_workspace() == lc.rcnn_workspace() == 20480


# ------------------------------------------------------------------------------------------------- the case table
@pytest.mark.parametrize("kind", ["rpn", "rcnn"])
def test_the_case_table_holds_what_it_must(kind):
    cases = lc.cases_of(kind)
    rows = {c["rows"] for c in cases}
    for r in lc.FWD_ROWS + lc.BWD_ROWS:
        assert r in rows, "no %s case of %d rows" % (kind, r)
    # both sides of every launch edge: one block / two, one trip / two / three in the forward, one trip / two in the backward
    assert {lc.fwd_blocks(r) for r in rows if r <= 257} == {1, 2} and {255, 256, 257} <= rows
    assert {1, 2, 3} <= {lc.fwd_trips(r) for r in rows} and {lc.fwd_trips(lc.FWD_STRIDE), lc.fwd_trips(lc.FWD_STRIDE + 1)} == {1, 2}
    assert {1, 2} <= {lc.bwd_trips(r) for r in rows} and {lc.bwd_trips(lc.BWD_STRIDE), lc.bwd_trips(lc.BWD_STRIDE + 1)} == {1, 2}
    shapes = {(c["k"], c["nbx"], c["nbt"]) for c in cases}
    own = ("rpn_stack_config2", "rpn_multiclass_heads") if kind == "rpn" else ("rcnn",)
    assert set(lc.EDGE_SHAPES) <= shapes and {lc.CONFIG_SHAPES[n] for n in own} <= shapes
    assert any(c["nbx"] != c["nbt"] for c in cases) and {1, 32} <= {c["nbx"] for c in cases} and {1, 32} <= {c["nbt"] for c in cases} and 7 in {c["k"] for c in cases}
    for c in cases:
        if c["rows"] > 300:
            assert (c["k"], c["nbx"], c["nbt"]) == lc.BIG_SHAPE and lc.head_width(c["nbx"], c["nbt"]) == 16
    assert {c["upstream"] for c in cases} == set(lc.UPSTREAMS)
    assert {c["mix"] for c in cases} == set(lc.RPN_MIXES if kind == "rpn" else lc.RCNN_MIXES)
    assert sum(c["off"] for c in cases) == 1
    assert any(c["weights"][-2] != c["weights"][-1] for c in cases), "the two box weights must differ somewhere"
    if kind == "rpn":
        assert any(c["logits"] == "gap40" and c["upstream"] != 0 for c in cases)
        assert any(c["mix"] == "one_fg_last" and lc.fwd_trips(c["rows"]) > 1 for c in cases) and any(c["mix"] == "one_fg_last" and lc.bwd_trips(c["rows"]) > 1 for c in cases)


@pytest.mark.parametrize("c", CASES, ids=lc.case_id)
def test_generator_satisfies_its_own_assertions(c):
    """make_inputs asserts the distance of p_t from the clip points and the caller's contract; here: the mix the case is named for"""
    t = lc.make_inputs(c)
    rows, k = c["rows"], c["k"]
    names = lc.RPN_ARGS if c["kind"] == "rpn" else lc.RCNN_ARGS
    assert all(t[n].dtype in (np.float32, np.int32) and t[n].shape[0] == rows and t[n].flags.c_contiguous for n in names)
    assert t["head"].shape == (rows, k, lc.head_width(c["nbx"], c["nbt"]))
    if c["kind"] == "rpn":
        lab = t["label"]
        assert lab.min(initial=0) >= -1 and lab.max(initial=0) <= k
        nfg, nign = int((lab > 0).sum()), int((lab < 0).sum())
        want = {"background": nfg == 0 and nign == 0, "foreground": nfg == rows, "ignored": nign == rows, "class_k": bool((lab == k).all()),
                "one_fg_last": nfg == 1 and lab[-1:].tolist() == [k], "mixed": rows < 255 or (nfg > 0 and nign > 0 and nfg + nign < rows)}
        assert want[c["mix"]]
        if c["mix"] == "mixed" and rows >= 255 and k > 1:
            assert set(lab.tolist()) == set(range(-1, k + 1))
    else:
        cmask, tgt, rmask = lc.rcnn_masks(c, t)
        ncls, nreg = int(cmask.sum()), int(rmask.sum())
        mix = c["mix"]
        if mix == "uniform" and rows:
            assert cmask[-1] and rmask[-1] and (rows < 255 or (0 < nreg < ncls < rows))
        if mix == "thresholds":
            nh, pl, rl = (np.float32(v) for v in c["thresholds"])
            v = lc.threshold_values(c["thresholds"])
            assert len(set(v.tolist())) == 9 and set(t["iou"].tolist()) == set(v.tolist())
            assert [bool(x < nh) for x in v[0:3]] == [True, False, False] and [bool(x > pl) for x in v[3:6]] == [False, False, True]
            assert [bool(x > rl) for x in v[6:9]] == [False, False, True]
        if mix == "class0":
            assert nreg > 0 and (t["gt_cls"] == 0).all()
        if mix == "class_outside":
            out = cmask & ((tgt < 0) | (tgt > k))
            assert {-1, k + 1} <= set(tgt[out].tolist()) and not (out & rmask).any() and (cmask & (tgt == 0) & (t["gt_cls"] == k + 1)).any()
        if mix == "empty":
            assert ncls == 0 and nreg == 0
        if mix == "non_empty_7":
            assert set(t["non_empty"].tolist()) == {0, 7} and nreg > 0
        if mix == "below_neg_hi":
            assert ncls > 0 and nreg == 0


# ------------------------------------------------------------------------------------------------- references against the torch forms
def _torch_rpn(c, t):
    from heterofusionrcnn_amd import rpn
    w = [float(np.float32(v)) for v in c["weights"]]
    cfg = dataclasses.replace(rpn.rpn_stack_config2(), num_classes=c["k"], xz_search_range=(c["nbx"] / 2.0,), xz_bin_len=(1.0,), theta_bin_num=c["nbt"],
                              seg_loss_weight=w[0], cls_loss_weight=w[1], reg_loss_weight=w[2])
    assert (cfg.num_bin_xz, cfg.theta_bin_num) == (c["nbx"], c["nbt"])
    rows = c["rows"]
    seg = torch.tensor(t["seg_logits"], dtype=torch.float64).reshape(1, rows, -1).requires_grad_()
    head = torch.tensor(t["head"], dtype=torch.float64).reshape(1, rows, c["k"], -1).requires_grad_()
    lab = torch.from_numpy(t["label"]).long().reshape(1, rows)
    cls0 = torch.clamp(lab - 1, min=0)
    pick = lambda a, dt: torch.gather(torch.tensor(a, dtype=dt).reshape(1, rows, -1), 2, cls0.unsqueeze(-1)).squeeze(-1)
    f = lambda a: torch.tensor(a, dtype=torch.float64).reshape((1,) + a.shape)
    targets = {"cls0": cls0, "bin_x": pick(t["bin_x"], torch.int64), "res_x": pick(t["res_x"], torch.float64), "bin_z": pick(t["bin_z"], torch.int64),
               "res_z": pick(t["res_z"], torch.float64), "bin_theta": torch.from_numpy(t["bin_theta"]).long().reshape(1, rows), "res_theta": f(t["res_theta"]),
               "res_y": f(t["res_y"]), "res_size": f(t["res_size"])}
    loss, parts = rpn.rpn_loss(cfg, seg, head, lab, targets)
    (loss * float(np.float32(c["upstream"]))).backward()
    out = [parts["segmentation"], parts["bin_classification"], parts["regression"], parts["num_foreground"], loss.detach()]
    return np.array([float(v) for v in out]), seg.grad[0].numpy(), head.grad[0].numpy()


def _torch_rcnn(c, t):
    from heterofusionrcnn_amd import rcnn_train
    w = [float(np.float32(v)) for v in c["weights"]]
    nh, pl, rl = c["thresholds"]
    cfg = types.SimpleNamespace(num_bin_xz=c["nbx"], num_bin_theta=c["nbt"])
    tcfg = rcnn_train.RcnnTrainConfig(cls_neg_iou_range=(0.05, nh), cls_pos_iou_range=(pl, 1.0), reg_pos_iou_range=(rl, 1.0), cls_loss_weight=w[0],
                                      reg_loss_weight=w[1])
    logits = torch.tensor(t["cls_logits"], dtype=torch.float64).requires_grad_()
    head = torch.tensor(t["head"], dtype=torch.float64).requires_grad_()
    targets = {n: torch.tensor(t[n], dtype=torch.int64 if n.startswith("bin") else torch.float64) for n in lc.RCNN_ARGS[5:]}
    loss, parts = rcnn_train.rcnn_loss(cfg, tcfg, logits, head, torch.from_numpy(t["iou"]), torch.from_numpy(t["gt_cls"]), torch.from_numpy(t["non_empty"]), targets)
    (loss * float(np.float32(c["upstream"]))).backward()
    out = [parts["box_classification"], parts["bin_classification"], parts["regression"], parts["num_cls"], parts["num_reg"], loss.detach()]
    return np.array([float(v) for v in out]), logits.grad.numpy(), head.grad.numpy()


@pytest.mark.parametrize("c", SMALL, ids=lc.case_id)
def test_references_equal_the_float64_torch_forms(c):
    """rpn.rpn_loss (pinned to the literal reference graph by test_rpn.py) and rcnn_train.rcnn_loss in float64, with autograd.  The small
    cases hold the ignore label, #fg == 0, the class-0 regression rows, the thresholds at equality and the classes outside 0..k"""
    t = lc.make_inputs(c)
    r = lc.REF[c["kind"]](c, t)
    out, g_logits, g_head = (_torch_rpn if c["kind"] == "rpn" else _torch_rcnn)(c, t)
    np.testing.assert_allclose(r["out"], out, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r[lc.LOGIT_GRAD[c["kind"]]], g_logits, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(r["grad_head"], g_head, rtol=1e-12, atol=1e-12)
    # what the reference calls structurally zero is zero in autograd too, bit for bit
    assert (g_head[~r["live_head"]] == 0).all() and (g_logits[~r[lc.LOGIT_LIVE[c["kind"]]]] == 0).all()
    assert (r["grad_head"][~r["live_head"]] == 0).all()


def test_small_cases_cover_the_branches_the_torch_comparison_is_for():
    rpn = [c for c in SMALL if c["kind"] == "rpn"]
    assert any(c["mix"] == "ignored" for c in rpn) and any(c["mix"] == "background" for c in rpn) and any(c["logits"] == "gap40" for c in rpn)
    rcnn = {c["mix"] for c in SMALL if c["kind"] == "rcnn"}
    assert {"class0", "thresholds", "class_outside", "below_neg_hi", "empty"} <= rcnn


def test_gap_rows_have_the_clipped_term_and_no_gradient():
    c = next(c for c in CASES if c["logits"] == "gap40")
    t = lc.make_inputs(c)
    r = lc.ref_rpn(c, t)
    rows = np.arange(c["rows"])
    valid = t["label"] >= 0
    up, down = (rows % 3 == 1) & valid, (rows % 3 == 2) & valid
    assert up.sum() > 50 and down.sum() > 50
    assert not r["live_seg"][up | down].any() and r["live_seg"][(rows % 3 == 0) & valid].all() and (r["grad_seg"][up | down] == 0).all()
    full = np.zeros(c["rows"])
    full[valid] = r["seg"]
    np.testing.assert_allclose(full[down], 0.25 * (1 - 1e-7) ** 2 * -np.log(1e-7), rtol=1e-12)
    np.testing.assert_allclose(full[up], 0.25 * 1e-14 * -np.log1p(-1e-7), rtol=1e-6)


# ------------------------------------------------------------------------------------------------- sensitivity of the bounds
@pytest.mark.parametrize("kind", ["rpn", "rcnn"])
def test_forward_bound_admits_fp32_and_rejects_a_block_of_rows_taken_twice(kind):
    """at 262 145 rows a forward stride one workgroup short takes rows 0..256 twice: each part of the output moves by more than its
    bound; a sequential fp32 sum of the fp32 terms (a chain far longer than any thread's) stays inside the bound of a thread chain that long"""
    c = next(c for c in lc.cases_of(kind) if c["rows"] == lc.FWD_STRIDE + 1 and c["mix"] in ("mixed", "uniform", "one_fg_last"))
    t = lc.make_inputs(c)
    r64, r32 = lc.REF[kind](c, t), lc.REF[kind](c, t, np.float32)
    bound = lc.forward_bounds(c, r64, r32)
    assert (bound[:3] >= 0).all() and (bound[3:-1] == 0).all()
    first = lc.TERMS[kind][0]
    terms, w, div = r64[first], lc.weights_of(c)[0], r64["divisors"][0]
    if kind == "rpn":
        twice = terms[:257 - int((t["label"][:257] < 0).sum())].sum()
    else:
        live = r64["live_cls"]
        twice = terms[:int(live[:257].sum())].sum()
    assert twice * w / div > 20 * bound[0] and bound[0] < 1e-4 * abs(r64["out"][0])
    got = np.float32(np.float32(r32[first].sum(dtype=np.float32)) * np.float32(w) / np.float32(div))
    assert abs(float(got) - r64["out"][0]) <= bound[0]


def test_backward_bound_rejects_the_neighbouring_divisor():
    """#fg + 1 for max(#fg, 1) moves every element of grad_head by 1 / (#fg + 1) of itself: far outside the bound at 86 foreground rows"""
    c = next(c for c in lc.cases_of("rpn") if c["rows"] == 257 and c["mix"] == "foreground")
    t = lc.make_inputs(c)
    r64, r32 = lc.ref_rpn(c, t), lc.ref_rpn(c, t, np.float32)
    b = lc.grad_bound(r32["grad_head"], r64["grad_head"])
    nfg = r64["counts"][0]
    moved = np.abs(r64["grad_head"]) / (nfg + 1)
    assert 0 < b < 1e-5 * np.abs(r64["grad_head"]).max() and (moved > b).mean() > 0.5
    assert (np.abs(r32["grad_head"].astype(np.float64) - r64["grad_head"]) <= b).all()
