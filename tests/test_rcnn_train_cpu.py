"""CPU tests (-m "not gpu") of the RCNN training pieces (heterofusionrcnn_amd/rcnn_train.py):
the op-by-op torch loss against a literal NumPy restatement of rcnn_model.py:783-810 (masks, class targets) and :1148-1262
(loss, with losses.py:131-200), the configuration against rcnn_multiclass.config, and the argument checks of the new C entry
points (HF_EINVAL before any device work)."""
import ctypes

import numpy as np
import pytest
import torch

from heterofusionrcnn_amd import _lib
from heterofusionrcnn_amd import rcnn_train as RT
from heterofusionrcnn_amd.rcnn import RcnnConfig


def _np_softmax_ce(logits, onehot):
    m = logits.max(-1, keepdims=True)
    lse = np.log(np.exp(logits - m).sum(-1)) + m[:, 0]
    return -(onehot * (logits - lse[:, None])).sum(-1)


def _np_rcnn_loss(cfg, tcfg, cls_logits, head, iou, gt_cls, non_empty, t):
    """rcnn_model.py:783-870 + :1148-1262 with boolean masks, as the reference writes it"""
    n, k1 = cls_logits.shape
    k = k1 - 1
    nbx, nbt = cfg.num_bin_xz, cfg.num_bin_theta
    neg = iou < np.float32(tcfg.cls_neg_iou_range[1])
    pos = iou > np.float32(tcfg.cls_pos_iou_range[0])
    cls_mask = (neg | pos) & non_empty
    cls_gt = np.where(neg, 0, gt_cls)
    onehot = np.eye(k1)[cls_gt]
    ce = _np_softmax_ce(cls_logits[cls_mask].astype(np.float64), onehot[cls_mask])
    ncls = cls_mask.sum()
    box = ce.sum() * tcfg.cls_loss_weight / ncls if ncls > 0 else 0.0
    reg_mask = (iou > np.float32(tcfg.reg_pos_iou_range[0])) & non_empty
    nreg = reg_mask.sum()
    bin_l, reg_l = 0.0, 0.0
    sl1 = lambda d: np.where(np.abs(d) < 1, 0.5 * d * d, np.abs(d) - 0.5)
    for r in np.nonzero(reg_mask)[0]:
        c = gt_cls[r] - 1
        h = head[r, c].astype(np.float64)
        bins = [t["bin_x"][r, c], t["bin_z"][r, c], t["bin_theta"][r]]
        res = [t["res_x"][r, c], t["res_z"][r, c], t["res_theta"][r]]
        off = 0
        for q, nb in enumerate((nbx, nbx, nbt)):
            lg = h[off:off + nb]
            bin_l += _np_softmax_ce(lg[None], np.eye(nb)[bins[q]][None])[0]
            reg_l += sl1(h[off + nb + bins[q]] - res[q])
            off += 2 * nb
        reg_l += sl1(h[off] - t["res_y"][r]) + sl1(h[off + 1:off + 4] - t["res_size"][r]).sum()
    bin_l = bin_l * tcfg.cls_loss_weight / nreg if nreg > 0 else 0.0
    reg_l = reg_l * tcfg.reg_loss_weight / nreg if nreg > 0 else 0.0
    return box, bin_l, reg_l, ncls, nreg


def _case(rng, n, cfg, iou, gt_cls, non_empty):
    k = cfg.num_classes
    d = cfg.head_width
    t = {"bin_x": rng.integers(0, cfg.num_bin_xz, (n, k)).astype(np.int32), "res_x": rng.uniform(-1, 1, (n, k)).astype(np.float32),
         "bin_z": rng.integers(0, cfg.num_bin_xz, (n, k)).astype(np.int32), "res_z": rng.uniform(-1, 1, (n, k)).astype(np.float32),
         "bin_theta": rng.integers(0, cfg.num_bin_theta, (n,)).astype(np.int32), "res_theta": rng.uniform(-1, 1, (n,)).astype(np.float32),
         "res_y": rng.uniform(-2, 2, (n,)).astype(np.float32), "res_size": rng.uniform(-1.5, 1.5, (n, 3)).astype(np.float32)}
    logits = rng.standard_normal((n, k + 1)).astype(np.float32) * 2
    head = (rng.standard_normal((n, k, d)) * 1.5).astype(np.float32)
    return logits, head, iou.astype(np.float32), gt_cls.astype(np.int32), non_empty, t


@pytest.mark.parametrize("kind", ["mixed", "no_cls", "no_reg", "nothing"])
def test_rcnn_loss_against_numpy_restatement(kind):
    cfg, tcfg = RcnnConfig(), RT.RcnnTrainConfig()
    rng = np.random.default_rng({"mixed": 0, "no_cls": 1, "no_reg": 2, "nothing": 3}[kind])
    n = 160
    iou = rng.uniform(0, 1, n)
    iou[:8] = [0.45, 0.6, 0.55, 0.05, 0.4499, 0.6001, 0.5501, 0.0]      # the strict comparisons at the edges
    gt_cls = rng.integers(1, 4, n)
    gt_cls[iou < 0.05] = 0                                               # frames without GT: class 0, IoU 0
    gt_cls[iou == 0.0] = 0
    non_empty = rng.random(n) < 0.85
    if kind == "no_cls":        # every IoU in the gap (0.45, 0.6] -> #cls = 0; some of them > 0.55 -> #reg > 0
        iou = rng.uniform(0.451, 0.6, n)
    elif kind == "no_reg":      # IoU below 0.45 -> #reg = 0, #cls > 0
        iou = rng.uniform(0.0, 0.44, n)
    elif kind == "nothing":
        non_empty[:] = False
    logits, head, iou32, gc, ne, t = _case(rng, n, cfg, iou, gt_cls, non_empty)
    want = _np_rcnn_loss(cfg, tcfg, logits, head, iou32, gc, ne, t)
    tt = {k: torch.from_numpy(v) for k, v in t.items()}
    cl, hd = torch.from_numpy(logits).requires_grad_(True), torch.from_numpy(head).requires_grad_(True)
    total, parts = RT.rcnn_loss(cfg, tcfg, cl, hd, torch.from_numpy(iou32), torch.from_numpy(gc), torch.from_numpy(ne), tt)
    got = [float(parts["box_classification"]), float(parts["bin_classification"]), float(parts["regression"]),
           int(parts["num_cls"]), int(parts["num_reg"])]
    np.testing.assert_allclose(got[:3], want[:3], rtol=1e-5, atol=1e-6)
    assert got[3:] == [int(want[3]), int(want[4])]
    if kind == "no_cls":
        assert got[3] == 0 and got[0] == 0.0 and got[4] > 0
    if kind == "no_reg":
        assert got[4] == 0 and got[1] == 0.0 and got[2] == 0.0 and got[3] > 0
    total.backward()
    assert torch.isfinite(cl.grad).all() and torch.isfinite(hd.grad).all()
    if kind == "nothing":
        assert float(total.detach()) == 0.0 and not cl.grad.any() and not hd.grad.any()


def test_rcnn_train_config_is_rcnn_multiclass_config():
    t = RT.RcnnTrainConfig()
    # rcnn_multiclass.config:285-300 (mini_batch_config) and :276 (aug_roi_method), :208-212 (loss_config)
    assert t.cls_neg_iou_range == (0.05, 0.45) and t.cls_pos_iou_range == (0.60, 1.0)
    assert t.reg_neg_iou_range == (0.0, 0.55) and t.reg_pos_iou_range == (0.55, 1.0)
    assert t.roi_per_sample == 64 and t.fg_ratio == 0.5 and t.hard_bg_ratio == 0.8
    assert t.aug_roi_method == "multiple" and RT.AUG_METHODS[t.aug_roi_method] == 2
    assert t.cls_loss_weight == 1.0 and t.reg_loss_weight == 1.0
    assert t.fg_thresh == 0.55
    # 32 fg slots, 32 bg slots of which int(32 * 0.8) = 25 hard
    assert int(np.round(t.fg_ratio * t.roi_per_sample)) == 32 and int((64 - 32) * t.hard_bg_ratio) == 25


def test_mean_sizes_by_class_row_zero_is_the_class_mean():
    cfg = RcnnConfig()
    got = RT.mean_sizes_by_class(cfg, torch.tensor([0, 1, 2, 3])).numpy()
    sizes = np.asarray(cfg.cluster_sizes, np.float32)
    np.testing.assert_allclose(got[0], sizes.mean(0), rtol=1e-6)
    np.testing.assert_array_equal(got[1:], sizes)


def test_new_entry_points_reject_bad_arguments_without_a_gpu():
    L = _lib.lib()
    fake = ctypes.c_void_p(16)      # never dereferenced: every call below fails its argument check first

    def targets(b=2, m=512, g=40, r=64, aug=2, train=1, fg_ratio=0.5):
        return L.hf_rcnn_proposal_targets(b, m, g, fake, fake, fake, fake, 0.05, 0.45, 0.6, 0.55, r, fg_ratio, 0.8, aug, train, fake,
                                          fake, fake, fake, None, fake, 1 << 30, None)

    assert targets(m=513) == _lib.HF_EINVAL
    assert targets(m=0) == _lib.HF_EINVAL
    assert targets(g=129) == _lib.HF_EINVAL
    assert targets(g=-1) == _lib.HF_EINVAL
    assert targets(r=0) == _lib.HF_EINVAL
    assert targets(r=-5) == _lib.HF_EINVAL
    assert targets(r=513) == _lib.HF_EINVAL
    assert targets(aug=4) == _lib.HF_EINVAL
    assert targets(aug=-1) == _lib.HF_EINVAL
    assert targets(fg_ratio=1.5) == _lib.HF_EINVAL
    assert targets(train=0, r=64) == _lib.HF_EINVAL          # val: one row per proposal
    assert targets(b=-1) == _lib.HF_EINVAL
    assert L.hf_rcnn_targets_workspace(2, 513, 40) == 0 and L.hf_rcnn_targets_workspace(2, 512, 129) == 0
    assert L.hf_rcnn_targets_workspace(2, 512, 40) >= 2 * 512 * 40 * 4
    # the loss pair: more than 7 classes, too many bins, missing pointers
    ws = ctypes.c_size_t(L.hf_rcnn_loss_workspace())
    assert ws.value > 0
    loss = lambda k, nbx, ptrs: L.hf_rcnn_loss_fwd(10, k, nbx, 9, *([ptrs] * 13), 0.45, 0.6, 0.55, 1.0, 1.0, fake, fake, ws, None)
    assert loss(8, 6, fake) == _lib.HF_EINVAL
    assert loss(3, 33, fake) == _lib.HF_EINVAL
    assert loss(3, 6, None) == _lib.HF_EINVAL
    assert L.hf_rcnn_loss_bwd(10, 3, 6, 9, *([None] * 13), 0.45, 0.6, 0.55, 1.0, 1.0, fake, fake, fake, fake, None) == _lib.HF_EINVAL


def test_python_layer_has_no_cpu_fallback():
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        RT.proposal_targets(torch.zeros(1, 4, 7), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 8),
                            torch.zeros(1, dtype=torch.int32), torch.zeros(2, dtype=torch.int64))
