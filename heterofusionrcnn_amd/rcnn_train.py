"""Training of the second stage (RCNN): the proposal-target layer on the device and the RCNN loss.

  proposal targets     kitti_dataset.py:440-770          sample_rois_for_rcnn_training, sample_bg_inds, aug_roi_by_noise,
                                                         random_aug_box3d: a host NumPy loop calling shapely per RoI in the
                                                         reference; here hf_rcnn_proposal_targets (csrc/rcnn_targets.hip),
                                                         three launches with no host read, so the step can be captured
  targets and masks    rcnn_model.py:783-870             cls / reg masks from the RoI's IoU, tf_encode around the RoI
                                                         (centre, heading), mean sizes by GT class (_gather_cls_mean_sizes)
  loss                 rcnn_model.py:1148-1262,           softmax cross-entropy / #cls, three bin cross-entropies / #reg,
                       losses.py:131-200                  smooth-L1 of the residuals / #reg

rcnn_loss is the op-by-op torch restatement (runs on CPU); rcnn_loss_fused is the same loss as one HIP forward / backward pair
(hf_rcnn_loss_fwd / _bwd in csrc/glue.hip).  RcnnTrainer chains targets -> RcnnModel -> encoding -> loss; rcnn_train_loss is
its loss_fn for graph_step.TrainStep.

Parity is unpinned against reference outputs (TensorFlow and shapely are not importable, and the random streams differ).
What the tests pin: the target layer draw for draw against a NumPy restatement of its counter hash, rules and jitter, its
3D IoU against an fp64 clip (tests/sampler_cases.py, tests/test_sampler_abi.py), and the loss graph.
"""
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import _lib, box_codec
from ._lib import check, dev_tensor, ptr, require, stream_ptr
from .rcnn import RcnnConfig, RcnnModel
from .rpn import parse_rpn_output

AUG_METHODS = {"": 0, "none": 0, "single": 1, "multiple": 2, "normal": 3}


@dataclass
class RcnnTrainConfig:
    """rcnn_multiclass.config:208-212 (loss weights) and :275-300 (aug_roi_method, mini_batch_config)."""
    cls_neg_iou_range: Tuple[float, float] = (0.05, 0.45)       # CLS_BG_THRESH_LO, CLS_BG_THRESH
    cls_pos_iou_range: Tuple[float, float] = (0.60, 1.0)        # CLS_FG_THRESH
    reg_neg_iou_range: Tuple[float, float] = (0.0, 0.55)
    reg_pos_iou_range: Tuple[float, float] = (0.55, 1.0)        # REG_FG_THRESH
    roi_per_sample: int = 64
    fg_ratio: float = 0.5
    hard_bg_ratio: float = 0.8
    aug_roi_method: str = "multiple"
    cls_loss_weight: float = 1.0
    reg_loss_weight: float = 1.0

    @property
    def fg_thresh(self):
        return min(self.reg_pos_iou_range[0], self.cls_pos_iou_range[0])      # kitti_dataset.py:559


# ------------------------------------------------------------------------------------------------ proposal targets
def proposal_targets(proposals, proposal_count, gt, gt_count, rng_state=None, cfg: RcnnTrainConfig = None, train=True,
                     aug_method=None):
    """hf_rcnn_proposal_targets.  proposals (B,m,7), proposal_count (B,) int32 valid rows; gt (B,g,8) [x,y,z,l,w,h,ry,cls 1..K]
    padded, gt_count (B,) int32; rng_state (2,) int64 on the device [base seed, call number], advanced by the call (train only).
    train=True -> (rois (B,R,7), iou_of_rois (B,R), gt_of_rois (B,R,8), stats (B,4) [#fg, #bg, sampled fg, sampled bg]);
    train=False (val) -> the same for every proposal (R = m), no sampling.  aug_method overrides cfg.aug_roi_method."""
    cfg = cfg or RcnnTrainConfig()
    require(proposals.dim() == 3 and proposals.shape[2] == 7, "proposals must be (B, m, 7)")
    require(gt.dim() == 3 and gt.shape[2] == 8 and gt.shape[0] == proposals.shape[0], "gt must be (B, g, 8)")
    b, m, _ = proposals.shape
    g = gt.shape[1]
    require(tuple(proposal_count.shape) == (b,) and tuple(gt_count.shape) == (b,), "counts must be (B,)")
    method = cfg.aug_roi_method if aug_method is None else aug_method
    aug = AUG_METHODS.get(method, -1) if isinstance(method, str) else int(method)
    r = cfg.roi_per_sample if train else m
    props = dev_tensor(proposals.detach(), torch.float32, "proposals")
    gts = dev_tensor(gt.detach(), torch.float32, "gt")
    pc = dev_tensor(proposal_count, torch.int32, "proposal_count")
    gc = dev_tensor(gt_count, torch.int32, "gt_count")
    state = None
    if train:
        require(rng_state is not None, "train mode needs an rng_state")
        state = dev_tensor(rng_state, torch.int64, "rng_state")
        require(state.numel() == 2 and state.data_ptr() == rng_state.data_ptr(), "rng_state must be a contiguous (2,) int64 tensor")
    L = _lib.lib()
    nbytes = L.hf_rcnn_targets_workspace(b, m, g)
    dev = props.device
    ws = torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=dev)
    rois = torch.empty((b, r, 7), dtype=torch.float32, device=dev)
    iou = torch.empty((b, r), dtype=torch.float32, device=dev)
    gt_of = torch.empty((b, r, 8), dtype=torch.float32, device=dev)
    stats = torch.empty((b, 4), dtype=torch.int32, device=dev)
    c_neg, c_pos, r_pos = cfg.cls_neg_iou_range, cfg.cls_pos_iou_range, cfg.reg_pos_iou_range
    check(L.hf_rcnn_proposal_targets(b, m, g, ptr(props), ptr(pc), ptr(gts) if g > 0 else None, ptr(gc), float(c_neg[0]), float(c_neg[1]),
                                     float(c_pos[0]), float(r_pos[0]), int(r), float(cfg.fg_ratio), float(cfg.hard_bg_ratio), aug,
                                     1 if train else 0, ptr(state), ptr(rois), ptr(iou), ptr(gt_of), ptr(stats), ptr(ws), int(nbytes),
                                     stream_ptr()), "rcnn_proposal_targets")
    return rois, iou, gt_of, stats


# ------------------------------------------------------------------------------------------------ encoding
def mean_sizes_by_class(cfg: RcnnConfig, gt_cls):
    """_gather_cls_mean_sizes (rcnn_model.py:361-388): row 0 (background) = the mean of the class sizes, rows 1..K the classes"""
    sizes = np.asarray(cfg.cluster_sizes, dtype=np.float32).reshape(-1, 3)
    table = np.concatenate([sizes.mean(axis=0, keepdims=True), sizes], axis=0)
    t = box_codec.const_f32(gt_cls.device, table)
    return t[gt_cls.long().clamp(0, sizes.shape[0])]


def rcnn_encode(cfg: RcnnConfig, rois, gt_of_rois):
    """rcnn_model.py:812-836: tf_encode of the assigned GT boxes around the RoIs (ref point = RoI centre, ref angle = RoI heading;
    the RCNN's rank-2 orientation rule) -> dict of the per-class targets"""
    rois, gt_of_rois = rois.reshape(-1, 7), gt_of_rois.reshape(-1, 8)
    ms = mean_sizes_by_class(cfg, gt_of_rois[:, 7])
    enc = box_codec.encode(rois[:, 0:3].contiguous(), rois[:, 6].contiguous(), gt_of_rois[:, 0:7].contiguous(), ms.contiguous(),
                           cfg.xz_search_range, cfg.xz_bin_len, cfg.r_theta, cfg.delta_theta, cfg.num_classes)
    return dict(zip(("bin_x", "res_x", "bin_z", "res_z", "bin_theta", "res_theta", "res_y", "res_size"), enc))


_ENC_KEYS = ("bin_x", "res_x", "bin_z", "res_z", "bin_theta", "res_theta", "res_y", "res_size")


# ------------------------------------------------------------------------------------------------ loss
def rcnn_loss(cfg: RcnnConfig, tcfg: RcnnTrainConfig, cls_logits, head, iou, gt_cls, non_empty, targets):
    """rcnn_model.py:783-870 (masks, targets of the GT class) + :1148-1262 (loss) op by op.  cls_logits (N,K+1), head (N,K,D),
    iou / gt_cls / non_empty (N,), targets as rcnn_encode returns them.  No boolean_mask: the masks multiply, so shapes are
    static.  -> (total, parts)"""
    n, k1 = cls_logits.shape
    k = k1 - 1
    nbx, nbt = cfg.num_bin_xz, cfg.num_bin_theta
    gt_cls = gt_cls.long()
    ne = non_empty.bool()
    # box_cls_gt (:783-801)
    neg = iou < tcfg.cls_neg_iou_range[1]
    pos = iou > tcfg.cls_pos_iou_range[0]
    cls_mask = (neg | pos) & ne
    cls_gt = torch.where(neg, torch.zeros_like(gt_cls), gt_cls)
    one_hot = (torch.arange(k1, device=cls_logits.device)[None, :] == cls_gt[:, None]).to(cls_logits.dtype)
    ce = -(one_hot * F.log_softmax(cls_logits, dim=-1)).sum(-1)
    cmf = cls_mask.to(cls_logits.dtype)
    num_cls = cmf.sum()
    box_cls = (ce * cmf).sum() * tcfg.cls_loss_weight / torch.clamp(num_cls, min=1.0)
    # box_cls_reg_gt (:804-870): the GT class's row of the head and of the x / z targets (class index max(cls - 1, 0))
    reg_mask = (iou > tcfg.reg_pos_iou_range[0]) & ne
    rmf = reg_mask.to(head.dtype)
    num_reg = rmf.sum()
    c = torch.clamp(gt_cls - 1, min=0, max=k - 1)
    row = head[torch.arange(n, device=head.device), c]                                   # (N, D)
    bx, rx, bz, rz, bt, rt, ry, rs = parse_rpn_output(row, nbx, nbx, nbt)
    pick = lambda t: torch.gather(t, 1, c[:, None]).squeeze(1)
    tbx, tbz, tbt = pick(targets["bin_x"]).long(), pick(targets["bin_z"]).long(), targets["bin_theta"].long().reshape(n)
    trx, trz = pick(targets["res_x"]), pick(targets["res_z"])

    def ce_bins(logits, target):
        return (F.cross_entropy(logits, target, reduction="none") * rmf).sum()

    bin_cls = (ce_bins(bx, tbx) + ce_bins(bz, tbz) + ce_bins(bt, tbt)) * tcfg.cls_loss_weight / torch.clamp(num_reg, min=1.0)
    take = lambda res, bins: torch.gather(res, 1, bins[:, None]).squeeze(1)             # _gather_cls_residuals: the TRUE bin

    def sl1(pred, target):
        d = (pred - target).abs()
        v = torch.where(d < 1, 0.5 * d * d, d - 0.5)
        if v.dim() == 2:
            v = v.sum(-1)
        return (v * rmf).sum()

    reg = (sl1(take(rx, tbx), trx) + sl1(take(rz, tbz), trz) + sl1(take(rt, tbt), targets["res_theta"].reshape(n)) +
           sl1(ry, targets["res_y"].reshape(n)) + sl1(rs, targets["res_size"].reshape(n, 3))) * tcfg.reg_loss_weight / \
        torch.clamp(num_reg, min=1.0)
    total = box_cls + bin_cls + reg
    return total, {"box_classification": box_cls.detach(), "bin_classification": bin_cls.detach(), "regression": reg.detach(),
                   "num_cls": num_cls.detach(), "num_reg": num_reg.detach()}


class _RcnnLossFused(torch.autograd.Function):
    """hf_rcnn_loss_fwd / hf_rcnn_loss_bwd.  Returns [box cls, bin cls, regression, #cls, #reg, total]; only the total carries a
    gradient."""

    @staticmethod
    def forward(ctx, cls_logits, head, iou, gt_cls, non_empty, enc, meta):
        L = _lib.lib()
        k, nbx, nbt, thr, w = meta
        rows = iou.numel()
        out6 = torch.empty((6,), dtype=torch.float32, device=head.device)
        nbytes = L.hf_rcnn_loss_workspace()
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=head.device)
        args = [ptr(t) for t in (cls_logits, head, iou, gt_cls, non_empty) + tuple(enc)]
        check(L.hf_rcnn_loss_fwd(rows, k, nbx, nbt, *args, *thr, *w, ptr(out6), ptr(ws), nbytes, stream_ptr()), "rcnn_loss_fwd")
        ctx.save_for_backward(cls_logits, head, iou, gt_cls, non_empty, out6, *enc)
        ctx.meta = (rows, meta)
        return out6

    @staticmethod
    def backward(ctx, g):
        cls_logits, head, iou, gt_cls, non_empty, out6 = ctx.saved_tensors[:6]
        enc = ctx.saved_tensors[6:]
        rows, (k, nbx, nbt, thr, w) = ctx.meta
        up = g[5:6].contiguous()
        grad_cls, grad_head = torch.empty_like(cls_logits), torch.empty_like(head)
        args = [ptr(t) for t in (cls_logits, head, iou, gt_cls, non_empty) + tuple(enc)]
        check(_lib.lib().hf_rcnn_loss_bwd(rows, k, nbx, nbt, *args, *thr, *w, ptr(out6), ptr(up), ptr(grad_cls), ptr(grad_head),
                                          stream_ptr()), "rcnn_loss_bwd")
        return grad_cls, grad_head, None, None, None, None, None


def rcnn_loss_fused(cfg: RcnnConfig, tcfg: RcnnTrainConfig, cls_logits, head, iou, gt_cls, non_empty, targets):
    """the same loss as rcnn_loss through the two HIP passes; -> (total, parts)"""
    n, k1 = cls_logits.shape
    k = k1 - 1
    require(tuple(head.shape) == (n, k, cfg.head_width), "head must be (N, K, D)")
    f = lambda t, name: dev_tensor(t.detach().reshape(n, -1).float(), torch.float32, name)
    i = lambda t, name: dev_tensor(t.detach().reshape(n, -1).to(torch.int32), torch.int32, name)
    enc = (i(targets["bin_x"], "bin_x"), f(targets["res_x"], "res_x"), i(targets["bin_z"], "bin_z"), f(targets["res_z"], "res_z"),
           i(targets["bin_theta"], "bin_theta"), f(targets["res_theta"], "res_theta"), f(targets["res_y"], "res_y"),
           f(targets["res_size"], "res_size"))
    thr = (float(tcfg.cls_neg_iou_range[1]), float(tcfg.cls_pos_iou_range[0]), float(tcfg.reg_pos_iou_range[0]))
    w = (float(tcfg.cls_loss_weight), float(tcfg.reg_loss_weight))
    out6 = _RcnnLossFused.apply(dev_tensor(cls_logits, torch.float32, "cls_logits"), dev_tensor(head, torch.float32, "head"),
                                f(iou, "iou").reshape(n), i(gt_cls, "gt_cls").reshape(n), i(non_empty, "non_empty").reshape(n), enc,
                                (k, cfg.num_bin_xz, cfg.num_bin_theta, thr, w))
    d = out6.detach()
    return out6[5], {"box_classification": d[0], "bin_classification": d[1], "regression": d[2], "num_cls": d[3], "num_reg": d[4]}


# ------------------------------------------------------------------------------------------------ the train step
class RcnnTrainer(nn.Module):
    """RcnnModel + the target layer + the loss.  The sampler's RNG state is a persistent buffer [seed, call number]: it is saved
    with the weights, and graph_step.TrainStep's warm-up snapshot / restore covers it, so eager and replayed steps draw the same
    RoIs."""

    def __init__(self, model: RcnnModel = None, train_cfg: RcnnTrainConfig = None, seed: int = 0):
        super().__init__()
        self.model = model if model is not None else RcnnModel()
        self.tcfg = train_cfg or RcnnTrainConfig()
        self.register_buffer("rng_state", torch.tensor([int(seed), 0], dtype=torch.int64))

    def forward(self, xyz, rpn_fts, intensity, fg_mask, proposals, proposal_count, gt, gt_count, img_fts, calib, fused=True):
        cfg = self.model.cfg
        with torch.no_grad():
            rois, iou, gt_of_rois, stats = proposal_targets(proposals, proposal_count, gt, gt_count, self.rng_state, self.tcfg)
        cls_logits, reg, pool = self.model(xyz, rpn_fts, intensity, fg_mask, rois, img_fts, calib)
        flat_rois, flat_gt = rois.reshape(-1, 7), gt_of_rois.reshape(-1, 8)
        with torch.no_grad():
            targets = rcnn_encode(cfg, flat_rois, flat_gt)
        loss_fn = rcnn_loss_fused if fused else rcnn_loss
        loss, parts = loss_fn(cfg, self.tcfg, cls_logits, reg, iou.reshape(-1), flat_gt[:, 7].to(torch.int32), pool["non_empty"],
                              targets)
        parts.update({"rois": rois, "iou_of_rois": iou, "gt_of_rois": gt_of_rois, "stats": stats})
        return loss, parts


def rcnn_train_loss_parts(model, inputs, geometry):
    """an RcnnTrainer's (loss, parts) from a step's inputs: xyz, rpn_fts, intensity, fg_mask, proposals, proposal_count, gt,
    gt_count, img_fts, calib (geometry is unused: the RoI crops are recomputed every step)"""
    return model(inputs["xyz"], inputs["rpn_fts"], inputs["intensity"], inputs["fg_mask"], inputs["proposals"],
                 inputs["proposal_count"], inputs["gt"], inputs["gt_count"], inputs["img_fts"], inputs["calib"])


def rcnn_train_loss(model, inputs, geometry):
    """loss_fn of graph_step.TrainStep for an RcnnTrainer: rcnn_train_loss_parts without the parts"""
    return rcnn_train_loss_parts(model, inputs, geometry)[0]


# ------------------------------------------------------------------------------------------------ with the image branch
class RcnnWithImageBranch(nn.Module):
    """The rcnn_multiclass step with its own VGG pyramid (rcnn_multiclass.config img_feature_extractor; inference.ImgVggPyr, a
    stock convolutional network on the vendor library), the twin of rpn.RpnWithImageBranch: `img_fts` of forward() and detect()
    is then the IMAGE (B,H,W,3); everything else is RcnnModel's interface, and `cfg` is exposed, so RcnnTrainer drives it."""

    def __init__(self, rcnn: RcnnModel, img_net: nn.Module):
        super().__init__()
        self.rcnn, self.img_net = rcnn, img_net
        self.cfg = rcnn.cfg

    def forward(self, xyz, rpn_fts, intensity, fg_mask, proposals, img_fts, calib):
        return self.rcnn(xyz, rpn_fts, intensity, fg_mask, proposals, self.img_net(img_fts), calib)

    @torch.no_grad()
    def detect(self, xyz, rpn_fts, intensity, fg_mask, proposals, img_fts, calib):
        return self.rcnn.detect(xyz, rpn_fts, intensity, fg_mask, proposals, self.img_net(img_fts), calib)
