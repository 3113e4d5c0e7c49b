"""RCNN train step timing: ms per step eager and replayed (graph_step.TrainStep) at batch 2 and 8 x 64 RoIs (512 proposals per
frame, full widths), the device target layer's time (hf_rcnn_proposal_targets, 'multiple' jitter), and the same sampling +
jitter as a host NumPy loop (kitti_dataset.py:545-770 restated; a float64 convex-clip IoU stands in for the reference's
box_util.box3d_iou) for comparison.  Also the share of fg slots that stay below fg_thresh after the jitter.  One JSON line.

  python scripts/probes/rcnn_train_timing.py [--steps 20] [--batches 2,8]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from heterofusionrcnn_amd import rcnn_train as RT  # noqa: E402
from heterofusionrcnn_amd.graph_step import TrainStep  # noqa: E402
from heterofusionrcnn_amd.optim import MultiTensorAdam  # noqa: E402
from heterofusionrcnn_amd.rcnn import RcnnConfig, RcnnModel  # noqa: E402
from test_rcnn_train import _np_convex_iou, rcnn_scene  # noqa: E402


def _ms(fn, iters):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def step_times(batch, steps):
    out = {}
    inputs = rcnn_scene(batch, 7)
    for graph in (False, True):
        torch.manual_seed(0)
        tr = RT.RcnnTrainer(RcnnModel(RcnnConfig()), seed=0).cuda().train()
        step = TrainStep(tr, MultiTensorAdam(tr.parameters(), lr=1e-3), inputs, None, graph=graph, loss_fn=RT.rcnn_train_loss)
        for _ in range(3):
            step()
        out["replayed" if graph else "eager"] = _ms(step, steps)
        del step, tr
        torch.cuda.empty_cache()
    return out, inputs


def host_sampling(rng, iou, props, gt, tc):
    """sample_rois_for_rcnn_training + aug_roi_by_noise ('multiple') for one frame, NumPy"""
    mx, ga = iou.max(1), iou.argmax(1)
    mg, ra = iou.max(0), iou.argmax(0)
    fg = np.concatenate([np.nonzero(mx >= tc.fg_thresh)[0], ra[mg > 0]])
    easy = np.nonzero(mx < tc.cls_neg_iou_range[0])[0]
    hard = np.nonzero((mx < tc.cls_neg_iou_range[1]) & (mx >= tc.cls_neg_iou_range[0]))[0]
    nf = min(int(np.round(tc.fg_ratio * tc.roi_per_sample)), len(fg))
    fg = fg[rng.permutation(len(fg))[:nf]]
    nb = tc.roi_per_sample - nf
    nh = int(nb * tc.hard_bg_ratio)
    bg = np.concatenate([hard[np.floor(rng.random(nh) * len(hard)).astype(int)], easy[np.floor(rng.random(nb - nh) * len(easy)).astype(int)]])
    rows = [(i, 10) for i in fg] + [(i, 1) for i in bg]
    ranges = [[0.2, 0.1, np.pi / 12], [0.3, 0.15, np.pi / 12], [0.5, 0.15, np.pi / 9], [0.8, 0.15, np.pi / 6], [1.0, 0.15, np.pi / 3]]
    for i, tries in rows:
        box, g = props[i].astype(np.float64), gt[ga[i], :7].astype(np.float64)
        t, c = 0.0, 0
        while t < tc.fg_thresh and c < tries:
            if rng.random() < 0.2:
                aug = box
            else:
                r = ranges[rng.integers(5)]
                aug = np.concatenate([box[0:3] + (rng.random(3) - 0.5) / 0.5 * r[0], box[3:6] * ((rng.random(3) - 0.5) / 0.5 * r[1] + 1),
                                      box[6:7] + (rng.random(1) - 0.5) / 0.5 * r[2]])
            t = _np_convex_iou(aug, g)
            c += 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--batches", default="2,8")
    args = ap.parse_args()
    tc = RT.RcnnTrainConfig()
    res = {"what": "rcnn train step (RcnnTrainer: targets + RcnnModel + fused loss + MultiTensorAdam), 512 proposals / frame, 64 RoIs"}
    for b in [int(x) for x in args.batches.split(",")]:
        t, inputs = step_times(b, args.steps)
        res["step_ms_eager_b%d" % b] = round(t["eager"], 3)
        res["step_ms_replayed_b%d" % b] = round(t["replayed"], 3)
        state = torch.tensor([1, 0], dtype=torch.int64, device="cuda")
        call = lambda: RT.proposal_targets(inputs["proposals"], inputs["proposal_count"], inputs["gt"], inputs["gt_count"], state, tc)
        for _ in range(3):
            call()
        res["targets_ms_b%d" % b] = round(_ms(call, 50), 4)
        low, total = 0, 0
        for _ in range(20):
            _, iou, _, st = call()
            iou, st = iou.cpu().numpy(), st.cpu().numpy()
            for f in range(b):
                low += int((iou[f, :st[f, 2]] < np.float32(tc.fg_thresh)).sum())
                total += int(st[f, 2])
        res["fg_below_thresh_b%d" % b] = [low, total]
        if b == min(int(x) for x in args.batches.split(",")):
            from heterofusionrcnn_amd import modules
            rng = np.random.default_rng(0)
            frames = []
            for f in range(b):
                n, g = int(inputs["proposal_count"][f]), int(inputs["gt_count"][f])
                P, G = inputs["proposals"][f, :n], inputs["gt"][f, :g]
                frames.append((modules.box3d_iou(P, G[:, :7].contiguous())[0].cpu().numpy(), P.cpu().numpy(), G.cpu().numpy()))
            t0 = time.perf_counter()
            for iou_m, P, G in frames:
                host_sampling(rng, iou_m, P, G, tc)
            res["host_numpy_sampling_ms_b%d" % b] = round((time.perf_counter() - t0) * 1e3, 2)
        del inputs
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
