"""GPU tests (-m gpu) of the RCNN training pieces: the device proposal-target layer (csrc/rcnn_targets.hip) against
modules.box3d_iou and a NumPy restatement of kitti_dataset.py:545-680 (selection rules), the jitter of :690-770, the fused
RCNN loss against the op-by-op torch form, and the RCNN train step at the config's own sizes, eager and replayed.
The random streams differ from NumPy's: parity is in the rules, the IoU arithmetic and the loss graph."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_cases as sc  # noqa: E402
from heterofusionrcnn_amd import kitti_io, modules
from heterofusionrcnn_amd import rcnn_train as RT
from heterofusionrcnn_amd.rcnn import RcnnConfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = {"Car": 1, "Pedestrian": 2, "Cyclist": 3}
pytestmark = pytest.mark.gpu


def _kitti_gt():
    """KITTI-like GT sets: the Car / Pedestrian / Cyclist boxes of tests/golden/kitti/label_2 (1-2 per file), pooled, and the pool
    repeated at lateral offsets so that a frame holds a crowd of objects as KITTI frames do -> 4 (g, 8) float32 arrays"""
    pool = []
    for name in sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "kitti", "label_2"))):
        types, b3, _, _ = kitti_io.read_labels(os.path.join(ROOT, "tests", "golden", "kitti", "label_2", name), set(CLASSES))
        cls = np.array([CLASSES[t] for t in types], np.float64).reshape(-1, 1)
        pool.append(np.concatenate([b3, cls], 1))
    pool = np.concatenate(pool, 0)
    assert len(pool) >= 4
    out = []
    for f, shifts in enumerate(((-12, 0, 12), (-6, 6), (-18, -9, 0, 9, 18), (0,))):
        rows = [pool + np.array([dx, 0, 2.0 * f, 0, 0, 0, 0, 0]) for dx in shifts]
        out.append(np.concatenate(rows, 0).astype(np.float32))
    return out


def _proposals(rng, gt, m, near=0.5):
    """m proposals: a share jittered from the GTs (fg / hard bg), the rest random boxes of the KITTI extents (mostly easy bg)"""
    g = len(gt)
    k = int(m * near) if g else 0
    src = gt[rng.integers(0, g, k), :7] if g else np.zeros((0, 7), np.float32)
    jit = src + np.concatenate([rng.normal(0, 0.3, (k, 3)), np.zeros((k, 3)), rng.normal(0, 0.2, (k, 1))], 1)
    jit[:, 3:6] = src[:, 3:6] * rng.uniform(0.75, 1.25, (k, 3))
    far = np.concatenate([rng.uniform(-30, 30, (m - k, 1)), rng.uniform(1.0, 2.0, (m - k, 1)), rng.uniform(5, 70, (m - k, 1)),
                          rng.uniform(0.5, 4.5, (m - k, 1)), rng.uniform(0.5, 2.0, (m - k, 1)), rng.uniform(1.2, 2.0, (m - k, 1)),
                          rng.uniform(-np.pi, np.pi, (m - k, 1))], 1)
    p = np.concatenate([jit, far], 0).astype(np.float32)
    return p[rng.permutation(m)]


def _pack(props, gts, m=512, g=128):
    b = len(props)
    P = np.zeros((b, m, 7), np.float32)
    G = np.zeros((b, g, 8), np.float32)
    pc, gc = np.zeros(b, np.int32), np.zeros(b, np.int32)
    for f in range(b):
        P[f, :len(props[f])], pc[f] = props[f], len(props[f])
        G[f, :len(gts[f])], gc[f] = gts[f], len(gts[f])
    # padding rows hold boxes that would overlap everything: they must never be read
    P[:, :, 3:6][P[:, :, 3] == 0] = 5.0
    return [torch.from_numpy(a).cuda() for a in (P, pc, G, gc)]


def _iou_np(props, gt):
    """modules.box3d_iou on the device, read back (n, g) float32"""
    if len(props) == 0 or len(gt) == 0:
        return np.zeros((len(props), len(gt)), np.float32)
    return modules.box3d_iou(torch.from_numpy(props).cuda(), torch.from_numpy(gt[:, :7]).cuda())[0].cpu().numpy()


def _rules(iou, tc):
    """kitti_dataset.py:555-575 restated: max / argmax, the fg list (ascending, then the per-GT argmax RoIs), easy / hard bg"""
    n, g = iou.shape
    if g:
        mx, ga = iou.max(1), iou.argmax(1)
        mg, ra = iou.max(0), iou.argmax(0)
        ra = ra[mg > 0]
    else:
        mx, ga, ra = np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(0, np.int64)
    f32 = np.float32
    fg = np.concatenate([np.nonzero(mx >= f32(tc.fg_thresh))[0], ra])
    easy = np.nonzero(mx < f32(tc.cls_neg_iou_range[0]))[0]
    hard = np.nonzero((mx < f32(tc.cls_neg_iou_range[1])) & (mx >= f32(tc.cls_neg_iou_range[0])))[0]
    return mx, ga, fg, easy, hard


def _state(seed=5):
    return torch.tensor([seed, 0], dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ 1. IoU / val mode
def test_val_mode_equals_box3d_iou_max_argmax():
    rng = np.random.default_rng(0)
    gts = _kitti_gt()
    props = [_proposals(rng, g, n) for g, n in zip(gts, (512, 300, 511, 64))]
    P, pc, G, gc = _pack(props, gts)
    rois, iou, gt_of, stats = RT.proposal_targets(P, pc, G, gc, train=False)
    assert rois.shape == (4, 512, 7) and iou.shape == (4, 512) and gt_of.shape == (4, 512, 8)
    rois, iou, gt_of = rois.cpu().numpy(), iou.cpu().numpy(), gt_of.cpu().numpy()
    for f in range(4):
        n, g = len(props[f]), len(gts[f])
        want = _iou_np(props[f], gts[f])
        assert np.array_equal(rois[f, :n], props[f])
        np.testing.assert_allclose(iou[f, :n], want.max(1), rtol=0, atol=1e-6)
        assert np.array_equal(gt_of[f, :n], gts[f][want.argmax(1)])
        assert not rois[f, n:].any() and not iou[f, n:].any() and not gt_of[f, n:].any()
        assert g > 0 and (want.max(1) > 0.55).any() and (want.max(1) == 0).any()      # the scene holds fg and easy bg


# ------------------------------------------------------------------------------------------------ 2. sampling rules
def _check_sampling(props, gts, P, pc, G, gc, tc, seed=1):
    state = _state(seed)
    rois, iou, gt_of, stats = RT.proposal_targets(P, pc, G, gc, state, tc, aug_method=0)
    assert int(state[1]) == 1 and int(state[0]) == seed
    rois, iou, gt_of, stats = (t.cpu().numpy() for t in (rois, iou, gt_of, stats))
    r = tc.roi_per_sample
    branches = []
    for f in range(len(props)):
        n, g = len(props[f]), len(gts[f])
        if n == 0:
            assert not rois[f].any() and not iou[f].any() and not gt_of[f].any() and list(stats[f]) == [0, 0, 0, 0]
            branches.append("empty")
            continue
        iou_m = _iou_np(props[f], gts[f])
        mx, ga, fg, easy, hard = _rules(iou_m, tc)
        index = {tuple(p): i for i, p in enumerate(props[f])}
        idx = np.array([index[tuple(row)] for row in rois[f]])            # every output row is one of the frame's proposals
        nfg, nbg = len(fg), len(easy) + len(hard)
        if nfg > 0 and nbg > 0:
            fs = min(int(np.round(tc.fg_ratio * r)), nfg)
            want = [nfg, nbg, fs, r - fs]
            branches.append("fg+bg")
        elif nfg > 0:
            want, fs = [nfg, 0, r, 0], r
            branches.append("fg")
        elif nbg > 0:
            want, fs = [0, nbg, 0, r], 0
            branches.append("bg")
        else:
            want, fs = [0, 0, 0, 0], 0
            branches.append("neither")
        assert list(stats[f]) == want, (f, list(stats[f]), want)
        fg_set = list(fg)
        for s in range(fs):                                              # fg slots: fg entries, without replacement in fg+bg
            assert idx[s] in fg_set
            if branches[-1] == "fg+bg":
                fg_set.remove(idx[s])
        bgs = r - fs if want[3] else 0
        if bgs:
            hs = int(bgs * tc.hard_bg_ratio) if (len(hard) and len(easy)) else (bgs if len(hard) else 0)
            assert set(idx[fs:fs + hs]) <= set(hard) and set(idx[fs + hs:r]) <= set(easy)
            band = mx[idx[fs:r]]
            assert (band < np.float32(tc.cls_neg_iou_range[1])).all()
        for s in range(r):
            i = idx[s]
            assert np.array_equal(gt_of[f, s], gts[f][ga[i]] if g else np.zeros(8, np.float32))
            assert abs(iou[f, s] - mx[i]) <= 1e-6
        if g:
            again = _iou_np(rois[f], gts[f])[np.arange(r), ga[idx]]
            np.testing.assert_allclose(iou[f], again, rtol=0, atol=1e-6)
        else:
            assert not iou[f].any()
    return branches, stats


def test_sampling_rules_every_branch():
    tc = RT.RcnnTrainConfig()
    rng = np.random.default_rng(1)
    gts = _kitti_gt()
    far_gt = gts[0].copy()
    far_gt[:, 0] += 500.0                                               # no proposal touches it: IoU 0 everywhere
    fg_only_gt = gts[1][:3]
    nf = 40 * len(fg_only_gt)
    fg_only = np.repeat(fg_only_gt[:, :7], 40, 0) + np.concatenate([rng.uniform(-0.05, 0.05, (nf, 3)), np.zeros((nf, 4))], 1)
    props = [_proposals(rng, gts[0], 512),              # fg + bg, plentiful: 32 fg, 25 hard + 7 easy
             fg_only.astype(np.float32),                # fg only
             _proposals(rng, far_gt, 200, near=0.0),    # bg only (easy)
             _proposals(rng, gts[2], 100, near=0.0),    # no GT
             np.zeros((0, 7), np.float32),              # no proposal
             _proposals(rng, gts[3], 77)]               # padded counts
    frame_gts = [gts[0], fg_only_gt, far_gt, np.zeros((0, 8), np.float32), gts[1], gts[3]]
    P, pc, G, gc = _pack(props, frame_gts)
    branches, stats = _check_sampling(props, frame_gts, P, pc, G, gc, tc)
    assert branches == ["fg+bg", "fg", "bg", "bg", "empty", branches[5]]
    assert list(stats[0][2:]) == [32, 32]
    # neither fg nor bg: with cls_neg_iou_range (0, 0) an IoU of 0 is neither easy (< 0) nor hard, and no GT overlaps a RoI
    tn = RT.RcnnTrainConfig(cls_neg_iou_range=(0.0, 0.0))
    P2, pc2, G2, gc2 = _pack([props[2]], [far_gt])
    branches, stats = _check_sampling([props[2]], [far_gt], P2, pc2, G2, gc2, tn)
    assert branches == ["neither"]


def test_sampling_counts_hard_and_easy_when_plentiful():
    tc = RT.RcnnTrainConfig()
    rng = np.random.default_rng(2)
    gts = _kitti_gt()
    props = [_proposals(rng, g, 512, near=0.6) for g in gts]
    P, pc, G, gc = _pack(props, gts)
    rois, iou, gt_of, stats = RT.proposal_targets(P, pc, G, gc, _state(), tc, aug_method=0)
    st = stats.cpu().numpy()
    for f in range(4):
        mx, _, fg, easy, hard = _rules(_iou_np(props[f], gts[f]), tc)
        if len(fg) >= 32 and len(hard) and len(easy):
            assert list(st[f][2:]) == [32, 32]
            ious = iou[f].cpu().numpy()
            assert (ious[32:32 + 25] >= 0.05).all() and (ious[32:32 + 25] < 0.45).all() and (ious[57:] < 0.05).all()


# ------------------------------------------------------------------------------------------------ 3. jitter
# the float64 3D IoU (a Sutherland-Hodgman clip of the two rotated BEV rectangles) lives in tests/sampler_cases.py
_np_convex_iou = sc.ref_iou3d


def test_jitter_multiple():
    tc = RT.RcnnTrainConfig()
    rng = np.random.default_rng(3)
    gts = _kitti_gt()
    props = [_proposals(rng, g, 512, near=0.6) for g in gts]
    P, pc, G, gc = _pack(props, gts)
    s0 = _state(11)
    src, _, _, _ = RT.proposal_targets(P, pc, G, gc, s0.clone(), tc, aug_method=0)     # the same draws pick the same RoIs
    s1 = s0.clone()
    rois, iou, gt_of, stats = RT.proposal_targets(P, pc, G, gc, s1, tc)
    rois2, iou2, gt2, _ = RT.proposal_targets(P, pc, G, gc, s0.clone(), tc)
    assert torch.equal(rois, rois2) and torch.equal(iou, iou2) and torch.equal(gt_of, gt2)     # same state, same output
    assert int(s1[1]) == 1
    rois3, iou3, _, _ = RT.proposal_targets(P, pc, G, gc, s1, tc)                          # the state advanced: new draws
    assert int(s1[1]) == 2 and not torch.equal(rois3, rois)
    b, r = rois.shape[:2]
    flat, gflat = rois.reshape(-1, 7), gt_of.reshape(-1, 8)
    want = modules.box3d_iou(flat, gflat[:, :7].contiguous())[0].diagonal()
    np.testing.assert_allclose(iou.reshape(-1).cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-5)
    fr, gr, ir = flat.cpu().numpy().astype(np.float64), gflat.cpu().numpy().astype(np.float64), iou.reshape(-1).cpu().numpy()
    for i in range(0, b * r, 3):
        assert abs(_np_convex_iou(fr[i], gr[i]) - ir[i]) < 1e-4, i
    # shifts, scales, rotations inside the largest 'multiple' row: pos 1.0, hwl 0.15, angle pi / 3
    s = src.reshape(-1, 7).cpu().numpy().astype(np.float64)
    assert (np.abs(fr[:, 0:3] - s[:, 0:3]) <= 1.0 + 1e-5).all()
    ratio = fr[:, 3:6] / s[:, 3:6]
    assert (ratio >= 0.85 - 1e-5).all() and (ratio <= 1.15 + 1e-5).all()
    assert (np.abs(fr[:, 6] - s[:, 6]) <= np.pi / 3 + 1e-5).all()
    moved = np.abs(fr - s).max(1) > 0
    assert 0.3 < moved.mean() < 1.0
    # fg slots below fg_thresh after up to 10 tries (mostly per-GT argmax RoIs that start far below it): measured 6 of 128 = 4.7 %
    # on this scene and seed
    st = stats.cpu().numpy()
    ious = iou.cpu().numpy()
    fg_low = [ious[f, :st[f, 2]] < np.float32(tc.fg_thresh) for f in range(b)]
    frac = np.concatenate(fg_low).mean()
    print("fg slots below fg_thresh after jitter: %.4f of %d" % (frac, sum(len(x) for x in fg_low)))
    assert frac <= 0.10, frac


# ------------------------------------------------------------------------------------------------ 4. fused loss
@pytest.mark.parametrize("kind", ["mixed", "empty_masks", "class0"])
def test_fused_loss_matches_torch_form(kind):
    cfg, tc = RcnnConfig(), RT.RcnnTrainConfig()
    rng = np.random.default_rng({"mixed": 0, "empty_masks": 1, "class0": 2}[kind])
    n, k, d = 300, cfg.num_classes, cfg.head_width
    iou = torch.from_numpy(rng.uniform(0, 1, n).astype(np.float32)).cuda()
    gt_cls = torch.from_numpy(rng.integers(1, 4, n).astype(np.int32)).cuda()
    ne = torch.from_numpy(rng.random(n) < 0.8).cuda()
    if kind == "empty_masks":
        ne[:] = False
    if kind == "class0":
        gt_cls[::3] = 0                                                  # class-0 rows inside the reg mask index class 0, never -1
        iou[::3] = torch.from_numpy(rng.uniform(0.56, 1.0, len(range(0, n, 3))).astype(np.float32)).cuda()
    t = {"bin_x": torch.randint(0, cfg.num_bin_xz, (n, k), dtype=torch.int32, device="cuda"),
         "res_x": torch.rand(n, k, device="cuda") * 2 - 1,
         "bin_z": torch.randint(0, cfg.num_bin_xz, (n, k), dtype=torch.int32, device="cuda"),
         "res_z": torch.rand(n, k, device="cuda") * 2 - 1,
         "bin_theta": torch.randint(0, cfg.num_bin_theta, (n,), dtype=torch.int32, device="cuda"),
         "res_theta": torch.rand(n, device="cuda") * 2 - 1, "res_y": torch.randn(n, device="cuda"),
         "res_size": torch.randn(n, 3, device="cuda")}
    logits = (torch.randn(n, k + 1, device="cuda") * 2).requires_grad_(True)
    head = (torch.randn(n, k, d, device="cuda") * 1.5).requires_grad_(True)
    ref, rp = RT.rcnn_loss(cfg, tc, logits, head, iou, gt_cls, ne, t)
    g_ref = torch.autograd.grad(ref * 1.7, [logits, head])
    got, gp = RT.rcnn_loss_fused(cfg, tc, logits, head, iou, gt_cls, ne, t)
    g_got = torch.autograd.grad(got * 1.7, [logits, head])
    for key in ("box_classification", "bin_classification", "regression", "num_cls", "num_reg"):
        np.testing.assert_allclose(float(gp[key]), float(rp[key]), rtol=1e-5, atol=1e-6, err_msg=key)
    np.testing.assert_allclose(float(got.detach()), float(ref.detach()), rtol=1e-5, atol=1e-6)
    for a, b_ in zip(g_got, g_ref):
        np.testing.assert_allclose(a.cpu().numpy(), b_.cpu().numpy(), rtol=1e-5, atol=1e-5)
    if kind == "empty_masks":
        assert float(gp["num_cls"]) == 0 and float(gp["num_reg"]) == 0 and float(got.detach()) == 0.0
        assert not g_got[0].any() and not g_got[1].any()
    else:
        assert float(gp["num_cls"]) > 0 and float(gp["num_reg"]) > 0


# ------------------------------------------------------------------------------------------------ 5. the train step
def rcnn_scene(b, seed, m=512):
    """frames at the config's sizes: 16384 points with 288-channel RPN features, a 360 x 1200 x 32 image feature map, GT boxes
    sitting on cloud points, 512 proposals around them"""
    import bench
    rng = np.random.default_rng(seed)
    xyz = bench.kitti_frustum(rng, b, bench.N0)
    gts, props = [], []
    for f in range(b):
        g = 12
        centre = xyz[f, rng.choice(bench.N0, g, replace=False)]
        cls = rng.integers(1, 4, g)
        size = np.asarray(RcnnConfig().cluster_sizes, np.float32)[cls - 1]
        box = np.concatenate([centre[:, 0:1], centre[:, 1:2] + size[:, 2:3] / 2, centre[:, 2:3], size,
                              rng.uniform(-np.pi, np.pi, (g, 1))], 1)
        gts.append(np.concatenate([box, cls[:, None]], 1).astype(np.float32))
        props.append(_proposals(rng, gts[-1], m, near=0.6))
    P, pc, G, gc = _pack(props, gts, m=m, g=64)
    inputs = {
        "xyz": torch.from_numpy(xyz).cuda(),
        "rpn_fts": torch.randn(b, bench.N0, 288, device="cuda"),
        "intensity": torch.rand(b, bench.N0, 1, device="cuda") - 0.5,
        "fg_mask": torch.rand(b, bench.N0, device="cuda") < 0.3,
        "proposals": P, "proposal_count": pc, "gt": G, "gt_count": gc,
        "img_fts": torch.randn(b, bench.IMG_H, bench.IMG_W, bench.IMG_C, device="cuda").requires_grad_(True),
        "calib": torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous(),
    }
    return inputs


def _trainers(seed):
    """two identical trainers (path drop off): the second gets the first's parameters and buffers, the dropout states and the
    sampler's RNG state included"""
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    from heterofusionrcnn_amd.rcnn import RcnnModel
    out = []
    for _ in range(2):
        torch.manual_seed(seed)
        out.append(RT.RcnnTrainer(RcnnModel(RcnnConfig(path_drop=(1.0, 1.0))), seed=seed).cuda().train())
    with torch.no_grad():
        for a, b_ in zip(list(out[0].parameters()) + list(out[0].buffers()), list(out[1].parameters()) + list(out[1].buffers())):
            b_.copy_(a)
    return [(tr, MultiTensorAdam(tr.parameters(), lr=1e-3)) for tr in out]


def test_train_step_eager_and_replayed_agree_and_learn():
    from heterofusionrcnn_amd.graph_step import TrainStep
    inputs = rcnn_scene(2, 7)
    losses = {}
    params = {}
    pairs = _trainers(3)
    for graph in (False, True):
        tr, opt = pairs[int(graph)]
        step = TrainStep(tr, opt, inputs, None, graph=graph, loss_fn=RT.rcnn_train_loss)
        losses[graph] = [float(step()) for _ in range(3)]
        torch.cuda.synchronize()
        params[graph] = [p.detach().clone() for p in tr.parameters()]
        if graph:
            img_grad = inputs["img_fts"].grad
            assert img_grad is not None and torch.isfinite(img_grad).all() and img_grad.abs().sum() > 0
            for _ in range(57):
                losses[graph].append(float(step()))
    diff = max(float((a - b_).abs().max()) for a, b_ in zip(params[True], params[False]))
    seq = np.asarray(losses[True])
    first, last = seq[:10].mean(), seq[-10:].mean()
    print("eager losses %s, replayed %s; max parameter difference after 3 steps %.3g" % (losses[False], losses[True][:3], diff))
    print("rcnn train loss: first 10 %.4f, last 10 %.4f" % (first, last))
    # the crop / image gradients sum with atomics: the two runs agree to rounding, not bit for bit.  Measured: losses equal to
    # 1e-7 relative.  Adam moves every element by up to ~lr per step whatever the gradient's size, so an element whose gradient is
    # rounding noise can end up to 2 x 3 steps x lr apart (measured max 2.7e-3); nearly all elements agree far more closely.
    np.testing.assert_allclose(losses[True][:3], losses[False], rtol=1e-4, atol=1e-6)
    flat_d = torch.cat([(a - b_).abs().reshape(-1) for a, b_ in zip(params[True], params[False])])
    frac_off = float((flat_d > 1e-4).float().mean())
    print("share of parameter elements more than 1e-4 apart: %.2e" % frac_off)
    assert float(flat_d.max()) <= 2 * 3 * 1e-3 + 1e-6
    assert frac_off < 1e-2
    # measured on this scene: mean of the first 10 losses 9.72, of the last 10 3.94
    assert np.isfinite(seq).all()
    assert last < 0.6 * first, (first, last)
