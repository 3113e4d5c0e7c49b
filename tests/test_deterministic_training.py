"""Bit-reproducible training (GPU): heterofusionrcnn_amd.deterministic through the Python layer.

  * every route whose floating-point sum has no fixed order raises a RuntimeError that names the op under the mode -- the atomic
    image-feature gradients of project_gather and image_crop_and_resize among them -- and runs as before outside it; with their
    inverse index the gather-form gradients run under the mode.
  * RpnModel without the image branch: forward + backward twice from one state, every gradient has equal bits; the same model with
    the fusion branch and RcnnModel with its image RoIs stop at the image gradient.
  * file-fed runs in fresh processes (the runner of tests/test_train_resume.py, batch 2, the reference train op) for
    rpn_multiclass_points: 4 steps with a checkpoint at 2, the same run again, and a resume from step 2 -- the losses and every saved
    tensor have EQUAL BITS across the three.  This is the only test here that takes more than a few seconds.
Reproducible up to the image branch: rpn_multiclass and train_rcnn do not run under the mode, because the gradient of the image
feature map (hf::project_gather_grad_kernel, hf::crop_and_resize_grad_kernel) is summed by fp32 atomics (DESIGN.md section 8,
"Reproducible training")."""
import copy
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_train_resume as TR  # noqa: E402
from test_train_resume import dataset  # noqa: E402,F401  (fixture)

import heterofusionrcnn_amd as hf  # noqa: E402
from heterofusionrcnn_amd import fusion  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(t):
    return t.detach().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- the refusals
def test_every_unordered_route_raises_under_the_mode():
    from heterofusionrcnn_amd import cropping, grouping, interpolate, pointcnn
    g = torch.Generator().manual_seed(0)
    pts = torch.randn(2, 64, 8, generator=g).cuda().requires_grad_(True)
    idx = torch.randint(0, 64, (2, 16, 4), generator=g).int().cuda()
    head = torch.randn(2, 16, 4, 3, generator=g).cuda()
    idx3 = torch.randint(0, 64, (2, 32, 3), generator=g).int().cuda()
    w3 = torch.rand(2, 32, 3, generator=g).cuda()
    k, c0, c1 = 8, 64, 8
    x = torch.randn(2, 16, k, k, generator=g).cuda().requires_grad_(True)
    f_delta = torch.randn(2, 16, k, c0, generator=g).cuda().requires_grad_(True)
    nbr = torch.randint(0, 64, (2, 16, k), generator=g).int().cuda()
    wd = torch.randn(k, c0 + c1, 1, generator=g).cuda().requires_grad_(True)
    img = torch.randn(2, 9, 11, 4, generator=g).cuda().requires_grad_(True)
    boxes = torch.tensor([[0.1, 0.1, 0.9, 0.9]]).cuda()
    ind = torch.zeros(1, dtype=torch.int32).cuda()
    xyz = torch.rand(2, 50, 3, generator=g).cuda() + 1.0
    calib = torch.tensor([[5.5, 0, 5.5, 0], [0, 4.5, 4.5, 0], [0, 0, 1, 0]]).cuda().repeat(2, 1, 1)
    with hf.deterministic(True):
        with pytest.raises(RuntimeError, match="project_gather"):
            fusion.project_gather(xyz, calib, img)
        with pytest.raises(RuntimeError, match="image_crop_and_resize"):
            fusion.image_crop_and_resize(img, boxes, ind, 3)
        with pytest.raises(RuntimeError, match="image_crop_and_resize"):                      # the tensor form on the device
            fusion.image_crop_and_resize(img.double(), boxes.double(), ind, 3)
        with pytest.raises(RuntimeError, match="project_boxes_to_image"):
            fusion.project_boxes_to_image(torch.rand(1, 2, 7).cuda().requires_grad_(True), torch.rand(1, 3, 4).cuda(), (9, 11))
        with pytest.raises(RuntimeError, match="gather_rows_grad"):
            grouping.group_point(pts, idx).sum().backward()
        with pytest.raises(RuntimeError, match="gather_rows_grad"):
            grouping.concat_group(head, pts, idx).sum().backward()
        with pytest.raises(RuntimeError, match="three_interpolate"):
            interpolate.three_interpolate(pts, idx3, w3)
        with pytest.raises(RuntimeError, match="xconv_depthwise_gather"):
            pointcnn.xconv_depthwise_gather(x, f_delta, pts.detach(), nbr, wd, use_workspace=False)
        with pytest.raises(RuntimeError, match="three_interpolate_channel_first_grad"):
            interpolate.three_interpolate_channel_first_grad((2, 8, 64), idx3, w3, torch.zeros(2, 8, 32).cuda())
        with pytest.raises(RuntimeError, match="pc_crop_and_sample_grad_fts"):
            cropping.pc_crop_and_sample_grad_fts(pts.detach(), torch.zeros(3, dtype=torch.int32).cuda(),
                                                 torch.zeros(3, 5, dtype=torch.int32).cuda(), torch.zeros(3, 5, 8).cuda())
        # what needs no gradient of the image, and the gather forms with their inverse index, run under the mode
        with torch.no_grad():
            fusion.project_gather(xyz, calib, img)
            interpolate.three_interpolate(pts, idx3, w3)
        interpolate.three_interpolate(pts.detach(), idx3, w3)
        pointcnn.xconv_depthwise_gather(x.detach(), f_delta.detach(), pts.detach(), nbr, wd.detach(), use_workspace=False)
        recorded_inside = grouping.group_point(pts, idx)
        fusion.project_gather(xyz, calib, img.detach())
        fusion.image_crop_and_resize(img.detach(), boxes, ind, 3)
        a = grouping.concat_group(head, pts, idx, inverse=grouping.index_inverse(idx, 64))
        b = interpolate.three_interpolate(pts, idx3, w3, inverse=interpolate.three_nn_inverse(idx3, 64))
        pts.grad = None
        (a.sum() + b.sum()).backward()
        first = pts.grad.clone()
        pts.grad = None
        a = grouping.concat_group(head, pts, idx, inverse=grouping.index_inverse(idx, 64))
        b = interpolate.three_interpolate(pts, idx3, w3, inverse=interpolate.three_nn_inverse(idx3, 64))
        (a.sum() + b.sum()).backward()
        assert torch.equal(bits(first), bits(pts.grad))
    # one rule: the mode is the one the op's forward recorded, wherever its backward runs
    with pytest.raises(RuntimeError, match="gather_rows_grad"):
        recorded_inside.sum().backward()
    recorded_outside = grouping.group_point(pts, idx)
    with hf.deterministic(True):
        recorded_outside.sum().backward()
    # outside the mode every route is what it was
    fusion.project_gather(xyz, calib, img).sum().backward()
    fusion.image_crop_and_resize(img, boxes, ind, 3).sum().backward()
    grouping.group_point(pts, idx).sum().backward()
    interpolate.three_interpolate(pts, idx3, w3).sum().backward()
    assert float(img.grad.abs().sum()) > 0


def test_fused_xconv_weight_gradient_takes_the_workspace_under_the_mode():
    """hf_xconv_depthwise_grad adds the row chunks' weight gradients with atomics; under the mode hf_xconv_depthwise_grad_ws writes them
    to a workspace and adds them in a fixed order: three calls give the same bits, the other two gradients are the bits of the atomic
    entry point, and the weight gradient agrees with it to rounding (1400 rows = 44 row chunks; k c m = 8 x 40 x 2)"""
    from heterofusionrcnn_amd import pointcnn
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 700, 8, 8, generator=g).cuda().requires_grad_(True)
    f = torch.randn(2, 700, 8, 40, generator=g).cuda().requires_grad_(True)
    wd = torch.randn(8, 40, 2, generator=g).cuda().requires_grad_(True)
    go = torch.randn(2, 700, 80, generator=g).cuda()

    def grads():
        return torch.autograd.grad((pointcnn.xconv_depthwise(x, f, wd) * go).sum(), (x, f, wd))

    plain = grads()
    with hf.deterministic(True):
        first = grads()
        for _ in range(2):
            again = grads()
            assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, again)), "two calls differ"
    assert torch.equal(bits(first[0]), bits(plain[0])) and torch.equal(bits(first[1]), bits(plain[1]))
    # against fp64 with the bounds of tests/test_xconv_grad_ws_abi.py: (depth + k + 2) u sum_r (|x| |f|) |go| with depth = 32 + 44 for
    # the workspace form (chunks of 32 rows, then 44 chunk sums in order) and 1400 for the atomic form (any order): 0.03 and 0.5 where
    # the elements are of size 100 and one dropped row chunk would move them by 16
    xd, fd, gd = x.detach().double().reshape(1400, 8, 8), f.detach().double().reshape(1400, 8, 40), go.double().reshape(1400, 40, 2)
    want = torch.einsum("rwc,rcm->wcm", xd @ fd, gd)
    mag = 2.0 ** -24 * torch.einsum("rwc,rcm->wcm", xd.abs() @ fd.abs(), gd.abs())
    assert float(((32 + 44 + 8 + 2) * mag).max()) < 0.05
    assert bool(((first[2].double() - want).abs() <= (32 + 44 + 8 + 2) * mag).all())
    assert bool(((plain[2].double() - want).abs() <= (1400 + 8 + 2) * mag).all())
    # the mode is the one the forward recorded: forward inside and backward outside takes the workspace form, and the reverse does not
    with hf.deterministic(True):
        out = pointcnn.xconv_depthwise(x, f, wd)
    outside = torch.autograd.grad((out * go).sum(), (x, f, wd))
    assert torch.equal(bits(outside[2]), bits(first[2]))


# ------------------------------------------------------------------------------------------------------------ whole models
def _twice(model, run):
    """run() -> scalar; forward + backward twice from one state -> the two dicts of gradients"""
    from heterofusionrcnn_amd import checkpoint as C
    state, drops, rng = copy.deepcopy(model.state_dict()), C.drop_states(model), C.rng_states()
    grads = []
    for _ in range(2):
        model.load_state_dict(state)
        C.load_drop_states(model, drops)
        C.load_rng_states(rng)
        model.zero_grad(set_to_none=True)
        loss = run()
        loss.backward()
        g = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        g["(loss)"] = loss.detach().reshape(1).clone()
        grads.append(g)
    return grads


def test_rpn_model_on_points_repeats_every_gradient():
    from test_graph_step import _frames, _small_multiclass

    from heterofusionrcnn_amd import rpn as R_
    cfg = _small_multiclass(img_c=0, dropout=0.5)
    inp = _frames(cfg, 2, 2048, seed=0)
    torch.manual_seed(4)
    model = R_.RpnModel(cfg).cuda().train()

    def run():
        seg, head = model(inp["xyz"], inp["intensity"])
        return model.loss(inp["xyz"], seg, head, inp["label_cls"], inp["label_reg"])[0]

    with hf.deterministic(True):
        a, b = _twice(model, run)
    assert a.keys() == b.keys() and len(a) > 20
    differ = [n for n in a if not torch.equal(bits(a[n]), bits(b[n]))]
    assert not differ, "gradients whose bits differ between two runs from one state: %s" % differ


def test_models_with_the_image_branch_stop_at_the_image_gradient():
    from test_graph_step import _frames, _small_multiclass
    from test_roi_image import small_rcnn, small_scene

    from heterofusionrcnn_amd import rpn as R_
    cfg = _small_multiclass()
    inp = _frames(cfg, 2, 2048, seed=0)
    rpn = R_.RpnModel(cfg).cuda().train()
    _, rcnn = small_rcnn()
    s = small_scene(11)
    s["img_fts"].requires_grad_(True)
    args = (s["xyz"], s["rpn_fts"], s["intensity"], s["fg_mask"], s["proposals"], s["img_fts"], s["calib"])
    with hf.deterministic(True):
        with pytest.raises(RuntimeError, match="project_gather"):
            rpn(inp["xyz"], inp["intensity"], img_fts=inp["img_fts"], calib=inp["calib"])
        with pytest.raises(RuntimeError, match="image_crop_and_resize"):
            rcnn.train()(*args)
        with torch.no_grad():                                    # inference needs no image gradient
            rcnn.eval()(*args)
    rcnn.train()(*args)


# ------------------------------------------------------------------------------------------------------------ file-fed runs
def _saved_bits(path):
    sd = torch.load(path, map_location="cpu")
    return {k: v.contiguous().view(torch.uint8).numpy().tobytes() for k, v in sd.items() if isinstance(v, torch.Tensor)}


def test_rpn_points_runs_repeat_and_resume_bit_for_bit(dataset, tmp_path):  # noqa: F811
    """4 steps with a checkpoint at 2; the same again; a resume from step 2 in a fresh process: equal bits everywhere"""
    from heterofusionrcnn_amd import checkpoint as C
    tmp = str(tmp_path)
    common = dict(dataset_dir=dataset, split="train", batch=2, seed=1, log_every=0, workers=2, config="rpn_multiclass_points",
                  deterministic=True, **TR.TRAIN_OP)
    runs = {}
    for tag in ("full", "again"):
        runs[tag] = TR._run(tmp, "rpn", steps=4, checkpoint_dir=os.path.join(tmp, tag), checkpoint_every=2,
                            save=os.path.join(tmp, tag + ".pt"), **common)
    res_dir = os.path.join(tmp, "res")
    os.makedirs(res_dir)
    shutil.copy(C.checkpoint_path(os.path.join(tmp, "full"), 2), res_dir)
    runs["resumed"] = TR._run(tmp, "rpn", steps=4, checkpoint_dir=res_dir, resume=True, save=os.path.join(tmp, "resumed.pt"), **common)
    full, again, resumed = runs["full"], runs["again"], runs["resumed"]
    print("losses", full.tolist(), again.tolist(), resumed.tolist())
    assert len(full) == 4 and len(resumed) == 2 and np.isfinite(full).all()
    assert full.tobytes() == again.tobytes(), "the repeated run's losses differ"
    assert full[2:].tobytes() == resumed.tobytes(), "the resumed run's losses differ"
    p_full = _saved_bits(os.path.join(tmp, "full.pt"))
    assert len(p_full) > 20
    for tag in ("again", "resumed"):
        p = _saved_bits(os.path.join(tmp, tag + ".pt"))
        assert p.keys() == p_full.keys()
        differ = [k for k in p if p[k] != p_full[k]]
        assert not differ, "%s: saved tensors whose bits differ from the uninterrupted run: %s" % (tag, differ[:10])
