"""Bit-reproducible training with the image (GPU): heterofusionrcnn_amd.deterministic("image") through the Python layer.

  * under the level both image ops run with a gradient and their image gradient has the BITS of the sequential fp32 sum of
    tests/ordered_grad_cases.py; the choice is the one the forward recorded, wherever the backward runs; ordered_grad=True takes the
    ordered form outside the mode and under level True, ordered_grad=False (the atomics) is refused under both levels.
  * RpnModel with the fusion branch and RcnnModel with its image RoIs: forward + backward twice from one state, every gradient has
    equal bits, the image feature map's included.
  * file-fed runs in fresh processes (the runner of tests/test_train_resume.py, batch 2, the reference train op, the captured graph on)
    for train_rpn --config rpn_multiclass and train_rcnn: 4 steps with a checkpoint at 2, the same run again, and a resume from
    step 2 -- the losses and every saved tensor, the VGG pyramid's included, have EQUAL BITS across the three.  These two are the
    only tests here that take more than a few seconds."""
import os
import shutil
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ordered_grad_cases as oc  # noqa: E402
import roi_image_cases as rc  # noqa: E402
import test_train_resume as TR  # noqa: E402
from test_deterministic_training import _twice, bits  # noqa: E402
from test_train_resume import dataset, handoff  # noqa: E402,F401  (fixtures)

import heterofusionrcnn_amd as hf  # noqa: E402
from heterofusionrcnn_amd import fusion  # noqa: E402

pytestmark = pytest.mark.gpu

GRADS = ("hf_project_gather_grad", "hf_project_gather_grad_ordered", "hf_crop_and_resize_grad", "hf_crop_and_resize_grad_ordered")


class Calls:
    """counts the calls of the four image-gradient entry points while it is active"""

    def __init__(self, monkeypatch):
        from heterofusionrcnn_amd import _lib
        self.seen = dict.fromkeys(GRADS, 0)
        real = _lib.lib()

        class Counting:
            def __getattr__(proxy, name):
                if name in self.seen:
                    self.seen[name] += 1
                return getattr(real, name)

        monkeypatch.setattr(_lib, "_lib", Counting())

    def take(self):
        seen, self.seen = self.seen, dict.fromkeys(GRADS, 0)
        return {k: v for k, v in seen.items() if v}


def same_bits(got, want):
    return np.array_equal(got.detach().cpu().contiguous().numpy().view(np.int32), np.ascontiguousarray(want).view(np.int32))


# ------------------------------------------------------------------------------------------------------------------ the two ops
def _project_inputs():
    """points that a pinhole spreads over a 6 x 10 map, many to a pixel, some outside it"""
    rng = np.random.default_rng(7)
    b, p, h, w, c = 2, 400, 6, 10, 5
    xyz = np.stack([rng.uniform(-6, 6, (b, p)), rng.uniform(-4, 4, (b, p)), rng.uniform(2, 10, (b, p))], -1).astype(np.float32)
    calib = torch.tensor([[w / 2.0, 0, w / 2.0, 0], [0, h / 2.0, h / 2.0, 0], [0, 0, 1, 0]], device="cuda").repeat(b, 1, 1)
    img = torch.from_numpy(rng.standard_normal((b, h, w, c)).astype(np.float32)).cuda().requires_grad_(True)
    go = oc.order_sensitive_values(rng, (b, p, c))
    return torch.from_numpy(xyz).cuda(), calib, img, go


def _project_want(pix, go, shape):
    b, h, w, c = shape
    u, v = pix[..., 0].astype(np.int64), pix[..., 1].astype(np.int64)
    valid = (u >= 0) & (u < w) & (v >= 0) & (v < h)
    key = np.where(valid, (np.arange(b)[:, None] * h + v) * w + u, 0)
    k = oc.counts(b * h * w, valid.reshape(-1), key.reshape(-1))
    assert k.max() >= 3 and not valid.all()
    return oc.sequential(b * h * w, valid.reshape(-1), key.reshape(-1), go.reshape(-1, c)).reshape(shape)


def _crop_inputs(name="vec_c32"):
    d, t = rc.dims(name), rc.make_inputs(name)
    img = torch.from_numpy(t["img"].copy()).cuda().requires_grad_(True)
    return d, img, torch.from_numpy(t["boxes"].copy()).cuda(), torch.from_numpy(t["ind"].copy()).cuda(), torch.from_numpy(t["go"].copy()).cuda()


def test_both_ops_take_the_ordered_gradient_under_the_level(monkeypatch):
    calls = Calls(monkeypatch)
    xyz, calib, img, go = _project_inputs()
    with hf.deterministic("image"):
        out, pix = fusion.project_gather(xyz, calib, img, return_pixels=True)
        (g,) = torch.autograd.grad(out, img, torch.from_numpy(go).cuda())
    assert calls.take() == {"hf_project_gather_grad_ordered": 1}
    assert same_bits(g, _project_want(pix.cpu().numpy(), go, tuple(img.shape)))
    d, cimg, boxes, ind, cgo = _crop_inputs()
    with hf.deterministic("image"):
        (g,) = torch.autograd.grad(fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"]), cimg, cgo)
    assert calls.take() == {"hf_crop_and_resize_grad_ordered": 1}
    assert same_bits(g, oc.crop_reference("vec_c32")["grad"])


def test_the_choice_is_the_one_the_forward_recorded(monkeypatch):
    calls = Calls(monkeypatch)
    xyz, calib, img, go = _project_inputs()
    d, cimg, boxes, ind, cgo = _crop_inputs()
    go = torch.from_numpy(go).cuda()
    with hf.deterministic("image"):
        inside = (fusion.project_gather(xyz, calib, img), fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"]))
    outside = (fusion.project_gather(xyz, calib, img), fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"]))
    g_in = (torch.autograd.grad(inside[0], img, go)[0], torch.autograd.grad(inside[1], cimg, cgo)[0])
    assert calls.take() == {"hf_project_gather_grad_ordered": 1, "hf_crop_and_resize_grad_ordered": 1}
    with hf.deterministic("image"):
        torch.autograd.grad(outside[0], img, go), torch.autograd.grad(outside[1], cimg, cgo)
    assert calls.take() == {"hf_project_gather_grad": 1, "hf_crop_and_resize_grad": 1}
    assert same_bits(g_in[1], oc.crop_reference("vec_c32")["grad"])
    # the keyword: True takes the ordered form outside the mode and under level True, with the same bits
    for level in (False, True):
        with hf.deterministic(level):
            a = fusion.project_gather(xyz, calib, img, ordered_grad=True)
            b = fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"], ordered_grad=True)
            ga, gb = torch.autograd.grad(a, img, go)[0], torch.autograd.grad(b, cimg, cgo)[0]
        assert calls.take() == {"hf_project_gather_grad_ordered": 1, "hf_crop_and_resize_grad_ordered": 1}
        assert torch.equal(bits(ga), bits(g_in[0])) and torch.equal(bits(gb), bits(g_in[1]))
    # False asks for the atomics: refused under both levels, the default route outside the mode
    for level in (True, "image"):
        with hf.deterministic(level):
            with pytest.raises(RuntimeError, match="project_gather"):
                fusion.project_gather(xyz, calib, img, ordered_grad=False)
            with pytest.raises(RuntimeError, match="image_crop_and_resize"):
                fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"], ordered_grad=False)
            with pytest.raises(RuntimeError, match="image_crop_and_resize"):                  # the tensor form on the device
                fusion.image_crop_and_resize(cimg.double(), boxes.double(), ind, d["ch"])
    torch.autograd.grad(fusion.project_gather(xyz, calib, img, ordered_grad=False), img, go)
    torch.autograd.grad(fusion.image_crop_and_resize(cimg, boxes, ind, d["ch"], ordered_grad=False), cimg, cgo)
    assert calls.take() == {"hf_project_gather_grad": 1, "hf_crop_and_resize_grad": 1}


# ------------------------------------------------------------------------------------------------------------ whole models
def _no_gradient_differs(model, run, image):
    seen = []
    hook = image.register_hook(lambda g: seen.append(g.clone()))
    with hf.deterministic("image"):
        a, b = _twice(model, run)
    hook.remove()
    assert len(seen) == 2 and float(seen[0].abs().sum()) > 0
    a["(image)"], b["(image)"] = seen
    assert a.keys() == b.keys() and len(a) > 10
    differ = [n for n in a if not torch.equal(bits(a[n]), bits(b[n]))]
    assert not differ, "gradients whose bits differ between two runs from one state: %s" % differ


def test_rpn_model_with_the_image_repeats_every_gradient():
    from test_graph_step import _frames, _small_multiclass

    from heterofusionrcnn_amd import rpn as R_
    cfg = _small_multiclass(dropout=0.5)
    inp = _frames(cfg, 2, 2048, seed=0)
    torch.manual_seed(4)
    model = R_.RpnModel(cfg).cuda().train()

    def run():
        seg, head = model(inp["xyz"], inp["intensity"], img_fts=inp["img_fts"], calib=inp["calib"])
        return model.loss(inp["xyz"], seg, head, inp["label_cls"], inp["label_reg"])[0]

    _no_gradient_differs(model, run, inp["img_fts"])


def test_rcnn_model_with_its_image_rois_repeats_every_gradient():
    from test_roi_image import small_rcnn, small_scene
    _, model = small_rcnn()
    model.train()
    s = small_scene(11)
    s["img_fts"].requires_grad_(True)
    args = (s["xyz"], s["rpn_fts"], s["intensity"], s["fg_mask"], s["proposals"], s["img_fts"], s["calib"])

    def run():
        outs = model(*args)
        return sum(o.square().sum() for o in outs[:2])

    _no_gradient_differs(model, run, s["img_fts"])


# ------------------------------------------------------------------------------------------------------------ file-fed runs
def _saved_bits(path):
    """the bytes of every saved tensor (the image pyramid's BatchNorm counters are 0-dim int64: flattened before the byte view)"""
    sd = torch.load(path, map_location="cpu")
    return {k: v.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes() for k, v in sd.items() if isinstance(v, torch.Tensor)}


def _repeat_and_resume(tmp, which, common):
    """4 steps with a checkpoint at 2; the same again; a resume from step 2 in a fresh process: equal bits everywhere"""
    from heterofusionrcnn_amd import checkpoint as C
    runs = {}
    for tag in ("full", "again"):
        runs[tag] = TR._run(tmp, which, steps=4, checkpoint_dir=os.path.join(tmp, tag), checkpoint_every=2,
                            save=os.path.join(tmp, tag + ".pt"), **common)
    res_dir = os.path.join(tmp, "res")
    os.makedirs(res_dir)
    shutil.copy(C.checkpoint_path(os.path.join(tmp, "full"), 2), res_dir)
    runs["resumed"] = TR._run(tmp, which, steps=4, checkpoint_dir=res_dir, resume=True, save=os.path.join(tmp, "resumed.pt"), **common)
    full, again, resumed = runs["full"], runs["again"], runs["resumed"]
    print("losses", full.tolist(), again.tolist(), resumed.tolist())
    assert len(full) == 4 and len(resumed) == 2 and np.isfinite(full).all()
    assert full.tobytes() == again.tobytes(), "the repeated run's losses differ"
    assert full[2:].tobytes() == resumed.tobytes(), "the resumed run's losses differ"
    p_full = _saved_bits(os.path.join(tmp, "full.pt"))
    assert len(p_full) > 20 and any("vgg" in k.lower() or "img" in k.lower() for k in p_full), sorted(p_full)[:20]
    for tag in ("again", "resumed"):
        p = _saved_bits(os.path.join(tmp, tag + ".pt"))
        assert p.keys() == p_full.keys()
        differ = [k for k in p if p[k] != p_full[k]]
        assert not differ, "%s: saved tensors whose bits differ from the uninterrupted run: %s" % (tag, differ[:10])


def test_rpn_multiclass_runs_repeat_and_resume_bit_for_bit(dataset, tmp_path):  # noqa: F811
    common = dict(dataset_dir=dataset, split="train", batch=2, seed=1, log_every=0, workers=2, config="rpn_multiclass",
                  img_conv=TR.IMG_CONV, deterministic="image", **TR.TRAIN_OP)
    _repeat_and_resume(str(tmp_path), "rpn", common)


def test_rcnn_runs_repeat_and_resume_bit_for_bit(dataset, handoff, tmp_path):  # noqa: F811
    common = dict(dataset_dir=dataset, handoff_dir=handoff, split="train", batch=2, seed=1, log_every=0, workers=2, img_conv=TR.IMG_CONV,
                  deterministic="image", **TR.TRAIN_OP)
    _repeat_and_resume(str(tmp_path), "rcnn", common)
