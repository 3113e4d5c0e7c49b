"""GPU tests of resumable training: train_rpn.train / train_rcnn.train with the reference's train op (clipping, a staircase decay,
TensorFlow's epsilon), dropout and path drop on, a checkpoint at step 3 of 6, then a resume in a fresh process up to step 6;
the CLI round trip (rotation, --resume, export_rpn reading a checkpoint) and the stop on a NaN loss.  On the four committed
KITTI frames of tests/golden/kitti (the fixture pattern of tests/test_rcnn_handoff.py)."""
import json
import lzma
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))
TRAIN_OP = dict(lr=1e-3, clip_norm=1.0, lr_decay=(2, 0.8, True), tf_epsilon=True, check_numerics=True)


def _png(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("kitti")
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    for i, n in enumerate(NAMES):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        _png(os.path.join(root, "image_2", n + ".png"), *SIZES[n], seed=i)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(NAMES) + "\n")
    return str(root)


# one run of train_rpn.train / train_rcnn.train in a fresh process (fresh dropout layer numbering, as a restarted job has):
# argv[1] = a JSON dict of keywords, argv[2] = where the losses go
_RUNNER = r"""
import json, sys
sys.path.insert(0, %r)
import numpy as np
kw = json.loads(sys.argv[1])
which = kw.pop("_which")
for k in ("img_conv", "lr_decay"):
    if kw.get(k) is not None:
        kw[k] = tuple(tuple(v) if isinstance(v, list) else v for v in kw[k])
if which == "rpn":
    from heterofusionrcnn_amd import train_rpn
    losses, _ = train_rpn.train(log=lambda s: None, **kw)
else:
    from heterofusionrcnn_amd import train_rcnn
    losses, _ = train_rcnn.train(log=lambda s: None, **kw)
np.save(sys.argv[2], np.array(losses, dtype=np.float64))
""" % ROOT


def _run(tmp, which, **kw):
    kw = dict(kw, _which=which)
    out = os.path.join(tmp, "losses_%d.npy" % len(os.listdir(tmp)))
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-c", _RUNNER, json.dumps(kw), out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


def _params(path):
    sd = torch.load(path, map_location="cpu")
    return {k: v.double().numpy() for k, v in sd.items() if v.is_floating_point()}


def _param_gap(a, b):
    """|a - b| / |a| over every floating-point entry of two state_dicts (L2).  Not an element-wise bound: Adam moves an element
    by up to ~lr per step whatever the size of its gradient, so an element whose gradient is rounding noise can end up 2 x steps
    x lr apart between two runs that differ only in the order of their atomic sums."""
    num = sum(float(((a[k] - b[k]) ** 2).sum()) for k in a)
    den = sum(float((a[k] ** 2).sum()) for k in a)
    return (num / den) ** 0.5


def _loss_gap(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(a))))


def _resume_check(tmp, which, common, control):
    """run 6 steps (checkpoints at 3 and 6), repeat it, resume from step 3 in a fresh process; then the control (the checkpoint
    with its optimizer state or its step counter left out).
    -> (measured repeat gap, resume gap, control gaps) for losses and parameters"""
    full_dir, again_dir = os.path.join(tmp, "full"), os.path.join(tmp, "again")
    full = _run(tmp, which, steps=6, checkpoint_dir=full_dir, checkpoint_every=3, save=os.path.join(tmp, "full.pt"), **common)
    again = _run(tmp, which, steps=6, checkpoint_dir=again_dir, checkpoint_every=3, save=os.path.join(tmp, "again.pt"), **common)
    from heterofusionrcnn_amd import checkpoint as C
    assert [s for s, _ in C.list_checkpoints(full_dir)] == [3, 6]
    res_dir = os.path.join(tmp, "res")
    os.makedirs(res_dir)
    shutil.copy(C.checkpoint_path(full_dir, 3), res_dir)
    resumed = _run(tmp, which, steps=6, checkpoint_dir=res_dir, resume=True, save=os.path.join(tmp, "resumed.pt"), **common)
    assert len(full) == 6 and len(resumed) == 3 and np.isfinite(full).all()
    pf, pa, pr = _params(os.path.join(tmp, "full.pt")), _params(os.path.join(tmp, "again.pt")), _params(os.path.join(tmp, "resumed.pt"))
    repeat = (_loss_gap(full[3:], again[3:]), _param_gap(pf, pa))
    resume = (_loss_gap(full[3:], resumed), _param_gap(pf, pr))
    # controls: the optimizer state left out (fresh moments and step counter), the global step left out (counter 0)
    ck = C.load_checkpoint(C.checkpoint_path(full_dir, 3))
    controls = []
    for name in (control,):
        bad = dict(ck)
        opt = dict(ck["optimizer"])
        if name == "no_optimizer_state":
            opt["exp_avg"], opt["exp_avg_sq"] = torch.zeros_like(opt["exp_avg"]), torch.zeros_like(opt["exp_avg_sq"])
        opt["step_count"] = torch.zeros_like(opt["step_count"])
        bad["optimizer"] = opt
        d = os.path.join(tmp, name)
        C.save_checkpoint(d, 3, bad)
        lc = _run(tmp, which, steps=6, checkpoint_dir=d, resume=True, save=os.path.join(tmp, name + ".pt"), **common)
        controls.append((name, _loss_gap(full[3:], lc), _param_gap(pf, _params(os.path.join(tmp, name + ".pt")))))
    return repeat, resume, controls


# Tolerance: a repeat of the same run differs by the atomically accumulated gradients (sums whose order varies between runs),
# amplified over the steps.  Each test measures that repeat gap and bounds the resumed run by FACTOR x the gap, with a floor
# for runs that happen to repeat bit for bit.  Measured on MI355X (relative gaps, losses of steps 4-6 | final parameters, L2):
#   RPN   repeat 1.6e-6 | 2.1e-5   resumed 9.5e-8 | 1.2e-6   optimizer state left out 4.6e-2 | 2.9e-2
#   RCNN  repeat 2.0e-5 | 4.6e-6   resumed 1.8e-7 | 2.5e-8   step counter left out    3.9e-1 | 2.2e-2
FACTOR, LOSS_FLOOR, PARAM_FLOOR = 20.0, 1e-5, 1e-5


def _assert_resume(repeat, resume, controls):
    tol_loss, tol_param = max(FACTOR * repeat[0], LOSS_FLOOR), max(FACTOR * repeat[1], PARAM_FLOOR)
    print("repeat gap loss %.3g param %.3g | resume gap loss %.3g param %.3g | tolerance %.3g %.3g | controls %s" % (
        repeat[0], repeat[1], resume[0], resume[1], tol_loss, tol_param, controls))
    assert resume[0] <= tol_loss and resume[1] <= tol_param
    for name, gl, gp in controls:
        assert gl > tol_loss or gp > tol_param, name


def test_rpn_resume_continues_the_uninterrupted_run(dataset, tmp_path):
    common = dict(dataset_dir=dataset, split="train", batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, **TRAIN_OP)
    _assert_resume(*_resume_check(str(tmp_path), "rpn", common, "no_optimizer_state"))


@pytest.fixture(scope="module")
def handoff(dataset, tmp_path_factory):
    from heterofusionrcnn_amd import export_rpn, train_rpn
    out = str(tmp_path_factory.mktemp("handoff"))
    model_path = os.path.join(out, "rpn.pt")
    train_rpn.train(dataset, "train", steps=2, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, save=model_path)
    export_rpn.export(dataset, model_path, out, "train", batch=2, img_conv=IMG_CONV, workers=2, log=None)
    return out


def test_rcnn_resume_continues_the_uninterrupted_run(dataset, handoff, tmp_path):
    common = dict(dataset_dir=dataset, handoff_dir=handoff, split="train", batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV,
                  **TRAIN_OP)
    _assert_resume(*_resume_check(str(tmp_path), "rcnn", common, "no_global_step"))


def _cli(*args):
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m"] + list(args), cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_cli_checkpoint_rotation_resume_and_export(dataset, tmp_path):
    d = str(tmp_path / "ck")
    base = ["heterofusionrcnn_amd.train_rpn", dataset, "--batch", "2", "--workers", "2", "--log-every", "2", "--reference-train-op",
            "--checkpoint-dir", d, "--checkpoint-every", "2", "--max-checkpoints", "1"]
    out = _cli(*(base + ["--steps", "4"]))
    assert "lr 0.001" in out and "done: 4 steps" in out
    assert os.listdir(d) == ["ckpt-00000004.pt"]
    out = _cli(*(base + ["--resume", "--steps", "6"]))
    assert "step 6 loss" in out and "done: 2 steps" in out
    assert os.listdir(d) == ["ckpt-00000006.pt"]
    from heterofusionrcnn_amd import checkpoint as C
    ck = C.load_checkpoint(os.path.join(d, "ckpt-00000006.pt"))
    assert ck["global_step"] == 6 and float(ck["optimizer"]["step_count"]) == 6.0 and ck["config"] == "rpn_multiclass"
    hand = str(tmp_path / "handoff")
    out = _cli("heterofusionrcnn_amd.export_rpn", dataset, os.path.join(d, "ckpt-00000006.pt"), hand, "--batch", "2", "--workers", "2")
    assert "done: 4 frames" in out
    assert sorted(os.listdir(os.path.join(hand, "rpn_feature"))) == [n + ".npy" for n in NAMES]


def test_nan_loss_stops_the_run_before_the_next_checkpoint(dataset, tmp_path, monkeypatch):
    from heterofusionrcnn_amd import kitti_data as KD
    from heterofusionrcnn_amd import train_rpn

    class Poisoned(KD.KittiRpnBatches):
        drawn = 0

        def next(self):
            b = super().next()
            if Poisoned.drawn == 3:                       # the batch of global step 4: no step runs on the NaN parameters
                b["intensity"].fill_(float("nan"))
            Poisoned.drawn += 1
            return b

    monkeypatch.setattr(train_rpn, "KittiRpnBatches", Poisoned)
    d = str(tmp_path / "ck")
    with pytest.raises(FloatingPointError, match="global step 4"):
        train_rpn.train(dataset, "train", steps=6, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, checkpoint_dir=d,
                        checkpoint_every=2, log=lambda s: None, **TRAIN_OP)
    assert os.listdir(d) == ["ckpt-00000002.pt"]
