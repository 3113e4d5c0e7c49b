"""GPU tests of the RPN training batches (csrc/rpn_batch.hip through heterofusionrcnn_amd/kitti_data.py) on the four committed
KITTI frames of tests/golden/kitti (scans decompressed into a temporary directory, synthetic PNGs of 1242 x 375 and 1224 x 370
written next to them), held against the NumPy restatement in tests/kitti_data_np.py; the ignore label in both RPN losses; and
a file-fed, captured train step end to end."""
import lzma
import os
import shutil
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from heterofusionrcnn_amd import kitti_data as KD
from heterofusionrcnn_amd import rpn as R_

import kitti_data_np as KN

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
HW = (360, 1200)


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


def _device_batch(frames):
    packed = KD.pack_frames(frames, KD._Staging())
    pts, imgs, meta = KD.upload(packed, torch.device("cuda"))
    return packed, pts, imgs, meta


def _points(frames, p, seed=7, rng_state=None):
    packed, pts, _, meta = _device_batch(frames)
    rs = rng_state if rng_state is not None else torch.tensor([seed, 0], dtype=torch.int64, device="cuda")
    out = KD.batch_points(pts, meta["offsets"], meta["velo_to_rect"], meta["p2"], meta["wh"], meta["flip"], rs, p,
                          packed["max_frame_points"])
    return [t.cpu().numpy() for t in out], meta


def _frames(root, augs):
    return [KD.read_frame(root, n, a, KD.CLASSES, HW) for n, a in zip(NAMES, augs)]


def _check_frame(fr, xyz, inten, src, p):
    """the rules of one frame's sample against the restatement; -> (n, n_far) of the restatement"""
    rect, _, inside, margin, zabs = KN.view_filter(fr["points"], fr["velo_to_rect"], fr["p2"], fr["wh"])
    ambiguous = (margin < 1e-6) | (zabs < 1e-9)
    assert (src >= 0).all() and (src < len(fr["points"])).all()
    assert (inside[src] | ambiguous[src]).all(), "a sampled point is outside the view"
    exp = rect[src].copy()
    if fr["flip"]:
        exp[:, 0] = -exp[:, 0]
    np.testing.assert_allclose(xyz, exp, rtol=0, atol=1e-5)
    assert np.array_equal(inten[:, 0], fr["points"][src, 3] - np.float32(0.5))
    n, far = int(inside.sum()), inside & (rect[:, 2] >= 40.0)
    counts = np.bincount(src, minlength=len(fr["points"]))
    sure = inside & ~ambiguous
    if p < n:
        assert counts.max() == 1, "a point drawn twice although n > P"
        assert (counts[far & sure] == 1).all(), "a far point is missing"
    else:
        assert (counts[sure] >= 1).all(), "an in-view point is missing although n <= P"
        assert counts.max() <= (2 if p <= 2 * n else p)
        if p <= 2 * n:
            assert abs(int((counts == 2).sum()) - (p - n)) <= int((ambiguous & (counts > 0)).sum())
    return n, int(far.sum())


def test_points_follow_the_reference_rules(dataset):
    augs = [(), ("flipping",), ("pca_jitter",), ("flipping", "pca_jitter")]
    frames = _frames(dataset, augs)
    (xyz, inten, src, status), _ = _points(frames, 16384)
    assert status.tolist() == [0, 0, 0, 0]
    for f, fr in enumerate(frames):
        n, nf = _check_frame(fr, xyz[f], inten[f], src[f], 16384)
        assert n > 16384 and nf < 16384, (n, nf)   # the committed frames exercise the near-sampling branch


def test_points_are_reproducible_and_advance(dataset):
    frames = _frames(dataset, [(), (), ("flipping",), ()])
    rs = torch.tensor([11, 0], dtype=torch.int64, device="cuda")
    (a, _, sa, _), _ = _points(frames, 16384, rng_state=rs)
    assert rs.cpu().tolist() == [11, 1]
    (b, _, sb, _), _ = _points(frames, 16384, rng_state=rs)
    (c, _, sc, _), _ = _points(frames, 16384, seed=11)
    assert np.array_equal(a, c) and np.array_equal(sa, sc), "same rng_state, different output"
    assert not np.array_equal(sa, sb), "the next call drew the same sample"


def test_points_replacement_branches_and_statuses(dataset):
    fr = _frames(dataset, [()] * 4)
    n0 = int(KN.view_filter(fr[0]["points"], fr[0]["velo_to_rect"], fr[0]["p2"], fr[0]["wh"])[2].sum())
    for p in (n0 + n0 // 2, 3 * n0):                  # n < P <= 2n: without replacement; P > 2n: with replacement
        (xyz, inten, src, status), _ = _points(fr[:1], p)
        assert status.tolist() == [0]
        _check_frame(fr[0], xyz[0], inten[0], src[0], p)
    # more than P far points: a random P of them, status bit; a frame with nothing in view: zeros and the empty bit
    empty = dict(fr[1])
    empty["points"] = fr[1]["points"][:64].copy()
    empty["points"][:, 0] = -np.abs(empty["points"][:, 0]) - 5.0      # behind the camera
    (xyz, inten, src, status), _ = _points([fr[0], empty], 16)
    assert status.tolist() == [KD.STATUS_TOO_MANY_FAR, KD.STATUS_EMPTY]
    rect, _, inside, _, _ = KN.view_filter(fr[0]["points"], fr[0]["velo_to_rect"], fr[0]["p2"], fr[0]["wh"])
    assert len(set(src[0].tolist())) == 16 and (rect[src[0], 2] >= 40.0 - 1e-9).all() and inside[src[0]].all()
    assert (xyz[1] == 0).all() and (inten[1] == 0).all() and (src[1] == -1).all()


def test_near_points_inclusion_rate(dataset):
    fr = _frames(dataset, [()])[:1]
    p, calls = 8192, 200
    rect, _, inside, margin, zabs = KN.view_filter(fr[0]["points"], fr[0]["velo_to_rect"], fr[0]["p2"], fr[0]["wh"])
    sure = inside & (margin >= 1e-6) & (zabs >= 1e-9)
    near, far = sure & (rect[:, 2] < 40.0), sure & (rect[:, 2] >= 40.0)
    rs = torch.tensor([5, 0], dtype=torch.int64, device="cuda")
    packed, pts, _, meta = _device_batch(fr)
    hits = np.zeros(len(fr[0]["points"]))
    for _ in range(calls):
        src = KD.batch_points(pts, meta["offsets"], meta["velo_to_rect"], meta["p2"], meta["wh"], meta["flip"], rs, p,
                              packed["max_frame_points"])[2]
        hits[np.unique(src[0].cpu().numpy())] += 1
    assert (hits[far] == calls).all()
    rate = (p - int((inside & (rect[:, 2] >= 40.0)).sum())) / int((inside & (rect[:, 2] < 40.0)).sum())
    sd = np.sqrt(calls * rate * (1 - rate))
    dev = np.abs(hits[near] - calls * rate) / sd
    assert dev.max() < 6.0, (rate, float(dev.max()))
    assert abs(hits[near].mean() / calls - rate) < 0.01


def test_labels_equal_the_restatement(dataset):
    for augs in ([()] * 4, [("flipping",)] * 4):
        frames = _frames(dataset, augs)
        (xyz, _, _, _), meta = _points(frames, 16384, seed=3)
        lc, lr = KD.point_labels(torch.from_numpy(xyz).cuda(), meta["boxes"], meta["cls"], meta["gt_count"])
        lc, lr = lc.cpu().numpy(), lr.cpu().numpy()
        boxes = meta["boxes"].cpu().numpy()
        near_face = 0
        for f, fr in enumerate(frames):
            ng = len(fr["cls"])
            c, r, near = KN.rpn_labels(xyz[f], boxes[f, :ng].astype(np.float64), fr["cls"])
            diff = c != lc[f]
            assert not (diff & (near >= 1e-4)).any(), "label differs away from a face"
            near_face += int(diff.sum())
            same = ~diff & (near >= 1e-4)
            assert np.array_equal(r[same], lr[f][same])
            assert (c == -1).any() and (c > 0).any()
        print("labels differing within 1e-4 m of a face:", near_face)


def test_labels_hand_built_boxes():
    boxes = np.array([[[0.0, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0], [0.3, 0.0, 0.0, 2.0, 4.0, 1.0, 0.0]]], np.float32)
    pts = np.array([[[0.5, -0.5, 0.0], [-0.8, -0.5, 0.0], [-0.95, -0.5, 0.0], [5.0, -0.5, 0.0], [0.0, 0.0, 0.0], [0.0, 0.2, 0.0]]],
                   np.float32)
    lc, lr = KD.point_labels(torch.from_numpy(pts).cuda(), torch.from_numpy(boxes).cuda(),
                             torch.tensor([[1, 2]], dtype=torch.int32, device="cuda"), torch.tensor([2], dtype=torch.int32, device="cuda"))
    assert lc.cpu().tolist() == [[2, -1, 1, 0, -1, 0]]
    r = lr.cpu().numpy()[0]
    assert np.array_equal(r[0], boxes[0, 1]) and np.array_equal(r[1], boxes[0, 0]) and (r[3] == 0).all()


def test_image_equals_the_restatement(dataset):
    augs = [("pca_jitter",), ("flipping", "pca_jitter"), ("flipping",), ()]
    frames = _frames(dataset, augs)
    packed, _, imgs, meta = _device_batch(frames)
    rs = torch.tensor([9, 0], dtype=torch.int64, device="cuda")
    image, noise, stats = KD.batch_image(imgs, meta["img_offsets"], meta["wh"], meta["flip"], meta["jitter"], rs, HW,
                                         packed["max_pixels"], stats=True)
    image, noise, stats = image.cpu().numpy(), noise.cpu().numpy(), stats.cpu().numpy()
    for f, fr in enumerate(frames):
        img = fr["image"]
        if fr["jitter"]:
            cov = KN.covariance(img)
            np.testing.assert_allclose(stats[f, :9].reshape(3, 3), cov, rtol=1e-10, atol=1e-10 * np.abs(cov).max())
            e, v = stats[f, 9:12], stats[f, 12:21].reshape(3, 3)
            np.testing.assert_allclose(cov @ v, v * e, rtol=0, atol=1e-12 * np.abs(cov).max())
            e_ref, v_ref = np.linalg.eigh(cov)
            np.testing.assert_allclose(e, e_ref, rtol=1e-9, atol=1e-15)
            np.testing.assert_allclose(np.abs((v * v_ref).sum(0)), 1.0, rtol=0, atol=1e-9)   # the same vectors up to sign
            assert np.abs(noise[f]).max() > 0
        else:
            assert (noise[f] == 0).all()
        exp = KN.image_sample(img, fr["flip"], noise[f] if fr["jitter"] else None, HW)
        assert np.array_equal(image[f], exp), (f, int((image[f] != exp).sum()))


def _small_cfg():
    s = R_.SAScale
    return R_.rpn_multiclass_heads(R_.RpnConfig(
        name="small", sa=(R_.SALevel(256, (s(0.8, 16, (16, 16, 32)), s(1.6, 32, (16, 16, 32)))),
                          R_.SALevel(64, (s(3.2, 16, (32, 32, 64)),))),
        fp=((64, 64), (32, 32)), backbone_fc=((32, 0.5), (32, 0.5)), rpn_fc=((64, 0.5), (64, 0.5))))


def test_loss_ignore_label():
    cfg = _small_cfg()
    rng = np.random.default_rng(4)
    b, p = 2, 4096
    xyz = np.stack([rng.uniform(-8, 8, (b, p)), rng.uniform(-1.0, 1.7, (b, p)), rng.uniform(2, 18, (b, p))], -1).astype(np.float32)
    boxes, cls = R_.synthetic_ground_truth(rng, b, 10, cfg, extent=((-7.0, 7.0), (3.0, 17.0)))
    xyz_t = torch.from_numpy(xyz).cuda()
    lab, reg = KD.point_labels(xyz_t, torch.from_numpy(boxes).cuda(), torch.from_numpy(cls.astype(np.int32)).cuda(),
                               torch.full((b,), 10, dtype=torch.int32, device="cuda"))
    assert int((lab == -1).sum()) > 20 and int((lab > 0).sum()) > 20
    g = torch.Generator().manual_seed(2)
    model = R_.RpnModel(cfg)
    seg = torch.randn(b, p, cfg.num_classes + 1, generator=g).cuda().requires_grad_(True)
    head = (2 * torch.randn(b, p, cfg.num_classes, cfg.head_width, generator=g)).cuda().requires_grad_(True)
    loss_f, parts_f = model.loss(xyz_t, seg, head, lab, reg, fused=True)
    gf = torch.autograd.grad(loss_f, (seg, head))
    loss_r, parts_r = model.loss(xyz_t, seg, head, lab, reg, fused=False)
    gr = torch.autograd.grad(loss_r, (seg, head), allow_unused=True)
    assert torch.isfinite(loss_f) and torch.allclose(loss_f, loss_r, rtol=2e-5, atol=1e-6)
    for name in ("segmentation", "bin_classification", "regression", "num_foreground"):
        assert torch.allclose(parts_f[name].float(), parts_r[name].float(), rtol=2e-5, atol=1e-6), name
    for a, r in zip(gf, gr):
        r = torch.zeros_like(a) if r is None else r
        assert torch.allclose(a, r, rtol=1e-4, atol=1e-7 + 1e-5 * float(r.abs().max()))
    ign = (lab == -1)
    assert (gf[0][ign] == 0).all(), "an ignored point has a segmentation gradient"
    # the ignored points' focal terms dropped from the sum, the normaliser still B P
    prob = torch.softmax(seg.detach().double(), -1)
    pt = torch.gather(prob, 2, lab.long().clamp(min=0).unsqueeze(-1)).squeeze(-1).clamp(1e-7, 1 - 1e-7)
    focal = 0.25 * (1 - pt) ** 2 * -torch.log(pt)
    exp = float(focal[~ign].sum()) * cfg.seg_loss_weight / (b * p)
    assert abs(float(parts_f["segmentation"]) - exp) <= 2e-5 * abs(exp)
    assert int(parts_f["num_foreground"]) == int((lab > 0).sum())


def test_file_fed_captured_train_step(dataset):
    from heterofusionrcnn_amd import train_rpn
    losses, status = train_rpn.train(dataset, "train", steps=30, batch=4, seed=1, log_every=0, workers=2,
                                     img_conv=((1, 16), (1, 16), (1, 16), (1, 16)))
    assert len(losses) == 30 and np.isfinite(losses).all()
    assert np.mean(losses[-5:]) < np.mean(losses[:5]), losses
    assert status == {"empty": 0, "too_many_far": 0}


def test_train_rpn_cli(dataset, tmp_path):
    out = tmp_path / "model.pt"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "heterofusionrcnn_amd.train_rpn", dataset, "--steps", "3",
                        "--batch", "2", "--log-every", "1", "--workers", "2", "--save", str(out)], cwd=ROOT, env=env,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "done: 3 steps" in r.stdout
    sd = torch.load(str(out), map_location="cpu")
    assert any(k.startswith("img_net.") for k in sd) and any(k.startswith("rpn.") for k in sd)


def _reader_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("hf-read")]


def test_close_leaves_no_reader_thread(dataset):
    data = KD.KittiRpnBatches(dataset, "train", batch=2, workers=2, seed=3)
    try:
        data.next()
        data.next()
        assert _reader_threads()
    finally:
        data.close()
    assert _reader_threads() == []


def test_a_missing_scan_ends_training_with_no_reader_thread_left(dataset, tmp_path):
    """a fifth labelled frame with calib, label and image but no velodyne file: 12 steps of batch 2 exceed the epoch of 5 frames
    x 4 augmentation combinations, so the loader's next() meets it whatever the shuffle"""
    from heterofusionrcnn_amd import train_rpn
    root = str(tmp_path / "kitti")
    shutil.copytree(dataset, root)
    for d, ext in (("calib", ".txt"), ("label_2", ".txt"), ("image_2", ".png")):
        shutil.copy(os.path.join(root, d, "000000" + ext), os.path.join(root, d, "000004" + ext))
    with open(os.path.join(root, "train.txt"), "a") as f:
        f.write("000004\n")
    with pytest.raises(FileNotFoundError, match="000004"):
        train_rpn.train(root, "train", steps=12, batch=2, seed=1, log_every=0, workers=2, graph=False,
                        img_conv=((1, 16), (1, 16), (1, 16), (1, 16)))
    assert _reader_threads() == []
