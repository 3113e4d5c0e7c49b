"""GPU tests of the file-to-file detector (csrc/kitti_result.hip, inference.result_boxes, rcnn_data.handoff_in_memory,
detect.py): the result-row kernel against the host writer's own functions on seeded boxes (tests/detect_cases.py), and detect()
from two saved models against the route over the on-disk hand-off (export_rpn + rcnn_data.run_rcnn_from_handoff) on the
committed KITTI frames of tests/golden/kitti."""
import lzma
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

import detect_cases as DC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
UNLABELLED = "000004"                 # a copy of 000001 without a label file: the val split's fifth frame (a short last batch)
IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))


# ------------------------------------------------------------------------------------------------ the kernel
def _device_dets(dets):
    return [{k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()} for d in dets]


@pytest.mark.parametrize("empty", DC.EMPTY_FRAMES)
def test_result_boxes_equal_the_host_writer(empty):
    """keep on every row that is not within 1e-6 px of a decision boundary; boxes2d of kept rows within 1e-9 max(1, |ref|): both
    sides are fp64 in one operation order and differ by ulps of cos / sin (ocml against glibc) and of the 4-term dot products,
    f * 3e-16 m * (1 + X/Z) ~ 1e-11 px for a corner a metre or more in front at f ~ 721"""
    from heterofusionrcnn_amd.inference import result_boxes, result_rows, write_frame_results, write_result_rows
    cases = DC.make_cases(empty)
    keep_ref, b2_ref, near, _, _ = DC.reference(cases)
    n = len(keep_ref)
    assert near.sum() <= DC.CAP * n
    res = result_boxes(_device_dets(cases["dets"]), cases["p2"], cases["wh"], DC.SCORE_THRESHOLD)
    assert res["counts"] == [len(d["boxes"]) for d in cases["dets"]] and res["counts"][empty] == 0
    keep, b2 = res["keep"].cpu().numpy(), res["boxes2d"].cpu().numpy()
    assert keep.dtype == np.bool_ and keep.shape == (n,) and b2.dtype == np.float64 and b2.shape == (n, 4)
    assert res["frame"].cpu().tolist() == [f for f in range(3) for _ in range(res["counts"][f])]
    sure = ~near
    print("rows %d, near a boundary %d, kept %d (reference %d)" % (n, near.sum(), keep.sum(), keep_ref.sum()))
    assert np.array_equal(keep[sure], keep_ref[sure]), np.nonzero(keep != keep_ref)[0]
    both = keep & keep_ref
    err = np.abs(b2[both] - b2_ref[both]) / np.maximum(1.0, np.abs(b2_ref[both]))
    print("largest relative rectangle error on %d kept rows: %.3g" % (both.sum(), err.max()))
    assert both.sum() >= 30 and err.max() <= 1e-9
    # p2 and image_wh as device tensors (what detect() passes: the fp64 P2 of the batch assembly, rounded to float32 inside)
    again = result_boxes(_device_dets(cases["dets"]), torch.from_numpy(cases["p2"].astype(np.float64)).cuda(),
                         torch.from_numpy(cases["wh"]).cuda(), DC.SCORE_THRESHOLD)
    assert torch.equal(again["keep"], res["keep"]) and torch.equal(again["boxes2d"], res["boxes2d"])
    # the packed rows through the writer: as many lines per frame as write_frame_results writes (rows on a boundary aside)
    rows = result_rows(res).cpu().numpy()
    if not near.any():
        import tempfile
        with tempfile.TemporaryDirectory() as tmp:
            at = 0
            for f, det in enumerate(cases["dets"]):
                cnt = res["counts"][f]
                a = write_frame_results(os.path.join(tmp, "a.txt"), det, cases["p2"][f], tuple(int(v) for v in cases["wh"][f]),
                                        DC.SCORE_THRESHOLD)
                assert write_result_rows(os.path.join(tmp, "b.txt"), rows[at:at + cnt]) == a
                at += cnt


def test_result_boxes_with_no_detection():
    from heterofusionrcnn_amd.inference import result_boxes
    cases = DC.make_cases()
    nothing = _device_dets([cases["dets"][1]] * 3)
    res = result_boxes(nothing, cases["p2"], cases["wh"], DC.SCORE_THRESHOLD)
    assert res["boxes2d"].shape == (0, 4) and res["keep"].shape == (0,) and res["counts"] == [0, 0, 0]
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ files to files
def _png(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    """the golden frames as tests/test_rcnn_handoff.py lays them out, plus one frame without a label file; train.txt lists the
    four labelled frames, val.txt all five"""
    root = tmp_path_factory.mktemp("kitti")
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    for i, n in enumerate(NAMES):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        _png(os.path.join(root, "image_2", n + ".png"), *SIZES[n], seed=i)
    shutil.copy(os.path.join(root, "velodyne", "000001.bin"), os.path.join(root, "velodyne", UNLABELLED + ".bin"))
    shutil.copy(os.path.join(root, "calib", "000001.txt"), os.path.join(root, "calib", UNLABELLED + ".txt"))
    _png(os.path.join(root, "image_2", UNLABELLED + ".png"), *SIZES["000001"], seed=9)
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(NAMES) + "\n")
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("\n".join(NAMES + [UNLABELLED]) + "\n")
    return str(root)


@pytest.fixture(scope="module")
def routes(dataset, tmp_path_factory):
    """two briefly trained, saved models; the file route's results; detect()'s results with host rows and with device rows
    (handoff_rounding, threshold 0) and unrounded.  batch 2 and seed 3 everywhere."""
    from heterofusionrcnn_amd import export_rpn, train_rcnn, train_rpn
    from heterofusionrcnn_amd import rcnn_data as RD
    from heterofusionrcnn_amd.detect import detect
    from heterofusionrcnn_amd import kitti_data as KD
    out = str(tmp_path_factory.mktemp("detect"))
    rpn_pt, rcnn_pt, handoff = os.path.join(out, "rpn.pt"), os.path.join(out, "rcnn.pt"), os.path.join(out, "handoff")
    kw = dict(batch=2, seed=3, workers=2, img_conv=IMG_CONV)
    ck = {k: os.path.join(out, "ckpt_" + k) for k in ("rpn", "rcnn")}         # a checkpoint at the last step: the saved weights
    quiet = lambda *a: None
    train_rpn.train(dataset, "train", steps=2, log_every=0, graph=False, save=rpn_pt, checkpoint_dir=ck["rpn"], checkpoint_every=2,
                    log=quiet, **kw)
    export_rpn.export(dataset, rpn_pt, handoff, "val", log=None, **kw)
    train_rcnn.train(dataset, handoff, "train", steps=2, log_every=0, graph=False, save=rcnn_pt, checkpoint_dir=ck["rcnn"],
                     checkpoint_every=2, log=quiet, **kw)
    names = KD.read_split(dataset, "val")
    c = RD.feature_shape(RD.handoff_paths(handoff, names[0])["features"])[1] - 5
    trainer = train_rcnn.make_trainer(c, IMG_CONV)
    trainer.load_state_dict(torch.load(rcnn_pt, map_location="cpu"), strict=True)
    dirs = {k: os.path.join(out, k) for k in ("file", "host", "device", "plain", "ckpt")}
    written = {"file": RD.run_rcnn_from_handoff(trainer, dataset, handoff, names, dirs["file"], batch=2, workers=2, score_threshold=0.0)}
    common = dict(split="val", score_threshold=0.0, **kw)
    written["host"] = detect(dataset, rpn_pt, rcnn_pt, dirs["host"], handoff_rounding=True, host_rows=True, **common)
    written["device"] = detect(dataset, rpn_pt, rcnn_pt, dirs["device"], handoff_rounding=True, **common)
    written["plain"] = detect(dataset, rpn_pt, rcnn_pt, dirs["plain"], handoff_rounding=False, **common)
    from heterofusionrcnn_amd import checkpoint as ckpt_mod
    ckpts = [ckpt_mod.latest_checkpoint(ck[k]) for k in ("rpn", "rcnn")]
    assert all(p is not None and p.endswith("ckpt-00000002.pt") for p in ckpts), ckpts
    written["ckpt"] = detect(dataset, ckpts[0], ckpts[1], dirs["ckpt"], handoff_rounding=True, **common)
    return {"names": names, "dirs": dirs, "written": written, "rpn": rpn_pt, "rcnn": rcnn_pt, "channels": c}


def _lines(path):
    with open(path) as f:
        return [l.split() for l in f if l.strip()]


def test_host_rows_are_byte_identical_to_the_file_route(routes):
    """the same kernels see the same bits: the in-memory hand-off with the file's rounding changes nothing"""
    assert sorted(routes["written"]["host"]) == sorted(routes["names"]) and routes["written"]["host"] == routes["written"]["file"]
    assert sum(routes["written"]["file"].values()) > 0, "no row was written: the comparison is vacuous"
    for n in routes["names"]:
        a = open(os.path.join(routes["dirs"]["file"], n + ".txt"), "rb").read()
        b = open(os.path.join(routes["dirs"]["host"], n + ".txt"), "rb").read()
        assert a == b, n


def test_device_rows_match_the_file_route(routes):
    """types and row counts equal, 3-D boxes and scores string-identical, image boxes within one unit of the last written digit"""
    assert routes["written"]["device"] == routes["written"]["file"]
    total, worst = 0, 0.0
    for n in routes["names"]:
        a, b = _lines(os.path.join(routes["dirs"]["file"], n + ".txt")), _lines(os.path.join(routes["dirs"]["device"], n + ".txt"))
        assert len(a) == len(b) == routes["written"]["device"][n], n
        for la, lb in zip(a, b):
            assert len(lb) == 16 and la[:4] == lb[:4] and la[8:] == lb[8:], (n, la, lb)
            worst = max(worst, max(abs(float(x) - float(y)) for x, y in zip(la[4:8], lb[4:8])))
        total += len(a)
    print("rows %d, largest image-box difference %.4f px" % (total, worst))
    assert total > 0 and worst <= 0.011


def test_checkpoint_files_load_like_the_saved_state_dicts(routes):
    """RPN.pt / RCNN.pt as ckpt-NNNNNNNN.pt files (checkpoint.model_state unwraps them): the files of the --save route, byte for byte"""
    assert routes["written"]["ckpt"] == routes["written"]["device"]
    for n in routes["names"]:
        assert open(os.path.join(routes["dirs"]["ckpt"], n + ".txt"), "rb").read() == \
            open(os.path.join(routes["dirs"]["device"], n + ".txt"), "rb").read(), n


def test_unrounded_handoff_writes_a_file_for_every_frame(routes):
    assert sorted(routes["written"]["plain"]) == sorted(routes["names"])
    for n in routes["names"]:
        rows = _lines(os.path.join(routes["dirs"]["plain"], n + ".txt"))
        assert len(rows) == routes["written"]["plain"][n] and all(len(r) == 16 for r in rows)
        assert np.isfinite(np.array([[float(v) for v in r[1:]] for r in rows], dtype=np.float64)).all()


def test_detect_restores_the_modes_and_takes_built_models(dataset, routes, tmp_path):
    """built modules instead of files: put in eval() for the run and restored afterwards; same rows as from the files"""
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    from heterofusionrcnn_amd.detect import detect, rpn_fts_channels
    net, _ = train_rpn.make_model("rpn_multiclass", IMG_CONV)
    net.load_state_dict(torch.load(routes["rpn"], map_location="cpu"), strict=True)
    assert rpn_fts_channels(net.rpn) == routes["channels"]
    trainer = train_rcnn.make_trainer(routes["channels"], IMG_CONV)
    trainer.load_state_dict(torch.load(routes["rcnn"], map_location="cpu"), strict=True)
    net.train()
    trainer.train()
    got = detect(dataset, net, trainer, str(tmp_path / "r"), split="val", batch=2, seed=3, workers=2, score_threshold=0.0,
                 handoff_rounding=True)
    assert net.training and trainer.model.training
    assert got == routes["written"]["device"]
    for n in routes["names"]:
        assert open(os.path.join(str(tmp_path / "r"), n + ".txt"), "rb").read() == \
            open(os.path.join(routes["dirs"]["device"], n + ".txt"), "rb").read()


def test_cli_detects_and_evaluates(dataset, tmp_path):
    """python -m heterofusionrcnn_amd.detect with a points-only RPN and the default RCNN (saved untrained: the command line is
    what is under test), --eval printing kitti_eval's report"""
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    from heterofusionrcnn_amd.detect import rpn_fts_channels
    rpn_pt, rcnn_pt, out = str(tmp_path / "rpn.pt"), str(tmp_path / "rcnn.pt"), str(tmp_path / "results")
    torch.manual_seed(0)
    net, with_image = train_rpn.make_model("rpn_multiclass_points")
    assert not with_image
    torch.save(net.state_dict(), rpn_pt)
    torch.save(train_rcnn.make_trainer(rpn_fts_channels(net)).state_dict(), rcnn_pt)
    del net
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run(["timeout", "-k", "10", "600", sys.executable, "-m", "heterofusionrcnn_amd.detect", dataset, rpn_pt, rcnn_pt, out,
                        "--split", "train", "--config", "rpn_multiclass_points", "--batch", "3", "--workers", "2", "--score-threshold",
                        "0.0", "--eval"], cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "done: 4 frames" in r.stdout
    assert sorted(os.listdir(out)) == [n + ".txt" for n in NAMES]
    from heterofusionrcnn_amd import kitti_eval
    report = kitti_eval.format_report(kitti_eval.evaluate_dirs(os.path.join(dataset, "label_2"), out))
    assert r.stdout.endswith(report), r.stdout
