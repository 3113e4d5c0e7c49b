"""The dataset and hand-off of tests/test_validate.py, built the way tests/test_rcnn_handoff.py builds its fixtures: the four
committed frames of tests/golden/kitti (scans decompressed into a temporary directory, synthetic PNGs next to them), a briefly
trained RPN with a small image branch, exported at batch 3 (the last batch is short)."""
import lzma
import os
import shutil

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
HW = (360, 1200)
IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))
EXPORT_BATCH, SEED = 3, 0


def _png(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    img = np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
    Image.fromarray(img).save(path)


def build_dataset(root):
    """velodyne/, calib/, label_2/, image_2/ and train.txt under `root` -> str(root)"""
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


def build_handoff(dataset, out):
    """a briefly trained RPN (3 steps at batch 2, saved as <out>/rpn.pt) exported at batch 3 -> (model path, export's totals)"""
    from heterofusionrcnn_amd import export_rpn, train_rpn
    model_path = os.path.join(out, "rpn.pt")
    train_rpn.train(dataset, "train", steps=3, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, save=model_path)
    totals = export_rpn.export(dataset, model_path, out, "train", batch=EXPORT_BATCH, img_conv=IMG_CONV, workers=2, seed=SEED, log=None)
    return model_path, totals
