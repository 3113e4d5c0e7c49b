"""Wall time per batch of the RPN loader fed from files: kitti_data.KittiRpnBatches(batch=8, workers=8) over the dataset of
scripts/probes/detect_timing.py (the committed KITTI frames repeated to 64 names, every one x 4 augmentation combinations), 5
warm-up next() calls, then 50 timed with one synchronisation at the end, REPEATS times with a fresh loader each.  Nothing consumes
the batches, so this is the loader alone: reading, packing, the copies and its three device calls.  Prints one JSON line and, when
a path is given, writes it there."""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import detect_timing as DT  # noqa: E402
from heterofusionrcnn_amd import kitti_data as KD  # noqa: E402

BATCH, WORKERS, WARMUP, TIMED, REPEATS = 8, 8, 5, 50, 3


def loader_ms_per_batch(root):
    data = KD.KittiRpnBatches(root, "val", batch=BATCH, workers=WORKERS, seed=0)
    try:
        for _ in range(WARMUP):
            data.next()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(TIMED):
            data.next()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / TIMED
    finally:
        data.close()


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    with tempfile.TemporaryDirectory() as tmp:
        DT.dataset(tmp)
        res = {"device": torch.cuda.get_device_name(0), "batch": BATCH, "workers": WORKERS, "warmup": WARMUP, "timed": TIMED,
               "rpn_loader_ms_per_batch": [loader_ms_per_batch(tmp) for _ in range(REPEATS)]}
    print(json.dumps(res), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
