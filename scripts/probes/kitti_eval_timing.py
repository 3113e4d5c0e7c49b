"""Timing of the device KITTI evaluator on a val-sized synthetic set (3769 frames, tests/kitti_eval_np.synthetic_set):
the device evaluation (hf_kitti_eval, host-to-device copies and the one read back included; parsing excluded), the host parse
of the same set written as KITTI files, and the NumPy restatement of the rules on the same frames.

    python scripts/probes/kitti_eval_timing.py [--out profiles/kitti_eval_timing.json] [--repeats 10]

Per-kernel times come from a separate run under rocprofv3 --kernel-trace --stats (--kernels-only skips the host timings)."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import kitti_eval_np as R  # noqa: E402
from heterofusionrcnn_amd import kitti_eval as KE  # noqa: E402


def write_set(d, g, det):
    os.makedirs(os.path.join(d, "gt"))
    os.makedirs(os.path.join(d, "res"))
    for i, ((gt_t, gt_v), (dt, dv)) in enumerate(zip(g, det)):
        with open(os.path.join(d, "gt", "%06d.txt" % i), "w") as f:
            for t, v in zip(gt_t, gt_v):
                f.write("%s %.2f %d %s\n" % (t, v[0], int(v[1]), " ".join("%.4f" % x for x in v[2:])))
        with open(os.path.join(d, "res", "%06d.txt" % i), "w") as f:
            for t, v in zip(dt, dv):
                f.write("%s -1 -1 %s\n" % (t, " ".join("%.4f" % x for x in v[2:])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kitti_eval_timing.json"))
    ap.add_argument("--frames", type=int, default=3769)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    g, d = R.synthetic_set(a.frames, 5)
    p = KE.pack_frames(g, d)
    for _ in range(2):                                              # warm-up: code objects, allocator
        KE.evaluate_packed(p)
    torch.cuda.synchronize()
    if a.kernels_only:
        for _ in range(a.repeats):
            KE.evaluate_packed(p)
        torch.cuda.synchronize()
        return
    dev = []
    for _ in range(a.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        KE.evaluate_packed(p)                                        # ends in the host read: synchronised
        dev.append(time.perf_counter() - t0)
    with tempfile.TemporaryDirectory() as tmp:
        write_set(tmp, g, d)
        t0 = time.perf_counter()
        KE.load_dirs(os.path.join(tmp, "gt"), os.path.join(tmp, "res"))
        parse = time.perf_counter() - t0
    t0 = time.perf_counter()
    R.evaluate(g, d)
    restate = time.perf_counter() - t0
    out = {
        "set": {"frames": a.frames, "gt_rows": int(len(p.gt)), "detections": int(len(p.det)), "pairs": int(p.pair_off()[-1]),
                "generator": "tests/kitti_eval_np.synthetic_set(3769, seed=5)"},
        "device_eval_ms": {"median": 1e3 * float(np.median(dev)), "min": 1e3 * float(np.min(dev)), "max": 1e3 * float(np.max(dev)),
                           "repeats": a.repeats,
                           "what": "evaluate_packed: uploads, hf_kitti_eval, one read back; host clock around a synchronised call"},
        "host_parse_ms": 1e3 * parse,
        "numpy_restatement_ms": 1e3 * restate,
        "reference_binary_ms": None,
        "reference_binary_note": "unmeasured: evaluate_object_3d_offline.cpp needs boost, which no machine that runs this has",
        "device": torch.cuda.get_device_name(0),
    }
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
