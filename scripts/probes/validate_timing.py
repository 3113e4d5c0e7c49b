"""Timing of the validation statistics (csrc/eval_stats.hip) and of validate_rpn against export_rpn.export.

    python scripts/probes/validate_timing.py [--out profiles/validate_timing.json] [--repeats 200] [--passes 3]

1. Per batch at (B, m, g) = (8, 100, 16) and points (8, 16384, 4), boxes from tests/eval_stats_cases.py's frame generator:
   hf_proposal_stats (no matrices asked for) and hf_argmax_accuracy, by device events and by a host clock around a synchronised
   call; beside them the route to the recall counts there was before: hf_box3d_iou_matrix, the copy of the (B, m, g) tensor to the
   host, export_rpn.recall_counts per frame (host clock; the copy synchronises).  The routes alternate call by call in one process.
2. Frames per second of validate.validate_rpn and of export_rpn.export (which writes the hand-off files) over the same frames: the
   four committed frames of tests/golden/kitti repeated --frames / 4 times, an untrained rpn_multiclass model, batch 8; one
   warm-up pass each, then --passes alternating passes, host clock (both end in a host read)."""
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

import eval_stats_cases as ec  # noqa: E402
import validate_fixtures as VF  # noqa: E402
from heterofusionrcnn_amd import export_rpn, train_rpn, validate  # noqa: E402
from heterofusionrcnn_amd.rcnn_data import box3d_iou_matrix  # noqa: E402

B, M, G, P, C = 8, 100, 16, 16384, 4


def stats(x, unit=1e6):
    x = np.asarray(x, np.float64) * unit
    return {"median": float(np.median(x)), "min": float(x.min()), "max": float(x.max()), "calls": int(x.size)}


def batch_inputs():
    case = ec._case("timing", M, G, [ec._fr(M, 11, r70=4, r50=3) for _ in range(B)])
    t = ec.make_proposal_inputs(case)
    cu = lambda a: torch.from_numpy(np.array(a)).cuda()
    rng = np.random.default_rng(0)
    logits = cu(rng.standard_normal((B * P, C)).astype(np.float32))
    target = cu(rng.integers(-1, C, B * P).astype(np.int32))
    return [cu(t[k]) for k in ("proposals", "proposal_count", "gt", "gt_count")], logits, target, t


def entry_points(repeats):
    ins, logits, target, t = batch_inputs()
    counts = torch.empty((B, 4), dtype=torch.int32, device="cuda")
    sums = torch.empty((B, 3), dtype=torch.float64, device="cuda")
    correct = torch.empty((B,), dtype=torch.int32, device="cuda")
    gcounts = [int(v) for v in t["gt_count"]]

    def old_route():
        iou = box3d_iou_matrix(*ins).cpu().numpy()
        return [export_rpn.recall_counts(iou[f, :, :gcounts[f]]) for f in range(B)]

    new_stats = lambda: validate.proposal_stats(*ins, counts=counts, sums=sums)
    new_acc = lambda: validate.argmax_accuracy(logits, target, B, correct)
    for _ in range(10):                                              # warm-up: code objects, allocator
        old, _, _ = old_route(), new_stats(), new_acc()
    torch.cuda.synchronize()
    assert [list(r) for r in old] == counts[:, 2:].cpu().tolist(), "the two routes count different recalls"
    ev = lambda: torch.cuda.Event(enable_timing=True)
    host = {"old_route": [], "proposal_stats": [], "argmax_accuracy": []}
    device = {"proposal_stats": [], "argmax_accuracy": []}
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        old_route()
        host["old_route"].append(time.perf_counter() - t0)
        for name, fn in (("proposal_stats", new_stats), ("argmax_accuracy", new_acc)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            host[name].append(time.perf_counter() - t0)
            a, b = ev(), ev()
            a.record()
            fn()
            b.record()
            b.synchronize()
            device[name].append(a.elapsed_time(b) * 1e-3)
    return {"shape": {"B": B, "m": M, "g": G, "points": [B, P, C], "labels_per_frame": 11},
            "hf_proposal_stats_us": {"device_events": stats(device["proposal_stats"]), "host_clock_synchronised": stats(host["proposal_stats"])},
            "hf_argmax_accuracy_us": {"device_events": stats(device["argmax_accuracy"]), "host_clock_synchronised": stats(host["argmax_accuracy"])},
            "recall_route_before_us": {"host_clock": stats(host["old_route"]),
                                       "what": "hf_box3d_iou_matrix, .cpu() of the (8, 100, 16) tensor, export_rpn.recall_counts per frame"},
            "what": "per batch; the wrappers of validate.py (allocation of the best_* outputs and the workspace included); routes alternate"}


def end_to_end(frames, passes):
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, "kitti")
        os.makedirs(root)
        VF.build_dataset(root)
        names = (VF.NAMES * ((frames + 3) // 4))[:frames]
        net, _ = train_rpn.make_model("rpn_multiclass")
        out = os.path.join(tmp, "handoff")
        run_val = lambda: validate.validate_rpn(root, net, names, batch=8, workers=8)
        run_exp = lambda: export_rpn.export(root, net, out, names, batch=8, workers=8, log=None)
        run_val(), run_exp()                                          # warm-up
        val, exp = [], []
        for _ in range(passes):
            for fn, acc in ((run_val, val), (run_exp, exp)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                acc.append(frames / (time.perf_counter() - t0))
    return {"frames": frames, "batch": 8, "config": "rpn_multiclass (untrained)", "passes": passes,
            "validate_rpn_frames_per_s": stats(val, 1.0), "export_rpn_frames_per_s": stats(exp, 1.0),
            "what": "the four frames of tests/golden/kitti repeated; export also writes the hand-off files; passes alternate"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "validate_timing.json"))
    ap.add_argument("--repeats", type=int, default=200)
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--passes", type=int, default=3)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    out = {"per_batch": entry_points(a.repeats), "end_to_end": end_to_end(a.frames, a.passes), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
