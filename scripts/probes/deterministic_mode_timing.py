"""What determinism.deterministic costs where it runs.

  kernels   the fused dense X-Conv gradient (pointcnn.xconv_depthwise, all three gradients) in its atomic form and in the workspace
            form the mode takes (hf_xconv_depthwise_grad / hf_xconv_depthwise_grad_ws), alternating in one process; device events
            around `inner` calls per repetition; median, p10 and p90 over the repetitions after a warm-up of both.
  step      the replayed rpn_multiclass_points train step (train_rpn.make_model, batch 8 x 16384 synthetic points, graph_step.TrainStep
            with optim.MultiTensorAdam) with and without the mode, one fresh child process per setting, the settings alternating.
One session on one device: there is no spread between sessions in these numbers.

  python scripts/probes/deterministic_mode_timing.py [--reps 40] [--out profiles/deterministic_mode_timing.json]"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

# rows, k, c, m: the test shape, and dense layers of the sizes the PointCNN configurations have
SHAPES = ((1400, 8, 40, 2), (8192, 8, 160, 2), (32768, 8, 64, 4), (131072, 8, 32, 1))


def percentiles(ms):
    a = np.sort(np.asarray(ms, np.float64))
    return {"median_ms": round(float(np.median(a)), 5), "p10_ms": round(float(np.percentile(a, 10)), 5),
            "p90_ms": round(float(np.percentile(a, 90)), 5)}


def timed(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def kernels(reps, inner=5):
    from heterofusionrcnn_amd import deterministic, pointcnn
    out = {}
    for rows, k, c, m in SHAPES:
        g = torch.Generator().manual_seed(rows)
        x = torch.randn(rows, k, k, generator=g).cuda().requires_grad_(True)
        f = torch.randn(rows, k, c, generator=g).cuda().requires_grad_(True)
        wd = torch.randn(k, c, m, generator=g).cuda().requires_grad_(True)
        go = torch.randn(rows, c * m, generator=g).cuda()

        def run(mode):
            with deterministic(mode):
                torch.autograd.grad((pointcnn.xconv_depthwise(x, f, wd) * go).sum(), (x, f, wd))

        for _ in range(5):
            run(True), run(False)
        torch.cuda.synchronize()
        t_ws, t_at = [], []
        for _ in range(reps):
            t_ws.append(timed(lambda: run(True), inner))
            t_at.append(timed(lambda: run(False), inner))
        r = {"workspace": percentiles(t_ws), "atomic": percentiles(t_at), "reps": reps, "calls_per_rep": inner,
             "what": "forward + all three gradients through autograd"}
        r["ratio_of_medians"] = round(r["workspace"]["median_ms"] / r["atomic"]["median_ms"], 3)
        out["rows%d_k%d_c%d_m%d" % (rows, k, c, m)] = r
        print(rows, k, c, m, r["workspace"], r["atomic"])
    return out


def step_child(mode, reps):
    from heterofusionrcnn_amd import deterministic, rpn as R_, train_rpn
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    b, p = 8, 16384
    torch.manual_seed(0)
    model, _ = train_rpn.make_model("rpn_multiclass_points")
    model.train()
    cfg = model.cfg
    rng = np.random.default_rng(0)
    xyz = np.stack([rng.uniform(-40, 40, (b, p)), rng.uniform(-1.0, 1.7, (b, p)), rng.uniform(0, 70, (b, p))], -1).astype(np.float32)
    boxes, cls = R_.synthetic_ground_truth(rng, b, 10, cfg)
    xyz_t = torch.from_numpy(xyz).cuda()
    inp = {"xyz": xyz_t, "intensity": torch.from_numpy(rng.uniform(-0.5, 0.5, (b, p, 1)).astype(np.float32)).cuda()}
    inp["label_cls"], inp["label_reg"] = R_.point_labels(xyz_t, torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda())
    with deterministic(mode):
        geo = model.geometry(xyz_t)
        opt = MultiTensorAdam([q for q in model.parameters() if q.requires_grad], lr=1e-3)
        step = TrainStep(model, opt, inp, geo, graph=True)
        for _ in range(5):
            step(geometry=geo)
        torch.cuda.synchronize()
        ms = [timed(lambda: step(geometry=geo), 1) for _ in range(reps)]
    print(json.dumps(percentiles(ms)))


def steps(reps, rounds=2):
    out = {"deterministic": [], "default": []}
    for _ in range(rounds):
        for name, mode in (("deterministic", 1), ("default", 0)):
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", str(mode), "--reps", str(reps)],
                               capture_output=True, text=True)
            if r.returncode != 0:
                raise RuntimeError(r.stdout[-2000:] + r.stderr[-2000:])
            out[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(name, out[name][-1])
    return {"what": "replayed rpn_multiclass_points step, batch 8 x 16384 points, one process per entry, settings alternating",
            "reps_per_process": reps, **out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deterministic_mode_timing.json"))
    ap.add_argument("--child", type=int, default=None)
    args = ap.parse_args()
    if args.child is not None:
        return step_child(bool(args.child), args.reps)
    result = {"device": torch.cuda.get_device_name(0), "sessions": 1, "kernels": kernels(args.reps), "step": steps(args.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
