"""Diagnostic: the two routes through the first layer of a feature-propagation MLP, forward plus backward, in one process.

  materialised: three_interpolate_concat writes [interpolated | points1 | 0-pad] (B, N, round_up(C2 + C1, 4)), shared_mlp reads it
                back for the first GEMM and again for the weight gradient
  in place:     mlp.shared_mlp_interp -- hf_linear_bn_fwd_interp / hf_linear_wgrad_interp build the operand rows from
                (points2, idx, weight, points1) while they stage them; the concat tensor never exists

The three shipped full-size FP shapes whose first layer fits the kernels (Cout <= 256), B = 8, real three_nn geometry on
bench.kitti_frustum clouds and their FPS subsets.  The routes alternate step by step inside the timed window (boxes differ by
several per cent, so only a comparison within one run means anything); every step is timed with device events around
zero-grad + forward + backward.  Reports median / p10 / p90 per route, the bytes of the concat tensor the in-place route no longer
moves (written once, read twice), and the largest difference between the routes' outputs and gradients on the timed inputs.
Writes profiles/fp_interp_timing.json (or --out)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import heterofusionrcnn_amd as hf
from heterofusionrcnn_amd import mlp
from heterofusionrcnn_amd.interpolate import three_interpolate_concat
from heterofusionrcnn_amd.modules import PointnetFPModule, SharedMLPLayer
from bench import kitti_frustum

SHAPES = ((16384, 4096, 256, 1, (128, 128)), (4096, 1024, 256, 64, (256, 256)), (4096, 1024, 512, 96, (256, 256)))
B = 8


def pct(samples, q):
    return round(float(np.percentile(np.asarray(samples), q)), 1)


def measure(n, m, c2, c1, widths, repeats, warm):
    rng = np.random.default_rng(n + c2)
    xyz1 = torch.from_numpy(kitti_frustum(rng, B, n)).cuda()
    xyz2 = hf.gather_point(xyz1, hf.farthest_point_sample(m, xyz1))
    idx, weight, inverse = PointnetFPModule.geometry(xyz1, xyz2)
    p2 = torch.randn(B, m, c2, device="cuda").requires_grad_(True)
    p1 = torch.randn(B, n, c1, device="cuda").requires_grad_(True)
    torch.manual_seed(1)
    layers, cin = [], c2 + c1
    for w in widths:
        layers.append(SharedMLPLayer(cin, w).cuda().train())
        cin = w
    assert mlp.interp_mlp_fusable(layers, p2, p1, idx)
    dout = torch.randn(B * n, widths[-1], device="cuda")
    leaves = [p2, p1] + [p for l in layers for p in l.parameters()]

    def materialised():
        x = three_interpolate_concat(p2, p1, idx, weight, inverse)
        return mlp.shared_mlp(layers, x.reshape(-1, x.shape[-1]))

    def in_place():
        return mlp.shared_mlp_interp(layers, p2, p1, idx, weight, inverse)

    routes = (("materialised", materialised), ("in_place", in_place))

    def step(fn, backward=True):
        for p in leaves:
            p.grad = None
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        if backward:
            out.backward(dout)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3, out.detach()

    results = {}
    for name, fn in routes:
        _, out = step(fn)
        results[name] = [out.clone()] + [p.grad.clone() for p in leaves]
    scale = [float(t.abs().max()) for t in results["materialised"]]
    rel = max(float((a - b).abs().max()) / max(s, 1e-30) for a, b, s in zip(results["in_place"], results["materialised"], scale))
    del results
    for _ in range(warm):
        for _, fn in routes:
            step(fn)
    both = {name: [] for name, _ in routes}
    fwd = {name: [] for name, _ in routes}
    for _ in range(repeats):          # alternating: drift of the box hits both routes alike
        for name, fn in routes:
            both[name].append(step(fn)[0])
        for name, fn in routes:
            fwd[name].append(step(fn, backward=False)[0])
    width = (c2 + c1 + 3) // 4 * 4
    concat_bytes = B * n * width * 4
    row = {"b": B, "n": n, "m": m, "c2": c2, "c1": c1, "widths": list(widths), "rows": B * n, "repeats": repeats,
           "concat_bytes": concat_bytes, "concat_traffic_bytes_not_moved": 3 * concat_bytes,
           "default_route_training": bool(mlp.interp_route_pays(B * n, c2 + c1, widths[0], True)),
           "default_route_inference": bool(mlp.interp_route_pays(B * n, c2 + c1, widths[0], False)),
           "max_rel_difference_between_routes": float("%.3g" % rel)}
    for name, _ in routes:
        row[name + "_fwd_bwd_us"] = {"median": pct(both[name], 50), "p10": pct(both[name], 10), "p90": pct(both[name], 90)}
        row[name + "_fwd_us"] = {"median": pct(fwd[name], 50), "p10": pct(fwd[name], 10), "p90": pct(fwd[name], 90)}
    a, b_ = row["in_place_fwd_bwd_us"], row["materialised_fwd_bwd_us"]
    spread = b_["p90"] - b_["p10"]
    row["in_place_no_worse_than_materialised_plus_spread"] = bool(a["median"] <= b_["median"] + spread)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fp_interp_timing.json"))
    args = ap.parse_args()
    assert args.repeats >= 20
    rows = [measure(*s, args.repeats, args.warmup) for s in SHAPES]
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "unit": "us per step (zero-grad + forward + backward), device events",
                   "shapes": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
