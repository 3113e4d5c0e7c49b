"""What the ordered image-feature gradients cost against the atomic ones.

  kernels   hf_project_gather_grad / hf_project_gather_grad_ordered at (8, 16384) points on the (8,360,1200,32) map, and on one frame with
            all 16384 points on ONE pixel (the adversarial list); hf_crop_and_resize_grad / hf_crop_and_resize_grad_ordered at
            (B, RoIs per frame) = (8,100), (2,64), (8,64), crop 7 x 7 x 32, the shapes and boxes of scripts/roi_image_timing.py.  Through the
            C ABI, the two entries alternating in one process; device events around `inner` calls per repetition; median, p10 and p90
            over the repetitions after a warm-up of both.  Both forms write the whole map once (the atomic form as its zero fill), so the
            map's write is the floor of either; `map_write_ms` times that fill alone.  The two results are compared on the timed inputs.
  step      the replayed rpn_multiclass train step at batch 8 (bench.py's: RpnModel, a resident (8,360,1200,32) feature map whose
            gradient is the step's last output) and the replayed train_rcnn step at batch 2 (train_rcnn.make_trainer with the VGG
            pyramid), under deterministic("image") and with the mode off, one fresh child process per setting, the settings alternating.
One session on one device: there is no spread between sessions in these numbers.

  python scripts/probes/ordered_image_grad_timing.py [--reps 40] [--out profiles/ordered_image_grad_timing.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

H, W, C, CROP = 360, 1200, 32, 7
CROP_SHAPES = (("detect_b8_n100", 8, 100), ("train_b2_n64", 2, 64), ("train_b8_n64", 8, 64))


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


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def alternate(ordered, atomic, fill, out, reps, inner):
    """-> the figures of one shape; `out` is the map both entries write"""
    for _ in range(5):
        ordered(), atomic(), fill()
    out.fill_(float("nan"))
    ordered()
    g_ordered = out.clone()
    out.fill_(float("nan"))
    atomic()
    diff = (g_ordered - out).abs().max()
    assert bool(torch.isfinite(g_ordered).all()) and bool(torch.isfinite(out).all())
    again = [g_ordered.clone().fill_(float("nan")) for _ in range(2)]
    for t in again:
        out.fill_(float("nan"))
        ordered()
        t.copy_(out)
    repeats = all(torch.equal(t.view(torch.int32), g_ordered.view(torch.int32)) for t in again)
    torch.cuda.synchronize()
    t_ord, t_at, t_fill = [], [], []
    for _ in range(reps):
        t_ord.append(timed(ordered, inner))
        t_at.append(timed(atomic, inner))
        t_fill.append(timed(fill, inner))
    r = {"ordered": percentiles(t_ord), "atomic": percentiles(t_at), "map_write_ms": percentiles(t_fill), "reps": reps, "calls_per_rep": inner,
         "map_bytes": out.numel() * 4, "max_abs_diff_of_the_two": float(diff), "grad_max_abs": float(g_ordered.abs().max()),
         "ordered_repeats_its_bits": repeats}
    r["ratio_of_medians"] = round(r["ordered"]["median_ms"] / r["atomic"]["median_ms"], 3)
    r["ordered_minus_atomic_ms"] = round(r["ordered"]["median_ms"] - r["atomic"]["median_ms"], 5)
    return r


def kernels(reps, inner=3):
    import bench
    from heterofusionrcnn_amd import _lib, fusion
    L, sp = _lib.lib(), _lib.stream_ptr()
    res = {}

    def project(name, b, p, pix):
        go = torch.randn(b, p, C, device="cuda")
        out = torch.empty(b, H, W, C, device="cuda")
        need = L.hf_project_gather_grad_ordered_workspace(b, p, H, W, C)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        ordered = lambda: _lib.check(L.hf_project_gather_grad_ordered(b, p, H, W, C, vp(go), vp(pix), vp(out), vp(ws), need, sp), name)
        atomic = lambda: _lib.check(L.hf_project_gather_grad(b, p, H, W, C, vp(go), vp(pix), vp(out), sp), name)
        res[name] = dict(alternate(ordered, atomic, out.zero_, out, reps, inner), points=b * p, workspace_bytes=need,
                         longest_list=int(torch.bincount(((torch.arange(b, device="cuda")[:, None] * H + pix[..., 1].long()) * W
                                                          + pix[..., 0].long()).reshape(-1)).max()))
        print(name, json.dumps(res[name]), flush=True)

    rng = np.random.default_rng(0)
    b, p = 8, 16384
    # the pixels of a KITTI-like frustum frame through the projection of the forward (every point has a pixel)
    xyz = torch.from_numpy(bench.kitti_frustum(rng, b, p)).cuda()
    calib = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
    _, pix = fusion.project_gather(xyz, calib, torch.zeros(b, H, W, 4, device="cuda"), return_pixels=True)
    pix = torch.stack([pix[..., 0].clamp(0, W - 1), pix[..., 1].clamp(0, H - 1)], -1).contiguous()
    project("project_b8_p16384", b, p, pix)
    one = torch.zeros(1, p, 2, dtype=torch.int32, device="cuda")
    one[..., 0], one[..., 1] = 600, 180
    project("project_b1_p16384_on_one_pixel", 1, p, one)
    torch.cuda.empty_cache()

    for name, b, n in CROP_SHAPES:
        rng = np.random.default_rng(b * 1000 + n)
        prop = np.concatenate([rng.uniform(-10, 10, (b, n, 1)), rng.uniform(0, 2, (b, n, 1)), rng.uniform(8, 40, (b, n, 1)),
                               rng.uniform(1, 4, (b, n, 3)), rng.uniform(-3, 3, (b, n, 1))], -1).astype(np.float32)
        boxes = fusion.roi_image_boxes(torch.from_numpy(prop).cuda(), torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous(), (H, W))
        ind = torch.arange(b, device="cuda", dtype=torch.int32).repeat_interleave(n)
        go = torch.randn(b * n, CROP, CROP, C, device="cuda")
        out = torch.empty(b, H, W, C, device="cuda")
        dims = (b, H, W, C, b * n, CROP, CROP)
        need = L.hf_crop_and_resize_grad_ordered_workspace(*dims)
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        ordered = lambda: _lib.check(L.hf_crop_and_resize_grad_ordered(*dims, vp(go), vp(boxes), vp(ind), vp(out), vp(ws), need, sp), name)
        atomic = lambda: _lib.check(L.hf_crop_and_resize_grad(*dims, vp(go), vp(boxes), vp(ind), vp(out), sp), name)
        res["crop_" + name] = dict(alternate(ordered, atomic, out.zero_, out, reps, inner), rois=b * n, workspace_bytes=need)
        print(name, json.dumps(res["crop_" + name]), flush=True)
        del out, ws, go
        torch.cuda.empty_cache()
    return res


def step_child(which, level, reps):
    import bench
    from heterofusionrcnn_amd import deterministic, rpn as R_
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    torch.manual_seed(0)
    with deterministic(level):
        if which == "rpn_multiclass":
            b, p = 8, bench.N0
            rng = np.random.default_rng(0)
            cfg = R_.rpn_multiclass(bench.IMG_C)
            model = R_.RpnModel(cfg).cuda().train()
            xyz = torch.from_numpy(bench.kitti_frustum(rng, b, p)).cuda()
            inp = {"xyz": xyz, "intensity": torch.from_numpy(rng.uniform(-0.5, 0.5, (b, p, 1)).astype(np.float32)).cuda()}
            boxes, cls = R_.synthetic_ground_truth(rng, b, 12, cfg, ground_y=3.0)
            inp["label_cls"], inp["label_reg"] = R_.point_labels(xyz, torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda())
            inp["img_fts"] = torch.randn(b, bench.IMG_H, bench.IMG_W, bench.IMG_C, device="cuda").requires_grad_(True)
            inp["calib"] = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
            geo = model.geometry(xyz)
            train = TrainStep(model, MultiTensorAdam(list(model.parameters()), lr=1e-3), inp, geo, graph=True)
            step = lambda: train(geometry=geo)
        else:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            from test_rcnn_train import rcnn_scene

            from heterofusionrcnn_amd import rcnn_train as RT
            from heterofusionrcnn_amd.train_rcnn import make_trainer
            inputs = rcnn_scene(2, 7)
            inputs["img_fts"] = torch.rand(2, bench.IMG_H, bench.IMG_W, 3, device="cuda") * 255.0
            tr = make_trainer(288, seed=0)
            step = TrainStep(tr, MultiTensorAdam(tr.parameters(), lr=1e-3), inputs, None, graph=True, loss_fn=RT.rcnn_train_loss)
        for _ in range(5):
            step()
        torch.cuda.synchronize()
        ms = [timed(step, 1) for _ in range(reps)]
    print(json.dumps(percentiles(ms)))


def steps(reps, rounds=2):
    out = {}
    for which, what in (("rpn_multiclass", "replayed rpn_multiclass step, batch 8 x 16384 points, resident (8,360,1200,32) feature map with a gradient"),
                        ("train_rcnn", "replayed train_rcnn step, batch 2, 512 proposals / frame, 64 RoIs, with the VGG pyramid")):
        r = {"what": what + "; one process per entry, settings alternating", "reps_per_process": reps, "image": [], "off": []}
        for _ in range(rounds):
            for name in ("image", "off"):
                p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", which, "--level", name,
                                    "--reps", str(reps)], capture_output=True, text=True)
                if p.returncode != 0:
                    raise RuntimeError(p.stdout[-2000:] + p.stderr[-2000:])
                r[name].append(json.loads(p.stdout.strip().splitlines()[-1]))
                print(which, name, r[name][-1], flush=True)
        out[which] = r
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ordered_image_grad_timing.json"))
    ap.add_argument("--child", default="")
    ap.add_argument("--level", default="off")
    ap.add_argument("--skip-steps", action="store_true")
    args = ap.parse_args()
    if args.child:
        return step_child(args.child, "image" if args.level == "image" else False, args.reps)
    result = {"device": torch.cuda.get_device_name(0), "sessions": 1, "kernels": kernels(args.reps)}

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")

    write()
    if not args.skip_steps:
        result["step"] = steps(args.reps)
        write()
    print("wrote", args.out)


if __name__ == "__main__":
    main()
