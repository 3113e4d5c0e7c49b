"""The image half of the RCNN's RoI pooling (box projection + crop_and_resize) on the (B,360,1200,32) feature map, crop 7, at
(B, n) = (8, 100) detection and (2, 64), (8, 64) training: the kernels of csrc/roi_image.hip against the tensor form they replace
(fusion._project_boxes_to_image_tensor + the column reorder + fusion._image_crop_and_resize_tensor), in one process, the two routes
alternating, forward alone and forward + backward with a gradient on the map.  Device events around `inner` calls per repetition;
median, p10 and p90 over the repetitions after a warm-up of both routes.  `wins` = the tensor form's median exceeds the kernels'
by more than the two p10-p90 spreads together.  The outputs of the two routes are compared on the timed inputs.

  python scripts/roi_image_timing.py [--reps 60] [--out profiles/roi_image_timing.json] [--end-to-end TREE=label,TREE=label [--rounds 2]]

--end-to-end: for every TREE (a checkout of this repository with its library built, e.g. this commit and its parent) a fresh child
process times one train_rcnn step with the image branch (train_rcnn.make_trainer: RcnnTrainer over RcnnModel + ImgVggPyr, batch 2,
eager and replayed) and one two-stage detect batch (TwoStageDetector, batch 2) with that tree's package; trees alternate."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

H, W, C, CROP = 360, 1200, 32, 7
SHAPES = (("detect_b8_n100", 8, 100), ("train_b2_n64", 2, 64), ("train_b8_n64", 8, 64))


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


def alternate(new, old, reps, inner, warmup=5):
    for _ in range(warmup):
        new()
        old()
    torch.cuda.synchronize()
    t_new, t_old = [], []
    for _ in range(reps):
        t_new.append(timed(new, inner))
        t_old.append(timed(old, inner))
    r = {"kernels": percentiles(t_new), "tensor_form": percentiles(t_old), "reps": reps, "calls_per_rep": inner}
    spread = (r["kernels"]["p90_ms"] - r["kernels"]["p10_ms"]) + (r["tensor_form"]["p90_ms"] - r["tensor_form"]["p10_ms"])
    r["speedup_of_medians"] = round(r["tensor_form"]["median_ms"] / r["kernels"]["median_ms"], 2)
    r["wins"] = bool(r["tensor_form"]["median_ms"] - r["kernels"]["median_ms"] > spread)
    return r


def ab(reps):
    sys.path.insert(0, ROOT)
    import bench
    from heterofusionrcnn_amd import fusion
    res = {}
    for name, b, n in SHAPES:
        rng = np.random.default_rng(b * 1000 + n)
        prop = np.concatenate([rng.uniform(-10, 10, (b, n, 1)), rng.uniform(0, 2, (b, n, 1)), rng.uniform(8, 40, (b, n, 1)),
                               rng.uniform(1, 4, (b, n, 3)), rng.uniform(-3, 3, (b, n, 1))], -1).astype(np.float32)
        prop = torch.from_numpy(prop).cuda()
        calib = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
        box_ind = torch.arange(b, device="cuda", dtype=torch.int32).repeat_interleave(n)
        img = torch.randn(b, H, W, C, device="cuda")
        go = torch.randn(b * n, CROP, CROP, C, device="cuda")

        def new_fwd(x=img):
            return fusion.image_crop_and_resize(x, fusion.roi_image_boxes(prop, calib, (H, W)), box_ind, CROP)

        def old_fwd(x=img):
            xyxy = fusion._project_boxes_to_image_tensor(prop, calib, (H, W))[1].reshape(-1, 4)
            yxyx = torch.stack([xyxy[:, 1], xyxy[:, 0], xyxy[:, 3], xyxy[:, 2]], dim=1)
            return fusion._image_crop_and_resize_tensor(x, yxyx, box_ind, CROP)

        leaf = img.clone().requires_grad_(True)

        def both(fwd):
            def run():
                leaf.grad = None
                fwd(leaf).backward(go)
            return run

        with torch.no_grad():
            out_new, out_old = new_fwd(), old_fwd()
            # the two projections differ in the last bits (sinf / cosf), and a crop follows its boxes: the crops are also
            # compared on the SAME boxes, where only the interpolation's roundings are left
            yxyx = fusion.roi_image_boxes(prop, calib, (H, W))
            xyxy = fusion._project_boxes_to_image_tensor(prop, calib, (H, W))[1].reshape(-1, 4)
            boxes_diff = float((yxyx - xyxy[:, [1, 0, 3, 2]]).abs().max())
            same_boxes_diff = float((fusion.image_crop_and_resize(img, yxyx, box_ind, CROP)
                                     - fusion._image_crop_and_resize_tensor(img, yxyx, box_ind, CROP)).abs().max())
            fwd = alternate(new_fwd, old_fwd, reps, inner=10)
        both(new_fwd)()
        g_new = leaf.grad.clone()
        both(old_fwd)()
        g_old = leaf.grad.clone()
        bwd = alternate(both(new_fwd), both(old_fwd), reps, inner=2)
        res[name] = {
            "b": b, "rois": b * n, "forward": fwd, "forward_backward": bwd,
            "agreement": {"boxes_max_abs_diff": boxes_diff, "rois_max_abs_diff_same_boxes": same_boxes_diff,
                          "rois_max_abs_diff": float((out_new - out_old).abs().max()), "img_max_abs": float(img.abs().max()),
                          "grad_max_abs_diff": float((g_new - g_old).abs().max()), "grad_max_abs": float(g_new.abs().max()),
                          "extrapolated_share": round(float((out_new == 0).float().mean()), 4)},
        }
        del img, leaf, go, g_new, g_old, out_new, out_old
        torch.cuda.empty_cache()
    return res


def end_to_end_child(tree, steps):
    """one tree's package: a train_rcnn step with the image branch and a two-stage detect batch, batch 2"""
    sys.path.insert(0, os.path.join(tree, "tests"))
    sys.path.insert(0, tree)
    import bench
    import heterofusionrcnn_amd
    from heterofusionrcnn_amd import rcnn_train as RT
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    from heterofusionrcnn_amd.train_rcnn import make_trainer
    from heterofusionrcnn_amd.two_stage import TwoStageDetector
    from test_rcnn_train import rcnn_scene
    assert os.path.realpath(heterofusionrcnn_amd.__file__).startswith(os.path.realpath(tree))
    res = {"tree": tree}
    b = 2
    inputs = rcnn_scene(b, 7)
    inputs["img_fts"] = torch.rand(b, bench.IMG_H, bench.IMG_W, 3, device="cuda") * 255.0
    for graph in (False, True):
        key = "train_step_ms_%s" % ("replayed" if graph else "eager")
        try:
            torch.manual_seed(0)
            tr = make_trainer(288, seed=0)
            step = TrainStep(tr, MultiTensorAdam(tr.parameters(), lr=1e-3), inputs, None, graph=graph, loss_fn=RT.rcnn_train_loss)
            for _ in range(3):
                step()
            res[key] = percentiles([timed(step, 1) for _ in range(steps)])
            del step, tr
        except Exception as e:        # recorded, not hidden: the figure is then missing from the file
            res[key] = "failed: %r" % (e,)
        torch.cuda.empty_cache()
    del inputs
    torch.manual_seed(3)
    det = TwoStageDetector().cuda().eval()
    rng = np.random.default_rng(3)
    xyz = torch.from_numpy(bench.kitti_frustum(rng, b, bench.N0)).cuda()
    inten = torch.from_numpy(rng.uniform(-0.5, 0.5, (b, bench.N0, 1)).astype(np.float32)).cuda()
    img = torch.randn(b, bench.IMG_H, bench.IMG_W, bench.IMG_C, device="cuda")
    calib = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
    run = lambda: det(xyz, inten, img, calib)
    for _ in range(3):
        run()
    res["detect_batch_ms"] = percentiles([timed(run, 1) for _ in range(steps)])
    print("END_TO_END " + json.dumps(res))


def end_to_end(spec, steps, rounds):
    trees = [t.split("=") for t in spec.split(",")]
    out = {label: [] for _, label in trees}
    for _ in range(rounds):
        for tree, label in trees:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(tree), "--steps", str(steps)],
                               capture_output=True, text=True, timeout=900)
            lines = [ln for ln in p.stdout.splitlines() if ln.startswith("END_TO_END ")]
            if p.returncode != 0 or not lines:
                raise RuntimeError("end-to-end child for %s failed:\n%s\n%s" % (tree, p.stdout[-2000:], p.stderr[-4000:]))
            r = json.loads(lines[-1][len("END_TO_END "):])
            r.pop("tree")
            out[label].append(r)
            print("end-to-end %s: %s" % (label, json.dumps(r)), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_image_timing.json"))
    ap.add_argument("--end-to-end", default="")
    ap.add_argument("--rounds", type=int, default=2, help="how often every tree of --end-to-end is visited")
    ap.add_argument("--child", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "a timing needs the GPU"
    if args.child:
        end_to_end_child(args.child, args.steps)
        return
    assert args.reps >= 50
    res = {"what": "RoI image pooling (projection + crop_and_resize 7x7) on a (B,%d,%d,%d) fp32 map: hf_roi_image_boxes + "
                   "hf_crop_and_resize[_grad] against the tensor form, alternating in one process" % (H, W, C),
           "device": torch.cuda.get_device_name(0), "shapes": ab(args.reps)}
    res["accepted"] = all(s[k]["wins"] for s in res["shapes"].values() for k in ("forward", "forward_backward"))

    def write():
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")

    write()
    print(json.dumps(res), flush=True)
    if args.end_to_end:
        res["end_to_end_batch2"] = end_to_end(args.end_to_end, args.steps, args.rounds)
        write()


if __name__ == "__main__":
    main()
