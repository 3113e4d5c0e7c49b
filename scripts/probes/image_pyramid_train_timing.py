"""The image pyramid (inference.ImgVggPyr, shipped widths) in training mode, forward plus backward at (8, 360, 1200, 3): the default
route on the vendor library against image_pyramid.train_branch("native"):
  alternating   the two routes in turn in one process after WARMUP steps of each (the vendor library's first-call search stays
                outside), REPS rounds, each step between its own pair of events: median and p10-p90
  phases        the native route call by call (an event pair around every C-ABI call, REPS steps, the median of each), summed per
                phase: forward convolutions, BatchNorm passes, wgrad, dgrad, pool; what is left of the step (the weight permutes, the
                running-statistics update, allocation) is "other".  Every wgrad launch with its TFLOP/s against the 157 TFLOP/s fp32
                MFMA peak
  steps         with --steps: the train_rpn step with the pyramid (rpn_multiclass, batch 8, captured) on bench.py's synthetic frames, ONE
                PROCESS PER SETTING, alternating twice (torch, native, torch, native).  The train_rcnn step is not measured here
Prints JSON lines and, when a path is given, writes the result there (profiles/image_pyramid_train_timing.json is such a file)."""
import json
import os
import statistics
import subprocess
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from heterofusionrcnn_amd import image_pyramid  # noqa: E402
from heterofusionrcnn_amd.inference import ImgVggPyr  # noqa: E402

SHAPE, WARMUP, REPS = (8, 360, 1200, 3), 3, 30
PEAK_TFLOPS = 157.0
PHASES = {"hf_bn_relu_fwd_train_ld": "batchnorm", "hf_bn_relu_bwd_ld": "batchnorm", "hf_conv3x3_nhwc_wgrad": "wgrad",
          "hf_upconv3x3s2_nhwc_wgrad": "wgrad", "hf_conv3x3s2_nhwc": "dgrad", "hf_maxpool2x2_nhwc": "pool", "hf_maxpool2x2_nhwc_bwd": "pool"}


def spread(ms):
    q = statistics.quantiles(ms, n=10)
    return {"median_ms": statistics.median(ms), "p10_ms": q[0], "p90_ms": q[-1], "n": len(ms)}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class TimedLib:
    """the library with an event pair around every kernel entry point of the training route: (phase, what, flop, start, end) per call"""

    def __init__(self, lib):
        self.lib, self.calls, self.backward = lib, [], False

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in PHASES and name not in ("hf_conv3x3_nhwc", "hf_upconv3x3s2_nhwc"):
            return fn

        def call(*args):
            phase = PHASES.get(name) or ("dgrad" if self.backward else "forward convolutions")
            flop, what = 0.0, name[3:]
            if phase in ("wgrad", "dgrad", "forward convolutions"):
                b, h, w, cin, cout = args[:5]
                flop = 2.0 * b * h * w * 9 * cin * cout
                what = "%s %dx%dx%d %d->%d" % (name[3:], b, h, w, cin, cout)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            status = fn(*args)
            e.record()
            self.calls.append((phase, what, flop, s, e))
            return status
        return call


def step(net, image, cot, proxy=None):
    for p in net.parameters():
        p.grad = None
    out = net(image)
    if proxy is not None:
        proxy.backward = True
    out.backward(cot)
    if proxy is not None:
        proxy.backward = False


def phases(net, image, cot):
    real = image_pyramid._lib.lib
    proxy = TimedLib(real())
    image_pyramid._lib.lib = lambda: proxy
    real_dense, image_pyramid._dense_kernels.lib = image_pyramid._dense_kernels.lib, lambda: proxy      # the BatchNorm launch site
    try:
        per, totals = None, []
        for _ in range(REPS):
            proxy.calls = []
            totals.append(timed(lambda: step(net, image, cot, proxy)))
            ms = [s.elapsed_time(e) for _, _, _, s, e in proxy.calls]
            per = [[m] for m in ms] if per is None else [p + [m] for p, m in zip(per, ms)]
        by_phase, wgrad = {}, []
        for (phase, what, flop, _, _), ms in zip(proxy.calls, per):
            med = statistics.median(ms)
            d = by_phase.setdefault(phase, {"ms": 0.0, "gflop": 0.0, "launches": 0})
            d["ms"] += med
            d["gflop"] += flop / 1e9
            d["launches"] += 1
            if phase == "wgrad":
                wgrad.append({"launch": what, "median_ms": med, "gflop": flop / 1e9, "tflops": flop / med / 1e9,
                              "fraction_of_fp32_mfma_peak": flop / med / 1e9 / PEAK_TFLOPS})
        for d in by_phase.values():
            d["tflops"] = d["gflop"] / d["ms"] if d["gflop"] else None
        step_ms = statistics.median(totals)        # with the event pairs inside: a little above the alternating median
        return {"step_with_events_ms": step_ms, "by_phase": by_phase, "other_ms": step_ms - sum(d["ms"] for d in by_phase.values()),
                "wgrad_launches": wgrad}
    finally:
        image_pyramid._lib.lib = real
        image_pyramid._dense_kernels.lib = real_dense


def pyramid(res):
    torch.manual_seed(0)
    net = ImgVggPyr().cuda().train()
    image = torch.empty(SHAPE, device="cuda").uniform_(0.0, 255.0)
    cot = torch.randn(SHAPE[:3] + (net.out_channel,), device="cuda")
    for _ in range(WARMUP):
        step(net, image, cot)
    ref = [p.grad.clone() for p in net.parameters()]
    with image_pyramid.train_branch("native"):
        for _ in range(WARMUP):
            step(net, image, cot)
    res["max_relative_gradient_difference"] = max(float((p.grad - r).abs().max() / r.abs().max().clamp(min=1e-30))
                                                  for p, r in zip(net.parameters(), ref))
    del ref
    torch.cuda.synchronize()
    t_ms, n_ms = [], []
    for _ in range(REPS):
        t_ms.append(timed(lambda: step(net, image, cot)))
        with image_pyramid.train_branch("native"):
            n_ms.append(timed(lambda: step(net, image, cot)))
    res["alternating"] = {"torch": spread(t_ms), "native": spread(n_ms)}
    print(json.dumps({"alternating": res["alternating"], "max_relative_gradient_difference": res["max_relative_gradient_difference"]}),
          flush=True)
    with image_pyramid.train_branch("native"):
        res["phases"] = phases(net, image, cot)
    print(json.dumps({"phases": res["phases"]}), flush=True)


def rpn_step():
    """the rpn_multiclass train step with the pyramid in front, batch 8, on bench.py's synthetic frames, captured as train_rpn runs it"""
    import numpy as np
    import bench
    from heterofusionrcnn_amd import rpn as rpn_mod
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    rng, b, n = np.random.default_rng(0), SHAPE[0], 16384
    torch.manual_seed(0)
    xyz = torch.from_numpy(bench.kitti_frustum(rng, b, n)).cuda()
    inputs = {"xyz": xyz, "intensity": torch.from_numpy(rng.uniform(-0.5, 0.5, (b, n, 1)).astype(np.float32)).cuda()}
    cfg = rpn_mod.rpn_multiclass(32)
    gt_boxes, gt_cls = rpn_mod.synthetic_ground_truth(rng, b, 12, cfg, ground_y=3.0)
    inputs["label_cls"], inputs["label_reg"] = rpn_mod.point_labels(xyz, torch.from_numpy(gt_boxes).cuda(), torch.from_numpy(gt_cls).cuda())
    inputs["img_fts"] = torch.rand(SHAPE, device="cuda") * 255.0
    inputs["calib"] = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
    model = rpn_mod.RpnWithImageBranch(rpn_mod.RpnModel(cfg).cuda(), ImgVggPyr().cuda()).cuda()
    geo = model.geometry(xyz)
    train = TrainStep(model, MultiTensorAdam(list(model.parameters()), lr=1e-3, tf_epsilon=False), inputs, geo, graph=True)
    return lambda: train(geometry=geo)


def step_child(mode):
    """one process: the whole train step on synthetic inputs, WARMUP + REPS steps"""
    with image_pyramid.train_branch(mode):
        run = rpn_step()
        for _ in range(WARMUP):
            run()
        torch.cuda.synchronize()
        ms = [timed(run) for _ in range(REPS)]
    print(json.dumps(dict(stage="train_rpn step, rpn_multiclass with the pyramid, batch %d, captured" % SHAPE[0], image_train_branch=mode,
                          **spread(ms))), flush=True)


def main():
    args = [a for a in sys.argv[1:] if a != "--steps"]
    if len(args) > 1 and args[0] == "--step-child":
        return step_child(args[1])
    path = args[0] if args else None
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "warmup": WARMUP, "reps": REPS}
    pyramid(res)
    torch.cuda.empty_cache()
    if "--steps" in sys.argv:
        res["steps"] = []
        for mode in ("torch", "native", "torch", "native"):          # a fresh process each: neither route inherits the other's state
            r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--step-child", mode],
                               capture_output=True, text=True)
            if r.returncode != 0:
                print(r.stdout[-2000:] + r.stderr[-4000:], flush=True)
                raise SystemExit("the step with image_train_branch=%s ended with status %d" % (mode, r.returncode))
            res["steps"].append(json.loads(r.stdout.strip().splitlines()[-1]))
            print(json.dumps({"step": res["steps"][-1]}), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
