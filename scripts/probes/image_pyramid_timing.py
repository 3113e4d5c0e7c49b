"""The image pyramid (inference.ImgVggPyr, full size) in eval mode at (8, 360, 1200, 3), the default route on the vendor library
against image_pyramid.image_branch("native"):
  torch_alone   the default route, WARMUP calls (the vendor library's first-call search stays outside), then REPS calls timed by events
  alternating   the two routes in turn in one process, REPS rounds, each call between its own pair of events: median and p10-p90
  launches      the native route launch by launch (an event pair around every C-ABI call, REPS passes, the median of each), with the
                TFLOP/s of each and of the whole against the 5.1 ms the forward's 0.80 TFLOP take at the 157 TFLOP/s fp32 MFMA peak
  detect        detect.detect frames/s over the committed KITTI frames repeated to 64 names (detect_timing.dataset), for either
                setting, ONE PROCESS EACH, alternating twice (torch, native, torch, native): one warm-up pass, then PASSES passes
Prints JSON lines and, when a path is given, writes the result there (profiles/image_pyramid_timing.json is such a file)."""
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from heterofusionrcnn_amd import image_pyramid  # noqa: E402
from heterofusionrcnn_amd.inference import ImgVggPyr  # noqa: E402

SHAPE, WARMUP, REPS, PASSES = (8, 360, 1200, 3), 5, 30, 3
PEAK_TFLOPS = 157.0


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
    """the library with an event pair around the three image entry points: (name, flop, start, end) per call"""

    def __init__(self, lib):
        self.lib, self.calls = lib, []

    def __getattr__(self, name):
        fn = getattr(self.lib, name)
        if name not in ("hf_conv3x3_nhwc", "hf_upconv3x3s2_nhwc", "hf_maxpool2x2_nhwc"):
            return fn

        def call(*args):
            b, h, w, cin, cout = args[:5]
            flop = 0 if name == "hf_maxpool2x2_nhwc" else 2.0 * b * h * w * 9 * cin * cout      # the up-convolution: real taps
            what = "%s %dx%dx%d %d->%d" % (name[3:], b, h, w, cin, cout) if flop else "%s %dx%dx%d c%d" % (name[3:], b, h, w, cin)
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            status = fn(*args)
            e.record()
            self.calls.append((what, flop, s, e))
            return status
        return call


def launches(net, image):
    real = image_pyramid._lib.lib
    proxy = TimedLib(real())
    image_pyramid._lib.lib = lambda: proxy
    try:
        per = None
        for _ in range(REPS):
            proxy.calls = []
            net(image)
            torch.cuda.synchronize()
            ms = [s.elapsed_time(e) for _, _, s, e in proxy.calls]
            per = [[m] for m in ms] if per is None else [p + [m] for p, m in zip(per, ms)]
        rows = []
        for (what, flop, _, _), ms in zip(proxy.calls, per):
            med = statistics.median(ms)
            rows.append({"launch": what, "median_ms": med, "gflop": flop / 1e9, "tflops": flop / med / 1e9 if flop else None})
        return rows
    finally:
        image_pyramid._lib.lib = real


def pyramid(res):
    torch.manual_seed(0)
    net = ImgVggPyr().cuda().eval()
    image = torch.empty(SHAPE, device="cuda").uniform_(0.0, 255.0)
    with torch.no_grad():
        for _ in range(WARMUP):
            net(image)
        torch.cuda.synchronize()
        res["torch_alone"] = spread([timed(lambda: net(image)) for _ in range(REPS)])
        print(json.dumps({"torch_alone": res["torch_alone"]}), flush=True)
        with image_pyramid.image_branch("native"):
            for _ in range(WARMUP):
                out = net(image)
        ref = net(image)
        res["max_abs_difference"] = float((out - ref).abs().max())
        res["max_abs_output"] = float(ref.abs().max())
        del out, ref
        t_ms, n_ms = [], []
        for _ in range(REPS):
            t_ms.append(timed(lambda: net(image)))
            with image_pyramid.image_branch("native"):
                n_ms.append(timed(lambda: net(image)))
        res["alternating"] = {"torch": spread(t_ms), "native": spread(n_ms)}
        print(json.dumps({"alternating": res["alternating"]}), flush=True)
        with image_pyramid.image_branch("native"):
            rows = launches(net, image)
    flop = sum(r["gflop"] for r in rows) * 1e9
    total = sum(r["median_ms"] for r in rows)
    res["launches"] = {"rows": rows, "count": len(rows), "sum_of_medians_ms": total, "gflop": flop / 1e9,
                       "tflops": flop / total / 1e9, "floor_ms_at_peak": flop / PEAK_TFLOPS / 1e9,
                       "fraction_of_fp32_mfma_peak": flop / total / 1e9 / PEAK_TFLOPS}
    print(json.dumps({"launches": res["launches"]}), flush=True)


def detect_child(mode):
    import detect_timing as DT
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    from heterofusionrcnn_amd.detect import detect, rpn_fts_channels
    torch.manual_seed(0)
    net, _ = train_rpn.make_model("rpn_multiclass")
    trainer = train_rcnn.make_trainer(rpn_fts_channels(net.rpn))
    with tempfile.TemporaryDirectory() as tmp:
        DT.dataset(tmp)
        times = []
        for i in range(PASSES + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            written = detect(tmp, net, trainer, os.path.join(tmp, "out"), split="val", batch=DT.BATCH, workers=DT.WORKERS,
                             score_threshold=0.0, image_branch=mode)
            torch.cuda.synchronize()
            if i > 0:
                times.append(time.perf_counter() - t0)
    print(json.dumps({"image_branch": mode, "seconds": times, "frames": DT.N, "frames_per_s": DT.N / statistics.median(times),
                      "rows_written": sum(written.values())}), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--detect-child":
        return detect_child(sys.argv[2])
    path = sys.argv[1] if len(sys.argv) > 1 else None
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "warmup": WARMUP, "reps": REPS}
    pyramid(res)
    torch.cuda.empty_cache()
    res["detect"] = []
    for mode in ("torch", "native", "torch", "native"):          # a fresh process each: neither route inherits the other's state
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--detect-child", mode],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-4000:], flush=True)
            raise SystemExit("the detect pass with image_branch=%s ended with status %d" % (mode, r.returncode))
        res["detect"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({"detect": res["detect"][-1]}), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
