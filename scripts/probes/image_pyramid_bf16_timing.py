"""The image pyramid (inference.ImgVggPyr, full size) in eval mode at (8, 360, 1200, 3) on its three routes: the vendor library, the
fp32 kernels of csrc/conv_nhwc.hip (image_branch("native")) and the bf16 kernels of csrc/conv_nhwc_bf16.hip (plus
image_precision("bf16")):
  alternating   the three routes in turn in one process, REPS rounds after WARMUP calls each, every call between its own pair of
                events: median and p10-p90.  The baseline of the bf16 route is the fp32 native route of this same run.  A fourth
                column sets image_pyramid.bf16_conv_pays aside and runs all sixteen convolutions in bf16
  layers        each of the sixteen convolution launches at its production shape, fp32 native against bf16, alternating, REPS rounds:
                median, p10-p90, TFLOP/s and bytes/s (input + output + weights, each counted once) of either; the constants of
                image_pyramid.bf16_conv_pays come from this table
  drift         max |bf16 feature map - fp32 native feature map| and the maximum of the fp32 map on the seeded, untrained model:
                reported, not asserted
  detect        detect.detect frames/s over the committed KITTI frames repeated to 64 names (detect_timing.dataset) with
                precision="bf16", image_branch="native", with and without image_precision="bf16", ONE PROCESS EACH, alternating twice:
                one warm-up pass, then PASSES passes
Prints JSON lines and, when a path is given, writes the result there (profiles/image_pyramid_bf16_timing.json is such a file)."""
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


def native(net, image, precision, every_layer=False):
    """every_layer: bf16_conv_pays set aside, all sixteen convolutions on the bf16 kernels"""
    pays = image_pyramid.bf16_conv_pays
    if every_layer:
        image_pyramid.bf16_conv_pays = lambda rows, cin, cout, up: True
    try:
        with image_pyramid.image_branch("native"), image_pyramid.image_precision(precision):
            return net(image)
    finally:
        image_pyramid.bf16_conv_pays = pays


def layer_table(net):
    """the sixteen convolution launches of forward_native at SHAPE, each on buffers of its own"""
    p = image_pyramid.pack(net)
    b, h, w, _ = SHAPE
    jobs = []
    for level, block in enumerate(p["blocks"]):
        for i, layer in enumerate(block):
            jobs.append(("conv%d_%d" % (level + 1, i), layer, h >> level, w >> level, p["mean"] if level == 0 and i == 0 else None))
    for level, up, fusion in zip((2, 1, 0), p["up"], p["fusion"]):
        jobs.append(("upconv%d" % (level + 1), up, h >> (level + 1), w >> (level + 1), None))
        jobs.append(("fusion%d" % (level + 1), fusion, h >> level, w >> level, None))
    rows = []
    for name, layer, hh, ww, sub in jobs:
        cin, cout, up = layer["cin"], layer["cout"], layer["up"]
        x = torch.empty((b, hh, ww, cin), device="cuda").uniform_(0.0, 2.0)
        y = torch.empty((b, 2 * hh, 2 * ww, cout) if up else (b, hh, ww, cout), device="cuda")
        for _ in range(3):
            image_pyramid._conv(layer, x, y, 0, sub, False)
            image_pyramid._conv(layer, x, y, 0, sub, True)
        torch.cuda.synchronize()
        f_ms, b_ms = [], []
        for _ in range(REPS):
            f_ms.append(timed(lambda: image_pyramid._conv(layer, x, y, 0, sub, False)))
            b_ms.append(timed(lambda: image_pyramid._conv(layer, x, y, 0, sub, True)))
        flop = 2.0 * b * hh * ww * 9 * cin * cout                       # the up-convolution: real taps only
        nbytes = 4.0 * (x.numel() + y.numel())
        row = {"layer": name, "shape": [b, hh, ww, cin, cout], "up": up, "gflop": flop / 1e9}
        for key, ms, wbytes in (("fp32", f_ms, 4.0 * layer["wt"].numel()), ("bf16", b_ms, 2.0 * layer["wt"].numel())):
            s = spread(ms)
            s.update(tflops=flop / s["median_ms"] / 1e9, gbytes_per_s=(nbytes + wbytes) / s["median_ms"] / 1e6)
            row[key] = s
        row["speedup"] = row["fp32"]["median_ms"] / row["bf16"]["median_ms"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y
    return rows


def pyramid(res):
    torch.manual_seed(0)
    net = ImgVggPyr().cuda().eval()
    image = torch.empty(SHAPE, device="cuda").uniform_(0.0, 255.0)
    with torch.no_grad():
        for _ in range(WARMUP):
            net(image)
            f32 = native(net, image, "fp32")
            b16 = native(net, image, "bf16")
            native(net, image, "bf16", True)
        torch.cuda.synchronize()
        res["drift"] = {"max_abs_bf16_minus_fp32_native": float((b16 - f32).abs().max()), "max_abs_fp32_native": float(f32.abs().max()),
                        "mean_abs_fp32_native": float(f32.abs().mean()), "note": "seeded, untrained weights: reported, not asserted"}
        print(json.dumps({"drift": res["drift"]}), flush=True)
        del f32, b16
        t_ms, f_ms, b_ms, a_ms = [], [], [], []
        for _ in range(REPS):
            t_ms.append(timed(lambda: net(image)))
            f_ms.append(timed(lambda: native(net, image, "fp32")))
            b_ms.append(timed(lambda: native(net, image, "bf16")))
            a_ms.append(timed(lambda: native(net, image, "bf16", True)))
        res["alternating"] = {"torch": spread(t_ms), "native_fp32": spread(f_ms), "native_bf16": spread(b_ms),
                              "native_bf16_every_layer": spread(a_ms)}
        print(json.dumps({"alternating": res["alternating"]}), flush=True)
        rows = layer_table(net)
    res["layers"] = {"rows": rows, "fp32_sum_of_medians_ms": sum(r["fp32"]["median_ms"] for r in rows),
                     "bf16_sum_of_medians_ms": sum(r["bf16"]["median_ms"] for r in rows), "gflop": sum(r["gflop"] for r in rows)}


def detect_child(image_precision):
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
                             score_threshold=0.0, precision="bf16", image_branch="native", image_precision=image_precision)
            torch.cuda.synchronize()
            if i > 0:
                times.append(time.perf_counter() - t0)
    print(json.dumps({"precision": "bf16", "image_branch": "native", "image_precision": image_precision, "seconds": times, "frames": DT.N,
                      "frames_per_s": DT.N / statistics.median(times), "rows_written": sum(written.values())}), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--detect-child":
        return detect_child(sys.argv[2])
    path = sys.argv[1] if len(sys.argv) > 1 else None
    res = {"device": torch.cuda.get_device_name(0), "shape": list(SHAPE), "warmup": WARMUP, "reps": REPS}

    def save():
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)

    pyramid(res)
    save()                                                       # the detect passes below add to the file
    torch.cuda.empty_cache()
    res["detect"] = []
    for mode in ("fp32", "bf16", "fp32", "bf16"):                # a fresh process each: neither setting inherits the other's state
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--detect-child", mode],
                           capture_output=True, text=True)
        if r.returncode != 0:
            print(r.stdout[-2000:] + r.stderr[-4000:], flush=True)
            raise SystemExit("the detect pass with image_precision=%s ended with status %d" % (mode, r.returncode))
        res["detect"].append(json.loads(r.stdout.strip().splitlines()[-1]))
        print(json.dumps({"detect": res["detect"][-1]}), flush=True)
    save()


if __name__ == "__main__":
    main()
