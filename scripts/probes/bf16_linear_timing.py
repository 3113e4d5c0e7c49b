"""The bf16 inference route against the fp32 one, stage by stage; results are merged into the JSON file given as the first argument
(profiles/bf16_inference_timing.json is such a file).  python scripts/probes/bf16_linear_timing.py OUT.json [kernels] [two_stage] [detect]

kernels    every GEMM shape of profiles/r04_two_stage_gemm_shapes.txt with cin >= 32, three routes alternated in one process, REPS
           rounds of ITERS back-to-back calls between two events:
             fp32_library   the library fp32 GEMM + the eval BatchNorm pass it needs (hf_bn_relu_fwd_eval, ELU on load): today's route
             bf16_library   the library's own bf16 GEMM with the cast pass it needs (x.to(bfloat16) @ w_bf16.T, fp32 out) + the BatchNorm pass
             bf16_kernel    hf_linear_bf16_fwd_eval, BatchNorm in the epilogue
           and "routing": the shapes where bf16_kernel beat fp32_library by more than the spread (max - min over the rounds) of the
           latter -- what mlp.bf16_route_pays has to reproduce.
two_stage  two-stage inference per batch of 8 at rcnn_multiclass.config's own sizes (bench.py's inputs), fp32 and bf16 detectors with
           the same weights alternated, plain and with the geometry computed ahead; and the drift of the head outputs.
detect     detect.detect frames/s on the committed frames both ways (the dataset of scripts/probes/detect_timing.py), and the share of
           fp32 result rows that have a bf16 row of the same class at BEV IoU > 0.9 on the four committed frames (untrained weights)."""
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from heterofusionrcnn_amd import _lib, mlp  # noqa: E402

REPS = 5


def shapes():
    out = []
    with open(os.path.join(ROOT, "profiles", "r04_two_stage_gemm_shapes.txt")) as f:
        for line in f:
            m = re.match(r"mm\s+\(\((\d+), (\d+)\), \((\d+), (\d+)\)\)\s+x(\d+)\s+(\d+) us", line)
            if m and int(m.group(2)) >= 32:
                out.append(dict(rows=int(m.group(1)), cin=int(m.group(2)), cout=int(m.group(4)), calls=int(m.group(5)),
                                r04_us_total=int(m.group(6))))
    return out


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / iters


def kernels():
    L = _lib.lib()
    ptr, sp = _lib.ptr, _lib.stream_ptr
    res = []
    for s in shapes():
        rows, cin, cout = s["rows"], s["cin"], s["cout"]
        g = torch.Generator(device="cuda").manual_seed(rows + cin + cout)
        x = torch.randn(rows, cin, device="cuda", generator=g)
        w = torch.randn(cout, cin, device="cuda", generator=g) * cin ** -0.5
        gamma, beta, mean = (torch.randn(cout, device="cuda", generator=g) for _ in range(3))
        invstd = torch.rand(cout, device="cuda", generator=g) + 0.5
        wb = torch.empty(cout, cin, dtype=torch.bfloat16, device="cuda")
        _lib.check(L.hf_f32_to_bf16(w.numel(), ptr(w), ptr(wb), sp()), "f32_to_bf16")
        assert torch.equal(wb, w.to(torch.bfloat16))
        y = torch.empty(rows, cout, device="cuda")
        wt, wbt = w.t(), wb.t()

        def bn(z):
            _lib.check(L.hf_bn_relu_fwd_eval(rows, cout, ptr(z), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd), 2, ptr(y), sp()), "bn")

        routes = {
            "fp32_library": lambda: bn(x @ wt),
            "bf16_library": lambda: bn((x.to(torch.bfloat16) @ wbt).float()),
            "bf16_kernel": lambda: _lib.check(L.hf_linear_bf16_fwd_eval(rows, cin, cout, ptr(x), ptr(wb), None, ptr(gamma), ptr(beta), ptr(mean),
                                                                        ptr(invstd), 2, ptr(y), sp()), "linear_bf16"),
        }
        iters = 3 if rows * cin * cout > 1e11 else 10
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in routes}
        for _ in range(REPS):
            for k, fn in routes.items():
                times[k].append(timed(fn, iters))
        row = dict(s)
        for k, v in times.items():
            row[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
        a, c = row["fp32_library_us"], row["bf16_kernel_us"]
        row["fp32_spread_us"] = round(a["max"] - a["min"], 1)
        row["kernel_beats_fp32_beyond_spread"] = bool(a["median"] - c["median"] > row["fp32_spread_us"])
        row["bf16_kernel_tflops"] = round(2.0 * rows * cin * cout / (c["median"] * 1e-6) / 1e12, 1)
        res.append(row)
        print(json.dumps(row), flush=True)
        del x, w, y, wb
        torch.cuda.empty_cache()
    return {"reps": REPS, "shapes": res,
            "routing": {"takes_kernel": [[r["rows"], r["cin"], r["cout"]] for r in res if r["kernel_beats_fp32_beyond_spread"]],
                        "stays_fp32": [[r["rows"], r["cin"], r["cout"]] for r in res if not r["kernel_beats_fp32_beyond_spread"]],
                        "predicate_agrees": all(mlp.bf16_route_pays(r["rows"], r["cin"], r["cout"]) == r["kernel_beats_fp32_beyond_spread"]
                                                for r in res),
                        "constants": {"BF16_MIN_ROWS": mlp.BF16_MIN_ROWS, "BF16_MIN_CIN": mlp.BF16_MIN_CIN,
                                      "BF16_MIN_COUT": mlp.BF16_MIN_COUT}}}


def two_stage():
    import bench
    from heterofusionrcnn_amd.pipeline import GeometryPrefetcher
    from heterofusionrcnn_amd.two_stage import TwoStageDetector
    B = 8
    torch.manual_seed(0)
    det32 = TwoStageDetector().cuda().eval()
    det16 = TwoStageDetector(precision="bf16").cuda().eval()
    det16.load_state_dict(det32.state_dict())
    fx = torch.from_numpy(bench.kitti_frustum(np.random.default_rng(7), B, bench.N0)).cuda()
    inten = torch.from_numpy(np.random.default_rng(8).uniform(-0.5, 0.5, (B, bench.N0, 1)).astype(np.float32)).cuda()
    img = torch.randn(B, bench.IMG_H, bench.IMG_W, bench.IMG_C, device="cuda")
    cal = torch.from_numpy(bench.KITTI_P2).cuda().repeat(B, 1, 1).contiguous()
    out = {"batch": B}
    before = mlp.BF16_ROUTED_CALLS[0]
    _, dbg16 = det16(fx, inten, img, cal, return_debug=True)
    out["bf16_kernel_launches_per_batch"] = mlp.BF16_ROUTED_CALLS[0] - before
    _, dbg32 = det32(fx, inten, img, cal, return_debug=True)
    # drift of the second stage alone: both detectors' RCNN on the fp32 first stage's hand-off
    r = dbg32["rpn"]
    args = (fx, r["rpn_fts"], inten, r["fg_mask"], r["proposals"], img, cal)
    with torch.no_grad():
        c32, g32, _ = det32.rcnn(*args)
        with mlp.inference_precision("bf16"):
            c16, g16, _ = det32.rcnn(*args)
    out["rcnn_head_drift_untrained"] = {"max_abs_d_cls_logits": float((c16 - c32).abs().max()), "max_abs_cls_logits": float(c32.abs().max()),
                                        "max_abs_d_reg": float((g16 - g32).abs().max()), "max_abs_reg": float(g32.abs().max())}
    plain = {"fp32": [], "bf16": []}
    for _ in range(REPS):
        for name, det in (("fp32", det32), ("bf16", det16)):
            plain[name].append(timed(lambda: det(fx, inten, img, cal), 3) / 1e3)
    piped = {"fp32": [], "bf16": []}
    for name, det in (("fp32", det32), ("bf16", det16)):
        pf = GeometryPrefetcher(det.geometry, depth=2)
        pf.submit(fx)
        pf.submit(fx)

        def step():
            geo = pf.get()
            pf.submit(fx)
            det(fx, inten, img, cal, geometry=geo)
        step()
        for _ in range(REPS):
            piped[name].append(timed(step, 4) / 1e3)
        pf.get()
        pf.get()
    for key, d in (("ms_per_batch", plain), ("pipelined_ms_per_batch", piped)):
        out[key] = {k: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in d.items()}
    print(json.dumps(out), flush=True)
    return out


def _matched_share(dir32, dir16, names):
    from heterofusionrcnn_amd import compute_bev_iou, kitti_io, modules
    rows = matched = rows16 = 0
    for n in names:
        t32, b32, _, _ = kitti_io.read_labels(os.path.join(dir32, n + ".txt"))
        t16, b16, _, _ = kitti_io.read_labels(os.path.join(dir16, n + ".txt"))
        rows, rows16 = rows + len(t32), rows16 + len(t16)
        if not len(t32) or not len(t16):
            continue
        a = modules.boxes3d_to_bev(torch.as_tensor(np.asarray(b32, np.float32)).cuda()).contiguous()
        b = modules.boxes3d_to_bev(torch.as_tensor(np.asarray(b16, np.float32)).cuda()).contiguous()
        _, iou = compute_bev_iou(a, b)
        same = torch.tensor([[x == y for y in t16] for x in t32], device="cuda")
        matched += int(((iou > 0.9) & same).any(dim=1).sum())
    return {"fp32_rows": rows, "bf16_rows": rows16, "fp32_rows_matched_at_bev_iou_0.9": matched, "share": matched / max(rows, 1)}


def detect_stage():
    import detect_timing as DT
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    from heterofusionrcnn_amd.detect import detect, rpn_fts_channels
    torch.manual_seed(0)
    net, _ = train_rpn.make_model("rpn_multiclass")
    trainer = train_rcnn.make_trainer(rpn_fts_channels(net.rpn))
    out = {"frames": DT.N, "batch": DT.BATCH, "note": "untrained weights: scores and boxes carry no meaning beyond being outputs of the same functions"}
    with tempfile.TemporaryDirectory() as tmp:
        DT.dataset(tmp)
        kw = dict(split="val", batch=DT.BATCH, workers=DT.WORKERS, score_threshold=0.0)
        dirs = {p: os.path.join(tmp, "out_" + p) for p in ("fp32", "bf16")}
        secs = {"fp32": [], "bf16": []}
        for p in dirs:
            detect(tmp, net, trainer, dirs[p], precision=p, **kw)       # warm-up pass
        for _ in range(3):
            for p in dirs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                detect(tmp, net, trainer, dirs[p], precision=p, **kw)
                torch.cuda.synchronize()
                secs[p].append(time.perf_counter() - t0)
        out["frames_per_s"] = {p: round(DT.N / statistics.median(v), 2) for p, v in secs.items()}
        out["seconds"] = {p: [round(s, 3) for s in v] for p, v in secs.items()}
        out["committed_frames_match"] = _matched_share(dirs["fp32"], dirs["bf16"], ["%06d" % i for i in range(len(DT.GOLD))])
    print(json.dumps(out), flush=True)
    return out


def main():
    path = sys.argv[1]
    stages = sys.argv[2:] or ["kernels", "two_stage", "detect"]
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    for name, fn in (("kernels", kernels), ("two_stage", two_stage), ("detect", detect_stage)):
        if name in stages:
            res[name] = fn()
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
