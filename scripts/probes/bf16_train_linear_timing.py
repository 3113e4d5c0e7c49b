"""The bf16 training route against the fp32 one; results are merged into the JSON file given as the first argument
(profiles/bf16_training_timing.json is such a file).  python scripts/probes/bf16_train_linear_timing.py OUT.json [layers] [step]

layers  the wide-layer shapes (every linear_nobias call whose layer allows bf16, cin >= 32) of the rpn_multiclass train step at batch 8
        and at one frame and of the RCNN step at batch 2, recorded from one forward pass of each model.  Per shape the three products
        of a layer, both routes alternated in one process, REPS rounds of ITERS back-to-back calls between two events:
          fp32   z = x W^T as linear_nobias computes it today, dx = g W (library), dW = mlp._splitk_wgrad
          bf16   the two weight conversions + hf_linear_bf16_fwd_eval, dx through the transposed weight, hf_linear_bf16_wgrad
        and "routing": the shapes where the summed bf16 trio beat the summed fp32 trio by more than the spread (max - min over the
        rounds) of the latter -- mlp.bf16_train_route_pays may route nothing else ("predicate_routes_only_winners").
step    the whole train_rpn-shaped step (rpn_multiclass at full width, batch 8, synthetic inputs of bench.py, MultiTensorAdam), captured
        and replayed, at both precisions alternated in one process.
Keys of OUT.json that no stage writes are carried over: "wgrad_staging" of profiles/bf16_training_timing.json is such a record."""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from heterofusionrcnn_amd import _lib, mlp, pointcnn  # noqa: E402

REPS = 5


def timed(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return 1e3 * start.elapsed_time(end) / iters


def _summary(v):
    return {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}


def rpn_inputs(b):
    import bench
    from heterofusionrcnn_amd import rpn as R_
    cfg = R_.rpn_multiclass(bench.IMG_C)
    rng = np.random.default_rng(11)
    xyz = torch.from_numpy(bench.kitti_frustum(rng, b, bench.N0)).cuda()
    inp = {"xyz": xyz, "intensity": torch.from_numpy(rng.uniform(-0.5, 0.5, (b, bench.N0, 1)).astype(np.float32)).cuda()}
    boxes, cls = R_.synthetic_ground_truth(rng, b, 12, cfg, ground_y=3.0)
    inp["label_cls"], inp["label_reg"] = R_.point_labels(xyz, torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda())
    inp["img_fts"] = torch.randn(b, bench.IMG_H, bench.IMG_W, bench.IMG_C, device="cuda")
    inp["calib"] = torch.from_numpy(bench.KITTI_P2).cuda().repeat(b, 1, 1).contiguous()
    return cfg, inp


def recorded_shapes():
    """{workload: {(rows, cin, cout): calls}} of the permitted linear_nobias calls of one training-mode forward pass"""
    from heterofusionrcnn_amd import rcnn_train as RT, rpn as R_
    from heterofusionrcnn_amd.rcnn import RcnnConfig, RcnnModel
    from test_rcnn_train import rcnn_scene
    real = pointcnn.linear_nobias
    seen = {}

    def recording(x, weight, allow_bf16=False):
        cout, cin = weight.shape
        if allow_bf16 and cin >= 32 and cin % 4 == 0 and cout % 4 == 0:
            key = (x.numel() // cin, cin, cout)
            seen[key] = seen.get(key, 0) + 1
        return real(x, weight, allow_bf16)

    out = {}
    pointcnn.linear_nobias = recording
    try:
        for b in (8, 1):
            seen = {}
            cfg, inp = rpn_inputs(b)
            torch.manual_seed(9)
            model = R_.RpnModel(cfg).cuda().train()
            model(inp["xyz"], inp["intensity"], geometry=model.geometry(inp["xyz"]), img_fts=inp["img_fts"], calib=inp["calib"])
            out["rpn_multiclass_b%d" % b] = seen
            del model, inp
            torch.cuda.empty_cache()
        seen = {}
        tr = RT.RcnnTrainer(RcnnModel(RcnnConfig()), seed=0).cuda().train()
        RT.rcnn_train_loss(tr, rcnn_scene(2, 7), None)
        out["rcnn_b2"] = seen
        del tr
        torch.cuda.empty_cache()
    finally:
        pointcnn.linear_nobias = real
    return out


def layers():
    L = _lib.lib()
    ptr, sp = _lib.ptr, _lib.stream_ptr
    per_workload = recorded_shapes()
    shapes = sorted({k for d in per_workload.values() for k in d})
    res = []
    for rows, cin, cout in shapes:
        gen = torch.Generator(device="cuda").manual_seed(rows + cin + cout)
        x = torch.randn(rows, cin, device="cuda", generator=gen)
        w = torch.randn(cout, cin, device="cuda", generator=gen) * cin ** -0.5
        g = torch.randn(rows, cout, device="cuda", generator=gen)
        wb = torch.empty(cout, cin, dtype=torch.bfloat16, device="cuda")
        wtb = torch.empty(cin, cout, dtype=torch.bfloat16, device="cuda")

        def convert():
            _lib.check(L.hf_f32_to_bf16(w.numel(), ptr(w), ptr(wb), sp()), "f32_to_bf16")
            _lib.check(L.hf_f32_to_bf16_transpose(cout, cin, ptr(w), ptr(wtb), sp()), "f32_to_bf16_transpose")

        def fwd16():
            convert()
            return mlp._bf16_gemm(rows, cin, cout, x, wb)

        tall = rows >= 2048          # linear_nobias: _LinearSplitK from 2048 rows, the library's linear below
        routes = {
            "fp32_fwd": (lambda: mlp._LinearSplitK.apply(x, w)) if tall else (lambda: torch.nn.functional.linear(x, w)),
            "fp32_dx": lambda: g @ w,
            "fp32_dw": (lambda: mlp._splitk_wgrad(g, x)) if tall else (lambda: g.t() @ x),
            "bf16_fwd": fwd16,
            "bf16_dx": lambda: mlp._bf16_gemm(rows, cout, cin, g, wtb),
            "bf16_dw": lambda: mlp.linear_bf16_wgrad(g, x),
        }
        with torch.no_grad():
            convert()
            assert torch.equal(wb, w.to(torch.bfloat16)) and torch.equal(wtb, w.t().contiguous().to(torch.bfloat16))
            iters = 3 if rows * cin * cout > 1e11 else 10
            for fn in routes.values():
                fn()
            torch.cuda.synchronize()
            times = {k: [] for k in routes}
            for _ in range(REPS):
                for k, fn in routes.items():
                    times[k].append(timed(fn, iters))
        row = {"rows": rows, "cin": cin, "cout": cout,
               "calls": {wl: d[(rows, cin, cout)] for wl, d in per_workload.items() if (rows, cin, cout) in d}}
        for k, v in times.items():
            row[k + "_us"] = _summary(v)
        for p in ("fp32", "bf16"):
            row[p + "_trio_us"] = _summary([sum(t) for t in zip(times[p + "_fwd"], times[p + "_dx"], times[p + "_dw"])])
        row["fp32_spread_us"] = round(row["fp32_trio_us"]["max"] - row["fp32_trio_us"]["min"], 1)
        row["bf16_beats_fp32_beyond_spread"] = bool(row["fp32_trio_us"]["median"] - row["bf16_trio_us"]["median"] > row["fp32_spread_us"])
        row["predicate_takes_bf16"] = bool(mlp.bf16_train_route_pays(rows, cin, cout))
        res.append(row)
        print(json.dumps(row), flush=True)
        del x, w, g
        torch.cuda.empty_cache()
    return {"reps": REPS, "shapes": res,
            "routing": {"takes_bf16": [[r["rows"], r["cin"], r["cout"]] for r in res if r["bf16_beats_fp32_beyond_spread"]],
                        "stays_fp32": [[r["rows"], r["cin"], r["cout"]] for r in res if not r["bf16_beats_fp32_beyond_spread"]],
                        "predicate_agrees": all(r["predicate_takes_bf16"] == r["bf16_beats_fp32_beyond_spread"] for r in res),
                        "predicate_routes_only_winners": all(r["bf16_beats_fp32_beyond_spread"] for r in res if r["predicate_takes_bf16"]),
                        "winners_left_fp32": [[r["rows"], r["cin"], r["cout"]] for r in res
                                              if r["bf16_beats_fp32_beyond_spread"] and not r["predicate_takes_bf16"]],
                        "constants": {"BF16_TRAIN_MIN_ROWS": mlp.BF16_TRAIN_MIN_ROWS, "BF16_TRAIN_MIN_CIN": mlp.BF16_TRAIN_MIN_CIN,
                                      "BF16_TRAIN_MIN_COUT": mlp.BF16_TRAIN_MIN_COUT}}}


def step():
    from heterofusionrcnn_amd import rpn as R_
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    B = 8
    cfg, inp = rpn_inputs(B)
    steps, routed, first = {}, {}, {}
    for p in ("fp32", "bf16"):
        torch.manual_seed(9)
        model = R_.RpnModel(cfg).cuda().train()
        geo = model.geometry(inp["xyz"])
        opt = MultiTensorAdam([q for q in model.parameters() if q.requires_grad], lr=1e-3)
        with mlp.training_precision(p):
            before = mlp.BF16_TRAIN_ROUTED_CALLS[0]
            s = TrainStep(model, opt, inp, geo, world=1, graph=True, warmup=2)
            routed[p] = mlp.BF16_TRAIN_ROUTED_CALLS[0] - before
        first[p] = [float(s(geometry=geo)) for _ in range(3)]
        steps[p] = (s, geo)
    ms = {"fp32": [], "bf16": []}
    for _ in range(REPS):
        for p, (s, geo) in steps.items():
            ms[p].append(timed(lambda: s(geometry=geo), 5) / 1e3)
    out = {"batch": B, "captured": True,
           "ms_per_step": {p: {"median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for p, v in ms.items()},
           "bf16_forward_launches_during_warmup_and_capture": routed["bf16"], "fp32_forward_launches": routed["fp32"],
           "first_losses": first}
    print(json.dumps(out), flush=True)
    return out


def main():
    path = sys.argv[1]
    stages = sys.argv[2:] or ["layers", "step"]
    res = {}
    if os.path.exists(path):
        with open(path) as f:
            res = json.load(f)
    res["device"] = torch.cuda.get_device_name(0)
    for name, fn in (("layers", layers), ("step", step)):
        if name in stages:
            res[name] = fn()
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
