"""The tree with train_loop.run against a checkout of its parent commit: the same trajectory, and the same ms/step.

  train_loop_equivalence.py --parent DIR --out DIR [--cases 1,2,3,4,5]      runs, one result file per case (case_N.json)
  train_loop_equivalence.py --parent DIR --out DIR --timing                  ms/step and bench.py, alternating (timing.json)
  train_loop_equivalence.py --report DIR                                     the tables of profiles/train_loop_equivalence.md and
                                                                             profiles/train_loop_ab.md from those files (no GPU)

DIR of --parent is a built checkout of the parent commit; the new tree is the one this file lies in.  Every train() call is a fresh
process under its own time limit (this file again, with --child and the tree to import from), and the first one that fails ends
the whole run.  Trajectory: the four committed KITTI frames, dataset and hand-off as in tests/test_train_resume.py, batch 2, seed 1,
2 workers, img_conv ((1, 16),) * 4, that test's train op, 6 steps with a checkpoint every 3 and a log line every 2; the parent
tree twice and the new tree twice per case, for the eager cases each followed by a resume from its own step-3 checkpoint.  Exact:
the checkpoint files, their keys, global_step, config, settings, loader, drop_states, the optimizer's step_count, keys and shapes of
model and of the --save file, the log lines with every number masked.  Gaps: the rule and numbers of tests/test_train_resume.py
(relative loss gap, max over steps; L2 gap over the floating-point entries of the --save file; each new-against-parent pair at most
max(20 x the parent's own two-run gap, 1e-5)).  Timing: the ms/step of the last log line of 60 captured steps over the dataset of
detect_timing.py (64 names), RPN at batch 8 and RCNN at batch 2, and bench.py's headline, three parent / new pairs each.
"""
import argparse
import itertools
import json
import lzma
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
NAMES = ["000000", "000001", "000002", "000003"]
SIZES = {"000000": (1242, 375), "000001": (1224, 370), "000002": (1242, 375), "000003": (1224, 370)}
IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))
TRAIN_OP = dict(lr=1e-3, clip_norm=1.0, lr_decay=(2, 0.8, True), tf_epsilon=True, check_numerics=True)
FACTOR, FLOOR = 20.0, 1e-5
CASES = {1: ("rpn_multiclass, captured", "rpn", "rpn_multiclass", True), 2: ("rpn_multiclass, eager, resumed", "rpn", "rpn_multiclass", False),
         3: ("rpn_multiclass_points, captured", "rpn", "rpn_multiclass_points", True), 4: ("RCNN, captured", "rcnn", None, True),
         5: ("RCNN, eager, resumed", "rcnn", None, False)}
ORDER = ("parent1", "new1", "parent2", "new2")
PAIRS = [(p, n) for p in ("parent1", "parent2") for n in ("new1", "new2")]


# ------------------------------------------------------------------------------------------------ one call, in a fresh process
def child(tree, spec):
    sys.path.insert(0, tree)
    import heterofusionrcnn_amd
    assert os.path.dirname(os.path.dirname(os.path.abspath(heterofusionrcnn_amd.__file__))) == os.path.abspath(tree)
    from heterofusionrcnn_amd import export_rpn, train_rcnn, train_rpn
    kw = {k: tuple(tuple(v) if isinstance(v, list) else v for v in val) if k in ("img_conv", "lr_decay") and val is not None else val
          for k, val in spec.get("kw", {}).items()}
    lines = []
    if spec["do"] == "handoff":                              # the hand-off fixture of tests/test_train_resume.py
        model = os.path.join(spec["out"], "rpn.pt")
        train_rpn.train(spec["dataset"], "train", steps=2, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, save=model)
        export_rpn.export(spec["dataset"], model, spec["out"], "train", batch=2, img_conv=IMG_CONV, workers=2, log=None)
        return
    if spec["do"] == "handoff64":                            # detect_timing.py's: full-size untrained models, batch 8
        import torch
        torch.manual_seed(0)
        export_rpn.export(spec["dataset"], train_rpn.make_model("rpn_multiclass")[0], spec["out"], "val", batch=8, workers=8, log=None)
        return
    losses, _ = (train_rpn if spec["do"] == "rpn" else train_rcnn).train(log=lines.append, **kw)
    with open(spec["result"], "w") as f:
        json.dump({"losses": losses, "log": lines}, f)


def spawn(tree, spec, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--child", tree, json.dumps(spec)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        print("FAILED (status %d): %s\n%s\n%s" % (r.returncode, spec, r.stdout[-3000:], r.stderr[-3000:]), flush=True)
        sys.exit(r.returncode or 1)


def kitti_frames(root):
    """the dataset fixture of tests/test_train_resume.py"""
    from PIL import Image
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    for i, n in enumerate(NAMES):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        w, h = SIZES[n]
        rng = np.random.default_rng(i)
        yy, xx = np.mgrid[0:h, 0:w]
        base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
        Image.fromarray(np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)).save(os.path.join(root, "image_2", n + ".png"))
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(NAMES) + "\n")


# ------------------------------------------------------------------------------------------------ what a run left behind
def plain(o):
    import torch
    if isinstance(o, torch.Tensor):
        return o.tolist()
    if isinstance(o, dict):
        return {str(k): plain(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [plain(v) for v in o]
    return o.tolist() if isinstance(o, np.generic) else o


def facts(run_dir, log):
    """everything that must be equal between two runs, as plain data"""
    import torch
    from heterofusionrcnn_amd import checkpoint as C
    shapes = lambda sd: {k: list(v.shape) for k, v in sd.items()}
    out = {"files": sorted(os.listdir(os.path.join(run_dir, "ck"))), "save": shapes(torch.load(os.path.join(run_dir, "save.pt"), map_location="cpu")),
           "log": [re.sub(r"[-+]?(\d+\.?\d*(e[-+]?\d+)?|nan|inf)", "#", l.replace(run_dir, "<run>")) for l in log]}
    for name in out["files"]:
        ck = C.load_checkpoint(os.path.join(run_dir, "ck", name))
        out[name] = {"keys": sorted(ck), "model": shapes(ck["model"]), "step_count": float(ck["optimizer"]["step_count"]),
                     **{k: plain(ck[k]) for k in ("global_step", "config", "settings", "loader", "drop_states")}}
    return out


def params(run_dir):
    import torch
    sd = torch.load(os.path.join(run_dir, "save.pt"), map_location="cpu")
    return {k: v.double().numpy() for k, v in sd.items() if v.is_floating_point()}


def param_gap(a, b):
    return (sum(float(((a[k] - b[k]) ** 2).sum()) for k in a) / sum(float((a[k] ** 2).sum()) for k in a)) ** 0.5


def loss_gap(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b)) / np.abs(np.asarray(a))))


def compare(dirs, results, first):
    """dirs / results: {tag: run directory / {"losses", "log"}}; losses[first:] are compared -> the case's table row"""
    f = {t: facts(dirs[t], results[t]["log"]) for t in ORDER}
    differs = sorted({k for t in ORDER[1:] for k in set(f[t]) | set(f["parent1"]) if f[t].get(k) != f["parent1"].get(k)})
    p = {t: params(dirs[t]) for t in ORDER}
    ls = {t: results[t]["losses"][first:] for t in ORDER}
    own = (loss_gap(ls["parent1"], ls["parent2"]), param_gap(p["parent1"], p["parent2"]))
    bound = (max(FACTOR * own[0], FLOOR), max(FACTOR * own[1], FLOOR))
    pairs = {"%s-%s" % (a, b): (loss_gap(ls[a], ls[b]), param_gap(p[a], p[b])) for a, b in PAIRS}
    return {"exact_differs": differs, "log": f["new1"]["log"], "files": f["new1"]["files"], "first_loss": {t: ls[t][0] for t in ORDER},
            "parent_gap": own, "bound": bound, "pairs": pairs,
            "within": not differs and all(g[0] <= bound[0] and g[1] <= bound[1] for g in pairs.values())}


def run_case(n, trees, dataset, handoff, work):
    title, which, config, graph = CASES[n]
    from heterofusionrcnn_amd import checkpoint as C
    kw = dict(dataset_dir=dataset, split="train", batch=2, seed=1, workers=2, img_conv=IMG_CONV, steps=6, checkpoint_every=3, log_every=2,
              graph=graph, **TRAIN_OP)
    kw.update({"config": config} if which == "rpn" else {"handoff_dir": handoff})
    dirs, res, rdirs, rres = {}, {}, {}, {}
    for tag in ORDER:
        d = dirs[tag] = os.path.join(work, "case%d" % n, tag)
        os.makedirs(d)
        spec = {"do": which, "result": os.path.join(d, "run.json"), "kw": dict(kw, checkpoint_dir=os.path.join(d, "ck"), save=os.path.join(d, "save.pt"))}
        spawn(trees[tag[:-1]], spec, 300)
        res[tag] = json.load(open(spec["result"]))
        if not graph:                                        # the eager cases: resume from this run's own step-3 checkpoint
            r = rdirs[tag] = os.path.join(d, "resumed")
            os.makedirs(os.path.join(r, "ck"))
            shutil.copy(C.checkpoint_path(os.path.join(d, "ck"), 3), os.path.join(r, "ck"))
            spec = {"do": which, "result": os.path.join(r, "run.json"),
                    "kw": dict(kw, checkpoint_dir=os.path.join(r, "ck"), save=os.path.join(r, "save.pt"), resume=True)}
            spawn(trees[tag[:-1]], spec, 300)
            rres[tag] = json.load(open(spec["result"]))
        print("case %d %s done" % (n, tag), flush=True)
    out = {"case": n, "title": title, "run": compare(dirs, res, 0)}
    if rres:
        out["resumed"] = compare(rdirs, rres, 0)
    return out


# ------------------------------------------------------------------------------------------------ ms/step, alternating
def timing(trees, work):
    sys.path.insert(0, HERE)
    import detect_timing as DT
    data, handoff = os.path.join(work, "kitti64"), os.path.join(work, "handoff64")
    os.makedirs(data)
    DT.dataset(data)
    spawn(trees["parent"], {"do": "handoff64", "dataset": data, "out": handoff}, 300)
    runs = {"rpn": {"parent": [], "new": []}, "rcnn": {"parent": [], "new": []}, "bench": {"parent": [], "new": []}}
    common = dict(dataset_dir=data, split="val", steps=60, log_every=60, workers=8, seed=0)
    for which, kw in (("rpn", dict(common, batch=8, config="rpn_multiclass")), ("rcnn", dict(common, batch=2, handoff_dir=handoff))):
        for _, tag in itertools.product(range(3), ("parent", "new")):
            spec = {"do": which, "result": os.path.join(work, "timing_run.json"), "kw": kw}
            spawn(trees[tag], spec, 300)
            line = [l for l in json.load(open(spec["result"]))["log"] if l.startswith("step 60 ")][-1]
            runs[which][tag].append(float(re.search(r"([0-9.]+) ms/step", line).group(1)))
            print(which, tag, runs[which][tag][-1], flush=True)
    for _, tag in itertools.product(range(3), ("parent", "new")):
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "bench.py", "--gpus", "1", "--steps", "20", "--warmup", "3"],
                           cwd=trees[tag], capture_output=True, text=True)
        if r.returncode != 0:
            print("bench.py FAILED (status %d)\n%s\n%s" % (r.returncode, r.stdout[-3000:], r.stderr[-3000:]), flush=True)
            sys.exit(r.returncode)
        runs["bench"][tag].append(json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])["value"])
        print("bench", tag, runs["bench"][tag][-1], flush=True)
    return runs


# ------------------------------------------------------------------------------------------------ the tables
def report(d):
    g = lambda v: "%.3g" % v
    print("| case | exact fields | loss of global step 1 bit-equal: parent1 = parent2 / all four | parent's own gap, loss / parameters | bound | "
          "new-against-parent pairs, loss / parameters (worst of 4) | within |\n|---|---|---|---|---|---|---|")
    for n in sorted(CASES):
        path = os.path.join(d, "case_%d.json" % n)
        if not os.path.exists(path):
            continue
        c = json.load(open(path))
        for part in ("run", "resumed"):
            if part in c:
                r, fl = c[part], c[part]["first_loss"]
                worst = [max(v[i] for v in r["pairs"].values()) for i in (0, 1)]
                print("| %d %s%s | %s | %s / %s | %s / %s | %s / %s | %s / %s | %s |" % (
                    n, c["title"], " (steps 4-6 after the resume)" if part == "resumed" else "",
                    "all equal" if not r["exact_differs"] else "DIFFER: " + ", ".join(r["exact_differs"]),
                    *(("-", "-") if part == "resumed" else ("yes" if fl["parent1"] == fl["parent2"] else "no",
                                                            "yes" if len(set(fl.values())) == 1 else "no")),
                    g(r["parent_gap"][0]), g(r["parent_gap"][1]), g(r["bound"][0]), g(r["bound"][1]), g(worst[0]), g(worst[1]),
                    "yes" if r["within"] else "NO"))
    path = os.path.join(d, "timing.json")
    if os.path.exists(path):
        t = json.load(open(path))
        print("\n| figure | parent runs | new runs | parent median | spread | new median | excess | within |\n|---|---|---|---:|---:|---:|---:|---|")
        names = {"rpn": "`train_rpn.train` ms/step (rpn_multiclass, batch 8)", "rcnn": "`train_rcnn.train` ms/step (batch 2)",
                 "bench": "`bench.py` headline, frames/s"}
        for k in ("rpn", "rcnn", "bench"):
            p, n = t[k]["parent"], t[k]["new"]
            pm, nm, spread = statistics.median(p), statistics.median(n), max(p) - min(p)
            slower = pm - nm if k == "bench" else nm - pm                   # frames/s: higher is better
            print("| %s | %s | %s | %s | %s | %s | %+.4g | %s |" % (names[k], ", ".join(g4(v) for v in p), ", ".join(g4(v) for v in n), g4(pm),
                                                                    g4(spread), g4(nm), nm - pm, "yes" if slower <= spread else "NO"))


def g4(v):
    return "%.4g" % v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=2)
    ap.add_argument("--parent")
    ap.add_argument("--out")
    ap.add_argument("--cases", default="1,2,3,4,5")
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--report")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], json.loads(a.child[1]))
    if a.report:
        return report(a.report)
    sys.path.insert(0, ROOT)
    trees = {"parent": os.path.abspath(a.parent), "new": ROOT}
    os.makedirs(a.out, exist_ok=True)
    with tempfile.TemporaryDirectory() as work:
        if a.timing:
            with open(os.path.join(a.out, "timing.json"), "w") as f:
                json.dump(timing(trees, work), f, indent=1)
            return
        dataset, handoff = os.path.join(work, "kitti"), os.path.join(work, "handoff")
        os.makedirs(dataset), os.makedirs(handoff)
        kitti_frames(dataset)
        cases = [int(c) for c in a.cases.split(",")]
        if any(CASES[n][1] == "rcnn" for n in cases):
            spawn(trees["parent"], {"do": "handoff", "dataset": dataset, "out": handoff}, 300)
        for n in cases:
            with open(os.path.join(a.out, "case_%d.json" % n), "w") as f:
                json.dump(run_case(n, trees, dataset, handoff, work), f, indent=1)


if __name__ == "__main__":
    main()
