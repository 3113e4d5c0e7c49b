"""Frames per second of detection from files, three ways over the same frames (the committed KITTI frames repeated to N names,
synthetic PNGs, full-size models with untrained weights, batch 8, score threshold 0 so that every detection reaches the writer):
  device_rows  detect.detect (hand-off in memory, hf_kitti_result_boxes, files written by worker threads)
  host_rows    detect.detect(host_rows=True) (hand-off in memory, inference.write_frame_results box by box)
  file_route   export_rpn.export + rcnn_data.run_rcnn_from_handoff (the hand-off on disk), and the bytes it wrote
each the median wall time of PASSES passes after one warm-up pass, models built once and passed in.  Also the result rows alone
for one batch of 8 x 100 boxes: host wall time per call of inference.result_boxes (its concatenations and small uploads
included, 50 back-to-back calls and one synchronisation) against the wall time of the host loop.
Prints the result as JSON lines and, when a path is given, writes it there (profiles/detect_timing.json is such a file)."""
import json
import lzma
import os
import shutil
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from heterofusionrcnn_amd import export_rpn, inference, train_rcnn, train_rpn  # noqa: E402
from heterofusionrcnn_amd import rcnn_data as RD  # noqa: E402
from heterofusionrcnn_amd.detect import detect, rpn_fts_channels  # noqa: E402

N, BATCH, PASSES, WORKERS = 64, 8, 5, 8
GOLD = ["000000", "000001", "000002", "000003"]
SIZES = [(1242, 375), (1224, 370), (1242, 375), (1224, 370)]


def dataset(tmp):
    gold = os.path.join(ROOT, "tests", "golden", "kitti")
    src = os.path.join(tmp, "src")
    os.makedirs(src)
    from PIL import Image
    rng = np.random.default_rng(0)
    for n, (w, h) in zip(GOLD, SIZES):
        with lzma.open(os.path.join(gold, "velodyne", n + ".bin.xz")) as f, open(os.path.join(src, n + ".bin"), "wb") as o:
            o.write(f.read())
        Image.fromarray(rng.integers(0, 255, (h, w, 3), dtype=np.uint8)).save(os.path.join(src, n + ".png"))
    for d in ("velodyne", "image_2", "calib", "label_2"):
        os.makedirs(os.path.join(tmp, d))
    names = ["%06d" % i for i in range(N)]
    for i, name in enumerate(names):
        g = GOLD[i % len(GOLD)]
        os.symlink(os.path.join(src, g + ".bin"), os.path.join(tmp, "velodyne", name + ".bin"))
        os.symlink(os.path.join(src, g + ".png"), os.path.join(tmp, "image_2", name + ".png"))
        for d in ("calib", "label_2"):
            shutil.copy(os.path.join(gold, d, g + ".txt"), os.path.join(tmp, d, name + ".txt"))
    with open(os.path.join(tmp, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return names


def tree_bytes(path):
    return sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(path) for f in fs)


def passes(fn, cleanup=None):
    times, last = [], None
    for i in range(PASSES + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn()
        torch.cuda.synchronize()
        if i > 0:
            times.append(time.perf_counter() - t0)
        if cleanup and i < PASSES:
            cleanup()
    return times, last


def rows_alone():
    """one batch of 8 frames x 100 boxes in view"""
    rng = np.random.default_rng(1)
    from heterofusionrcnn_amd import kitti_io
    p2 = kitti_io.read_calib(os.path.join(ROOT, "tests", "golden", "kitti", "calib", "000000.txt"))["p2"].astype(np.float32)
    dets_np = []
    for _ in range(BATCH):
        z = rng.uniform(8, 60, 100)
        boxes = np.stack([rng.uniform(-0.6, 0.6, 100) * z, rng.uniform(1.0, 2.0, 100), z, rng.uniform(3, 4.5, 100), rng.uniform(1.4, 1.8, 100),
                          rng.uniform(1.3, 1.7, 100), rng.uniform(-3.1, 3.1, 100)], 1).astype(np.float32)
        dets_np.append({"boxes": boxes, "scores": rng.uniform(0, 1, 100).astype(np.float32), "classes": rng.integers(1, 4, 100)})
    dets = [{k: torch.from_numpy(v).cuda() for k, v in d.items()} for d in dets_np]
    p2s, whs = np.stack([p2] * BATCH), np.array([[1242, 375]] * BATCH, np.int32)
    p2d, whd = torch.from_numpy(p2s.astype(np.float64)).cuda(), torch.from_numpy(whs).cuda()
    for _ in range(5):
        inference.result_boxes(dets, p2d, whd, 0.1)
    torch.cuda.synchronize()
    n = 50
    t0 = time.perf_counter()
    for _ in range(n):
        inference.result_boxes(dets, p2d, whd, 0.1)
    torch.cuda.synchronize()
    dev_us = 1e6 * (time.perf_counter() - t0) / n
    with tempfile.TemporaryDirectory() as tmp:
        t0 = time.perf_counter()
        for _ in range(3):
            wrote = sum(inference.write_frame_results(os.path.join(tmp, "h.txt"), d, p2, (1242, 375), 0.1) for d in dets_np)
        host_ms = 1e3 * (time.perf_counter() - t0) / 3
        rows = inference.result_rows(inference.result_boxes(dets, p2d, whd, 0.1)).cpu().numpy()
        t0 = time.perf_counter()
        for _ in range(3):
            wrote_d = sum(inference.write_result_rows(os.path.join(tmp, "d.txt"), rows[100 * i:100 * i + 100]) for i in range(BATCH))
        fmt_ms = 1e3 * (time.perf_counter() - t0) / 3
    return {"boxes_per_batch": 100 * BATCH, "result_boxes_wall_us_per_batch": dev_us, "host_loop_ms_per_batch": host_ms,
            "row_writer_ms_per_batch": fmt_ms, "rows_written_host": wrote, "rows_written_device": wrote_d}


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    res = {"device": torch.cuda.get_device_name(0), "frames": N, "batch": BATCH, "passes": PASSES, "workers": WORKERS,
           "score_threshold": 0.0}
    res["rows_alone"] = rows_alone()
    print(json.dumps(res), flush=True)
    torch.manual_seed(0)
    net, _ = train_rpn.make_model("rpn_multiclass")
    trainer = train_rcnn.make_trainer(rpn_fts_channels(net.rpn))
    with tempfile.TemporaryDirectory() as tmp:
        names = dataset(tmp)
        out, handoff = os.path.join(tmp, "out"), os.path.join(tmp, "handoff")
        kw = dict(split="val", batch=BATCH, workers=WORKERS, score_threshold=0.0)
        for key, host_rows in (("device_rows", False), ("host_rows", True)):
            t, written = passes(lambda: detect(tmp, net, trainer, out, host_rows=host_rows, **kw))
            res[key] = {"seconds": t, "frames_per_s": N / statistics.median(t), "rows_written": sum(written.values())}
            print(json.dumps({key: res[key]}), flush=True)
        wrote = {}

        def file_route():
            export_rpn.export(tmp, net, handoff, "val", batch=BATCH, workers=WORKERS, log=None)
            return RD.run_rcnn_from_handoff(trainer, tmp, handoff, names, out, batch=BATCH, workers=WORKERS, score_threshold=0.0)

        def measure_and_remove():                       # outside the timed region
            wrote["bytes"] = tree_bytes(handoff)
            shutil.rmtree(handoff)

        t, written = passes(file_route, cleanup=measure_and_remove)
        res["file_route"] = {"seconds": t, "frames_per_s": N / statistics.median(t), "rows_written": sum(written.values()),
                             "handoff_bytes": wrote["bytes"], "handoff_bytes_per_frame": wrote["bytes"] / N}
        print(json.dumps({"file_route": res["file_route"]}), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
