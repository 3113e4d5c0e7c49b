"""Timing of the RPN -> RCNN hand-off at b = 8, p = 16384, c = 288: hf_rpn_handoff_pack and hf_rcnn_batch_inputs (device time per
call from back-to-back calls between two events, bytes read + written), the loader's wall time per batch
(rcnn_data.KittiRcnnBatches, train mode, on the committed KITTI frames with a synthetic hand-off), and the captured RCNN step
fed from files against the same step replayed on resident inputs.  Prints the result as one JSON line and, when a path is
given, also writes it there (profiles/rcnn_handoff_timing.json is such a file)."""
import json
import lzma
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from heterofusionrcnn_amd import rcnn_data as RD  # noqa: E402

B, P, C = 8, 16384, 288


def timed(fn, n=50):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n


def kernels():
    g = torch.Generator(device="cuda").manual_seed(0)
    xyz = torch.randn(B, P, 3, device="cuda", generator=g)
    inten = torch.randn(B, P, 1, device="cuda", generator=g)
    fg = torch.rand(B, P, device="cuda", generator=g) < 0.3
    fts = torch.randn(B, P, C, device="cuda", generator=g)
    rows = RD.handoff_pack(xyz, inten, fg, fts)
    flip = torch.tensor([i % 2 for i in range(B)], dtype=torch.int32, device="cuda")
    t_pack = timed(lambda: RD.handoff_pack(xyz, inten, fg, fts))
    t_in = timed(lambda: RD.batch_inputs(rows, flip))
    moved = B * P * ((5 + C) * 4 + 12 + 4 + 1 + 4 * C)   # the rows on one side; xyz, intensity, fg (1 byte), rpn_fts on the other
    return {"pack_us": t_pack, "pack_TBps": moved / t_pack / 1e6, "batch_inputs_us": t_in, "batch_inputs_TBps": moved / t_in / 1e6,
            "bytes_read_plus_written": moved}


def dataset(tmp):
    gold = os.path.join(ROOT, "tests", "golden", "kitti")
    names = ["000000", "000001", "000002", "000003"]
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(gold, d), os.path.join(tmp, d))
    for d in ("velodyne", "image_2") + RD.HANDOFF_DIRS:
        os.makedirs(os.path.join(tmp, d))
    from PIL import Image
    rng = np.random.default_rng(0)
    for n in names:
        with lzma.open(os.path.join(gold, "velodyne", n + ".bin.xz")) as f, open(os.path.join(tmp, "velodyne", n + ".bin"), "wb") as o:
            o.write(f.read())
        Image.fromarray(rng.integers(0, 255, (375, 1242, 3), dtype=np.uint8)).save(os.path.join(tmp, "image_2", n + ".png"))
        rows = rng.standard_normal((P, 5 + C)).astype(np.float32)
        rows[:, 4] = rng.random(P) < 0.2
        np.save(os.path.join(tmp, "rpn_feature", n + ".npy"), rows)
        props = np.concatenate([rng.uniform(-20, 20, (100, 1)), rng.uniform(1, 2, (100, 1)), rng.uniform(5, 60, (100, 1)),
                                rng.uniform(1, 4, (100, 3)), rng.uniform(-3, 3, (100, 1))], 1)
        np.savetxt(os.path.join(tmp, "proposals_and_scores", n + ".txt"), np.hstack([props, rng.random((100, 1))]), fmt="%.3f")
    with open(os.path.join(tmp, "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    return tmp


def loader_and_step(root):
    from heterofusionrcnn_amd import train_rcnn
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    from heterofusionrcnn_amd.rcnn_train import rcnn_train_loss
    out = {}
    data = RD.KittiRcnnBatches(root, root, "train", batch=B, seed=0, workers=16)
    try:
        data.next()
        torch.cuda.synchronize()
        n = 10
        t0 = time.perf_counter()
        for _ in range(n):
            data.next()
        torch.cuda.synchronize()
        out["loader_ms_per_batch"] = 1e3 * (time.perf_counter() - t0) / n
        torch.manual_seed(0)
        trainer = train_rcnn.make_trainer(C, seed=0)
        cur = data.next()
        opt = MultiTensorAdam([p for p in trainer.parameters() if p.requires_grad], lr=1e-3, tf_epsilon=False)
        step = TrainStep(trainer, opt, cur.train_inputs(), None, graph=True, loss_fn=rcnn_train_loss)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        out["step_resident_ms"] = 1e3 * (time.perf_counter() - t0) / n
        nxt = data.next()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(n):
            cur, nxt = nxt, data.next()
            step(**cur.train_inputs())
        torch.cuda.synchronize()
        out["step_file_fed_ms"] = 1e3 * (time.perf_counter() - t0) / n
    finally:
        data.close()
    out["batch"] = B
    return out


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else None
    res = {"b": B, "p": P, "c": C, "device": torch.cuda.get_device_name(0)}
    res.update(kernels())
    print(json.dumps(res), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        res.update(loader_and_step(dataset(tmp)))
    print(json.dumps(res), flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
