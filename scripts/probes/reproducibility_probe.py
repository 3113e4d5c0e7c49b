"""What still moves the bits of a training step: one step of rpn_multiclass, rpn_multiclass_points and train_rcnn (eager, batch 2, the
committed frames of tests/golden/kitti with synthetic images) is run twice from the same state -- parameters,
buffers, dropout counters, generator states -- and every gradient tensor of the two runs is compared bit for bit, with
determinism.deterministic on and off.  Separately ImgVggPyr alone: the same input and weights, forward + backward twice under the
mode, and a small-width RpnModel on synthetic points (widths of 32: no layer meets the fused gather kernel's 64-channel condition, so
every X-Conv takes the dense fused form).  For every stage the JSON lists the tensors whose bits differ (none = the step repeats), or the refusal the mode raised.

  python scripts/probes/reproducibility_probe.py [--out profiles/reproducibility_probe.json] [--repeats 3]

--level image: only the two stages that fuse the image, rpn_multiclass and train_rcnn, under determinism.deterministic("image") (the
image-feature gradients in their ordered form), written to profiles/reproducibility_probe_image.json.
"""
import argparse
import copy
import json
import lzma
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

IMG_CONV = ((1, 16), (1, 16), (1, 16), (1, 16))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")
IMAGE_WH = (1242, 375)


def make_dataset(root):
    """the committed calibration, labels and point clouds, and one noisy gradient image per frame"""
    from PIL import Image
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    names = sorted(n[:-len(".bin.xz")] for n in os.listdir(os.path.join(GOLD, "velodyne")) if n.endswith(".bin.xz"))
    w, h = IMAGE_WH
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    for i, n in enumerate(names):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        img = np.clip(base + np.random.default_rng(i).normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "image_2", n + ".png"))
    with open(os.path.join(root, "train.txt"), "w") as f:
        f.write("\n".join(names) + "\n")


def small_width(repeats, mode):
    """RpnModel on points with 32-wide X-Conv layers, 2 x 2048 synthetic points: -> (differing gradient tensors, tensors compared)"""
    import dataclasses

    from heterofusionrcnn_amd import checkpoint as C
    from heterofusionrcnn_amd import deterministic, pointcnn as P_, rpn as R_
    small = P_.PointCnnConfig(xconv=((8, 1, -1, 32), (8, 1, 512, 32), (8, 1, 128, 64), (8, 1, 32, 128), (8, 1, 16, 128)), fc=((32, 0.5), (32, 0.5)))
    cfg = dataclasses.replace(R_.rpn_multiclass(0), pointcnn=small, rpn_fc=((64, 0.5), (64, 0.5)))
    rng = np.random.default_rng(0)
    b, p = 2, 2048
    xyz = torch.from_numpy(np.stack([rng.uniform(-8, 8, (b, p)), rng.uniform(-1.0, 1.7, (b, p)), rng.uniform(2, 18, (b, p))], -1).astype(np.float32)).cuda()
    intensity = torch.from_numpy(rng.uniform(-0.5, 0.5, (b, p, 1)).astype(np.float32)).cuda()
    boxes, cls = R_.synthetic_ground_truth(rng, b, 10, cfg, extent=((-7.0, 7.0), (3.0, 17.0)))
    label_cls, label_reg = R_.point_labels(xyz, torch.from_numpy(boxes).cuda(), torch.from_numpy(cls).cuda())
    torch.manual_seed(4)
    model = R_.RpnModel(cfg).cuda().train()
    state, drops, rng_state = copy.deepcopy(model.state_dict()), C.drop_states(model), C.rng_states()
    runs = []
    with deterministic(mode):
        for _ in range(repeats):
            model.load_state_dict(state)
            C.load_drop_states(model, drops)
            C.load_rng_states(rng_state)
            model.zero_grad(set_to_none=True)
            seg, head = model(xyz, intensity)
            model.loss(xyz, seg, head, label_cls, label_reg)[0].backward()
            torch.cuda.synchronize()
            runs.append({n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None})
    return sorted(set(sum((differing(runs[0], r) for r in runs[1:]), []))), len(runs[0])


def differing(a, b):
    return sorted(k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)))


def step_gradients(stage, repeats, mode):
    """`repeats` runs of loss + backward from one state -> (names whose gradient bits differ from the first run's, tensors compared)"""
    from heterofusionrcnn_amd import checkpoint as C
    from heterofusionrcnn_amd import deterministic
    data = stage.open(None)
    try:
        torch.manual_seed(1)
        module = stage.build(data)
        cur = data.next()
        inputs = stage.inputs(cur)
        geometry = stage.geometry(cur.xyz) if stage.geometry else None
        state, drops, rng = copy.deepcopy(module.state_dict()), C.drop_states(module), C.rng_states()
        runs = []
        with deterministic(mode):
            for _ in range(repeats):
                module.load_state_dict(state)
                C.load_drop_states(module, drops)
                C.load_rng_states(rng)
                module.zero_grad(set_to_none=True)
                loss, _ = stage.loss(module, inputs, geometry)
                loss.backward()
                torch.cuda.synchronize()
                grads = {n: p.grad.detach().clone() for n, p in module.named_parameters() if p.grad is not None}
                grads["(loss)"] = loss.detach().reshape(1).clone()
                runs.append(grads)
        bad = sorted(set(sum((differing(runs[0], r) for r in runs[1:]), [])))
        return bad, len(runs[0])
    except RuntimeError as e:
        if "deterministic mode refuses" not in str(e):
            raise
        return "refused: " + str(e), 0
    finally:
        data.close()


def image_pyramid(repeats):
    from heterofusionrcnn_amd import deterministic
    from heterofusionrcnn_amd.inference import ImgVggPyr
    torch.manual_seed(2)
    net = ImgVggPyr().cuda().train()
    x = torch.randn(2, 360, 1200, 3, device="cuda") * 50.0 + 110.0      # channel-last, pixel values
    state = copy.deepcopy(net.state_dict())
    runs = []
    with deterministic(True):
        for _ in range(repeats):
            net.load_state_dict(state)
            net.zero_grad(set_to_none=True)
            xi = x.clone().requires_grad_(True)
            out = net(xi)
            weight = torch.linspace(-1, 1, out.numel(), device="cuda").reshape(out.shape)
            (out * weight).sum().backward()
            torch.cuda.synchronize()
            g = {n: p.grad.detach().clone() for n, p in net.named_parameters()}
            g["(output)"], g["(input gradient)"] = out.detach().clone(), xi.grad.clone()
            runs.append(g)
    return sorted(set(sum((differing(runs[0], r) for r in runs[1:]), []))), len(runs[0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--level", choices=("true", "image"), default="true", help="image: the stages that fuse the image under that level")
    args = ap.parse_args()
    image = args.level == "image"
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "reproducibility_probe_image.json" if image else "reproducibility_probe.json")
    from heterofusionrcnn_amd import export_rpn, train_rcnn, train_rpn
    from heterofusionrcnn_amd.inference import CLASSES
    tmp = tempfile.mkdtemp()
    result = {"device": torch.cuda.get_device_name(0), "repeats": args.repeats, "batch": 2, "img_conv": IMG_CONV}
    try:
        data_dir, hand = os.path.join(tmp, "kitti"), os.path.join(tmp, "handoff")
        os.makedirs(data_dir)
        make_dataset(data_dir)
        if not image:
            bad, n = image_pyramid(args.repeats)
            result["ImgVggPyr alone (2,360,1200,3), forward + backward, mode on"] = {"tensors": n, "differ": bad}
            print("ImgVggPyr:", n, "tensors,", len(bad), "differ", bad)
            for mode in (True, False):
                bad, n = small_width(args.repeats, mode)
                result["small-width RpnModel on points (dense fused X-Conv layers), mode %s" % ("on" if mode else "off")] = {"tensors": n, "differ": bad}
                print("small-width mode", mode, ":", n, "tensors,", len(bad), "differ", bad[:8])
        loader = dict(dataset_dir=data_dir, split="train", batch=2, seed=1, workers=2)
        label = lambda mode: "level image" if mode == "image" else "mode %s" % ("on" if mode else "off")
        for config in (("rpn_multiclass",) if image else ("rpn_multiclass_points", "rpn_multiclass")):
            for mode in (("image",) if image else (True, False)):
                stage = train_rpn.RpnStage(config, IMG_CONV, classes=CLASSES, num_points=16384, **loader)
                bad, n = step_gradients(stage, args.repeats, mode)
                result["%s step, %s" % (config, label(mode))] = {"tensors": n, "differ": bad}
                print(config, "mode", mode, ":", n, "tensors,", bad if isinstance(bad, str) else "%d differ %s" % (len(bad), bad[:8]))
        model_path = os.path.join(hand, "rpn.pt")
        os.makedirs(hand)
        train_rpn.train(data_dir, "train", steps=2, batch=2, seed=1, log_every=0, workers=2, img_conv=IMG_CONV, save=model_path)
        export_rpn.export(data_dir, model_path, hand, "train", batch=2, img_conv=IMG_CONV, workers=2, log=None)
        for mode in (("image",) if image else (True, False)):
            stage = train_rcnn.RcnnStage(IMG_CONV, handoff_dir=hand, aug_list=None, **loader)
            bad, n = step_gradients(stage, args.repeats, mode)
            result["train_rcnn step, %s" % label(mode)] = {"tensors": n, "differ": bad}
            print("train_rcnn mode", mode, ":", n, "tensors,", bad if isinstance(bad, str) else "%d differ %s" % (len(bad), bad[:8]))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
