"""GPU tests of the image pyramid's bf16 route through the Python layer (image_pyramid.image_precision, forward_native, detect.py).

No whole-module tolerance: a CPU emulation of this model with fp32 against fp64 accumulation differs by 1.9e-5 at seed 0 and by 4e-3 at
seed 1 -- one activation that flips to the neighbouring bf16 value is amplified downstream -- so a tolerance measured on one seed
would be luck.  Instead every layer is checked on its own: the reference of tests/conv_bf16_cases.py is fed with what the kernels
produced for the layers before it, wired as image_pyramid_cases.module_forward wires them, and held to the derived bound.  That a
wrong wiring would show is asserted first, on the reference side."""
import lzma
import os
import shutil
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bf16_cases as cb  # noqa: E402
import image_pyramid_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "kitti")


def routed(net, image):
    """the layers the documented predicate sends to the bf16 kernels, of the module's convolutions in launch order"""
    from heterofusionrcnn_amd import image_pyramid
    b, h, w, _ = image.shape
    n = 0
    for name, seq, _ in cb.module_layers(net):
        if seq is not None:
            conv = seq[0]
            up = isinstance(conv, torch.nn.ConvTranspose2d)
            level = int(name[-3 if name.startswith("conv") else -1]) - 1
            rows = b * (h >> (level + 1 if up else level)) * (w >> (level + 1 if up else level))
            n += bool(image_pyramid.bf16_conv_pays(rows, conv.in_channels, conv.out_channels, up))
    return n


def _run(net, image, precision, taps=None):
    from heterofusionrcnn_amd import image_pyramid
    with torch.no_grad(), image_pyramid.image_precision(precision):
        return image_pyramid.forward_native(net, image, taps=taps)


def _mean():
    from heterofusionrcnn_amd.inference import IMAGE_MEAN
    return torch.tensor(IMAGE_MEAN, dtype=torch.float32)


def check_layers(host_net, taps, image, what):
    """every tapped output against the layer's reference on the tapped inputs; -> {tap name: the layer's largest bound}"""
    got = {name: t.detach().cpu() for name, t in taps}
    order = [name for name, _ in taps]
    recs = cb.module_layers(host_net)
    assert order == [r[0] for r in recs], "launch order"
    largest, worst = {}, 0.0
    for name, seq, src in recs:
        if src == "image":
            x, sub = image.cpu(), _mean()
        elif isinstance(src, tuple):
            x, sub = torch.cat([got[src[1]], got[src[2]]], dim=-1), None          # [encoder | up], the module's order
        else:
            x, sub = got[src], None
        if seq is None:
            want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
            assert torch.equal(got[name], want), "%s: %s differs from max_pool2d of its input" % (what, name)
            continue
        y, bound = cb.layer_reference(seq, x, sub)
        assert got[name].shape == y.shape, (name, got[name].shape, y.shape)
        ratio = float(((got[name].double() - y).abs() / bound).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, "%s: %s outside its bound, ratio %.3g" % (what, name, ratio)
        largest[name] = float(bound.max())
    print("%s: %d layers, worst |got - ref64| / bound = %.3g" % (what, len(largest), worst))
    return largest, got


def check_wiring_is_visible(host_net, got, largest):
    """on the reference side: the halves of each level's concat swapped move that fusion layer's reference by more than SWAP_FACTOR
    times the layer's largest bound"""
    for name, seq, src in cb.module_layers(host_net):
        if isinstance(src, tuple):
            right, _ = cb.layer_reference(seq, torch.cat([got[src[1]], got[src[2]]], dim=-1))
            swapped, _ = cb.layer_reference(seq, torch.cat([got[src[2]], got[src[1]]], dim=-1))
            moved = float((right - swapped).abs().max())
            print("%s: swapped halves move the reference by %.3g, largest bound %.3g" % (name, moved, largest[name]))
            assert moved > pc.SWAP_FACTOR * largest[name], name


@pytest.mark.parametrize("conv", [pc.MODEL_CONV, cb.MODEL_CONV_DEEP], ids=["model_conv", "two_and_three_layers"])
def test_every_layer_within_its_bound_under_both_scopes(conv, monkeypatch):
    from heterofusionrcnn_amd import image_pyramid
    monkeypatch.setattr(image_pyramid, "bf16_conv_pays", lambda rows, cin, cout, up: True)      # all layers on the bf16 kernels
    host = pc.make_model(conv=conv)
    net, image = pc.make_model(conv=conv).cuda(), pc.make_image().cuda()
    n_layers = sum(1 for r in cb.module_layers(host) if r[1] is not None)
    before = image_pyramid.NATIVE_BF16_LAUNCHES[0]
    taps32 = []
    out32 = _run(net, image, "fp32", taps32)
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == before, "the bf16 counter moved under fp32"
    taps16 = []
    out16 = _run(net, image, "bf16", taps16)
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == before + n_layers
    assert len(taps16) == len(taps32) == n_layers + 3 and taps16[-1][1] is out16 and taps32[-1][1] is out32
    largest, got = check_layers(host, taps16, image, "bf16")
    check_wiring_is_visible(host, got, largest)
    # the fp32 kernels keep their own, tighter contract (tests/test_image_pyramid_abi.py); here: the same wiring, pools included
    got32 = {name: t.cpu() for name, t in taps32}
    for name, seq, src in cb.module_layers(host):
        if seq is None:
            assert torch.equal(got32[name], F.max_pool2d(got32[src].permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)), name
    assert [n for n, _ in taps32] == [n for n, _ in taps16]


def test_predicate_keeps_the_first_layer_on_the_fp32_kernel():
    """the documented routing: cin = 3 stays fp32 -- its output has the fp32 route's bits -- and every other layer is bf16 and within
    its bound on the inputs it was given"""
    from heterofusionrcnn_amd import image_pyramid
    host = pc.make_model()
    net, image = pc.make_model().cuda(), pc.make_image().cuda()
    n_layers = sum(1 for r in cb.module_layers(host) if r[1] is not None)
    assert routed(net, image) == n_layers - 1
    assert not image_pyramid.bf16_conv_pays(2 * 24 * 40, 3, 8, False) and image_pyramid.bf16_conv_pays(2 * 24 * 40, 8, 16, False)
    taps32, taps16 = [], []
    _run(net, image, "fp32", taps32)
    before = image_pyramid.NATIVE_BF16_LAUNCHES[0]
    _run(net, image, "bf16", taps16)
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == before + n_layers - 1
    assert taps16[0][0] == taps32[0][0] == "conv1_0" and torch.equal(taps16[0][1], taps32[0][1])
    second = [n for n, _ in taps16].index("conv2_0")
    assert not torch.equal(taps16[second][1], taps32[second][1])
    got = {name: t.cpu() for name, t in taps16}
    for name, seq, src in cb.module_layers(host)[1:]:
        if seq is not None:
            x = torch.cat([got[src[1]], got[src[2]]], dim=-1) if isinstance(src, tuple) else got[src]
            y, bound = cb.layer_reference(seq, x)
            assert bool(((got[name].double() - y).abs() <= bound).all()), name


def test_route_accounting_and_bits():
    from heterofusionrcnn_amd import image_pyramid
    net, image = pc.make_model().cuda(), pc.make_image().cuda()
    n_layers = routed(net, image)
    with torch.no_grad(), image_pyramid.image_branch("native"):
        first32 = net(image)                                   # no precision scope, before any bf16 call on this module
    calls, launches = image_pyramid.NATIVE_CALLS[0], image_pyramid.NATIVE_BF16_LAUNCHES[0]
    with torch.no_grad(), image_pyramid.image_branch("native"), image_pyramid.image_precision("bf16"):
        a = net(image)
        b = net(image)
    assert image_pyramid.NATIVE_CALLS[0] == calls + 2 and image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches + 2 * n_layers
    assert image_pyramid.image_precision_name() == "fp32"
    assert torch.equal(a, b), "two bf16 calls differ"
    assert not torch.equal(a, first32), "the bf16 route gave the fp32 route's bits"
    with torch.no_grad(), image_pyramid.image_branch("native"):
        again = net(image)
        with image_pyramid.image_precision("fp32"):
            inside = net(image)
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches + 2 * n_layers
    assert torch.equal(first32, again) and torch.equal(first32, inside), "the fp32 native bits moved after a bf16 call"
    with torch.no_grad(), image_pyramid.image_precision("bf16"):
        stock = net(image)                                     # the precision scope alone routes nothing
    with torch.no_grad():
        assert torch.equal(stock, net(image))
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches + 2 * n_layers


def test_cache_and_its_bf16_weights_are_rebuilt_after_load_state_dict():
    from heterofusionrcnn_amd import image_pyramid
    net, image = pc.make_model().cuda(), pc.make_image().cuda()
    first = _run(net, image, "bf16")
    packed = image_pyramid.pack(net)
    layers = [l for block in packed["blocks"] for l in block] + packed["up"] + packed["fusion"]
    assert "wt_bf16" not in layers[0], "the first layer stays on the fp32 kernel and needs no bf16 weights"
    assert all(l["wt_bf16"].dtype == torch.bfloat16 and l["wt_bf16"].shape == l["wt"].shape for l in layers[1:])
    assert image_pyramid.pack(net) is packed
    held = layers[1]["wt_bf16"]
    _run(net, image, "bf16")
    assert image_pyramid.pack(net)["blocks"][1][0]["wt_bf16"] is held, "the bf16 weights were converted again"
    other = pc.make_model(seed=5)
    net.load_state_dict(other.state_dict())
    taps = []
    second = _run(net, image, "bf16", taps)
    repacked = image_pyramid.pack(net)
    assert repacked is not packed and repacked["blocks"][1][0]["wt_bf16"] is not held
    # the first layer ran on the fp32 kernel: its tighter bound is inside this one (u' = 2 u, 9 cin + 8 > 9 cin + 2) only up to the
    # operand rounding, so it is checked from the second layer on, each on the inputs it was given
    got = {name: t.cpu() for name, t in taps}
    for name, seq, src in cb.module_layers(other)[1:]:
        if seq is not None:
            x = torch.cat([got[src[1]], got[src[2]]], dim=-1) if isinstance(src, tuple) else got[src]
            y, bound = cb.layer_reference(seq, x)
            assert bool(((got[name].double() - y).abs() <= bound).all()), name
    assert not torch.equal(first, second)
    assert float((first - second).abs().max()) > pc.SWAP_FACTOR * pc.model_reference()["tol"], "the two models do not differ"
    # a pack made under fp32 gains its bf16 weights on the first bf16 use, without a rebuild
    net.load_state_dict(pc.make_model(seed=6).state_dict())
    _run(net, image, "fp32")
    fresh = image_pyramid.pack(net)
    assert "wt_bf16" not in fresh["blocks"][1][0]
    _run(net, image, "bf16")
    assert image_pyramid.pack(net) is fresh and "wt_bf16" in fresh["blocks"][1][0]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_training_mode_or_autograd_still_raises(precision):
    from heterofusionrcnn_amd import image_pyramid
    net, image = pc.make_model().cuda(), pc.make_image().cuda()
    launches = image_pyramid.NATIVE_BF16_LAUNCHES[0]
    with image_pyramid.image_branch("native"), image_pyramid.image_precision(precision):
        with pytest.raises(RuntimeError, match="inference only"):
            net(image)                                         # autograd on
        net.train()
        with torch.no_grad(), pytest.raises(RuntimeError, match="inference only"):
            net(image)
        net.eval()
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches


def test_forward_train_never_reads_the_precision():
    import copy
    from heterofusionrcnn_amd import image_pyramid
    image = pc.make_image().cuda()
    outs, grads = [], []
    for precision in ("fp32", "bf16"):
        net = copy.deepcopy(pc.make_model()).cuda().train()
        launches = image_pyramid.NATIVE_BF16_LAUNCHES[0]
        with image_pyramid.train_branch("native"), image_pyramid.image_precision(precision):
            calls = image_pyramid.NATIVE_TRAIN_CALLS[0]
            out = net(image)
            out.square().sum().backward()
            assert image_pyramid.NATIVE_TRAIN_CALLS[0] == calls + 1
        assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in net.parameters() if p.grad is not None])
    assert torch.equal(outs[0], outs[1])
    assert len(grads[0]) == len(grads[1]) > 0 and all(torch.equal(a, b) for a, b in zip(*grads))


# ------------------------------------------------------------------------------------------------ files to files
def _png(path, w, h, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([xx * 200.0 / w, yy * 200.0 / h, (xx + yy) * 100.0 / (w + h)], -1)
    Image.fromarray(np.clip(base + rng.normal(0, 25, (h, w, 3)), 0, 255).astype(np.uint8)).save(path)


def test_detect_runs_both_pyramids_in_bf16(tmp_path):
    """three committed KITTI frames in batches of two, set up as tests/test_image_pyramid.py does: one well-formed result file per
    frame, 2 pyramids x 2 batches x the routed layers of bf16 launches, the scope cells restored"""
    import detect_cases as DC
    from heterofusionrcnn_amd import image_pyramid, train_rcnn, train_rpn
    from heterofusionrcnn_amd.detect import detect, rpn_fts_channels
    root, names = str(tmp_path / "kitti"), list(DC.FRAMES)
    for d in ("calib", "label_2"):
        shutil.copytree(os.path.join(GOLD, d), os.path.join(root, d))
    os.makedirs(os.path.join(root, "velodyne"))
    os.makedirs(os.path.join(root, "image_2"))
    for i, (n, (w, h)) in enumerate(zip(names, DC.SIZES)):
        with lzma.open(os.path.join(GOLD, "velodyne", n + ".bin.xz")) as f, open(os.path.join(root, "velodyne", n + ".bin"), "wb") as g:
            g.write(f.read())
        _png(os.path.join(root, "image_2", n + ".png"), w, h, seed=i)
    with open(os.path.join(root, "val.txt"), "w") as f:
        f.write("\n".join(names) + "\n")
    img_conv = ((1, 16), (1, 16), (1, 16), (1, 16))
    torch.manual_seed(0)
    net, with_image = train_rpn.make_model("rpn_multiclass", img_conv)
    assert with_image
    trainer = train_rcnn.make_trainer(rpn_fts_channels(net.rpn), img_conv)
    n_layers = routed(net.img_net, torch.empty((2, 360, 1200, 3)))
    assert n_layers == 10 - 1                                  # the first layer of either pyramid stays on the fp32 kernel
    calls, launches = image_pyramid.NATIVE_CALLS[0], image_pyramid.NATIVE_BF16_LAUNCHES[0]
    written = detect(root, net, trainer, str(tmp_path / "bf16"), split="val", batch=2, seed=3, workers=2, score_threshold=0.0,
                     image_branch="native", image_precision="bf16")
    assert sorted(written) == names
    assert sorted(os.listdir(str(tmp_path / "bf16"))) == [n + ".txt" for n in names]
    assert image_pyramid.NATIVE_CALLS[0] == calls + 2 * 2
    assert image_pyramid.NATIVE_BF16_LAUNCHES[0] == launches + 2 * 2 * n_layers
    assert image_pyramid.image_branch_name() == "torch" and image_pyramid.image_precision_name() == "fp32"
    for n in names:
        rows = [l.split() for l in open(os.path.join(str(tmp_path / "bf16"), n + ".txt")) if l.strip()]
        assert len(rows) == written[n] and all(len(r) == 16 for r in rows)
