"""mlp.training_precision("bf16") on the device: linear_nobias with autograd on against the fp64 emulation with bf16-rounded operands
(the bounds of tests/linear_bf16_cases.py and tests/linear_bf16_train_cases.py), Dense and SeparableK in training mode against a torch
op-by-op emulation, the layers and modes that must stay fp32, a weight that changes between two steps (eagerly and inside a replayed
graph), and the small model of tests/test_graph_step.py: captured against eager steps, and twenty steps on one batch.  The routing
constants are lowered by monkeypatch so that the small shapes used here take the kernels."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as lc  # noqa: E402
import linear_bf16_train_cases as tc  # noqa: E402
from test_graph_step import _frames, _small_multiclass  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture
def low_thresholds(monkeypatch):
    from heterofusionrcnn_amd import mlp
    monkeypatch.setattr(mlp, "BF16_TRAIN_MIN_ROWS", 1)
    monkeypatch.setattr(mlp, "BF16_TRAIN_MIN_COUT", 4)
    monkeypatch.setattr(mlp, "BF16_TRAIN_MIN_CIN", 32)
    assert mlp.training_precision_name() == "fp32" and mlp.inference_precision_name() == "fp32"
    return mlp


def _routed(mlp, fn):
    before, before_eval = mlp.BF16_TRAIN_ROUTED_CALLS[0], mlp.BF16_ROUTED_CALLS[0]
    out = fn()
    assert mlp.BF16_ROUTED_CALLS[0] == before_eval          # the inference route is never taken here
    return out, mlp.BF16_TRAIN_ROUTED_CALLS[0] - before


def _inside(got, ref, err, name):
    diff = (got.detach().cpu().double() - ref).abs()
    ratio = float((diff / err.clamp(min=1e-300)).max())
    print("%s: max |got - ref64| / bound = %.3g" % (name, ratio))
    assert bool((diff <= err).all()), (name, ratio)


@pytest.mark.parametrize("rows,cin,cout", [(257, 36, 260), (300, 260, 36), (2304, 132, 68)])
def test_linear_nobias_three_products_against_the_fp64_emulation(low_thresholds, rows, cin, cout):
    mlp = low_thresholds
    gen = torch.Generator().manual_seed(rows + cin * 1000 + cout)
    x = (torch.randn(rows, cin, generator=gen) + 0.3).cuda().requires_grad_(True)
    w = (torch.randn(cout, cin, generator=gen) * 0.5).cuda().requires_grad_(True)
    go = (torch.randn(rows, cout, generator=gen) * 0.5).cuda()

    def run(**kw):
        z = mlp.linear_nobias(x, w, **kw)
        dx, dw = torch.autograd.grad(z, (x, w), go)
        return z, dx, dw

    with mlp.training_precision("bf16"):
        (z, dx, dw), n = _routed(mlp, lambda: run(allow_bf16=True))
        _, n_refused = _routed(mlp, run)                     # the caller did not allow it
        with torch.no_grad():
            _, n_nograd = _routed(mlp, lambda: mlp.linear_nobias(x, w, allow_bf16=True))
    assert (n, n_refused, n_nograd) == (1, 0, 0)
    assert getattr(w, "_hf_bf16", None) is None              # the inference cache is neither read nor written
    xc, wc, gc = x.detach().cpu(), w.detach().cpu(), go.cpu()
    fz = lc.reference(dict(x=xc, w=wc, bias=None, bn=None), 0)
    _inside(z, fz["y"], fz["err"], "z")
    fdx = lc.reference(dict(x=gc, w=wc.t().contiguous(), bias=None, bn=None), 0)      # dx = bf16(g) bf16(W): the emulation rounds g too
    _inside(dx, fdx["y"], fdx["err"], "dx")
    fdw = tc.reference(dict(g=gc, x=xc))
    _inside(dw, fdw["dw"], fdw["err"], "dW")
    # fp32: nothing routed, and the permission changes no bit of today's path
    (z32, dx32, dw32), n32 = _routed(mlp, lambda: run(allow_bf16=True))
    base = run()
    assert n32 == 0 and torch.equal(z32, base[0]) and torch.equal(dx32, base[1]) and torch.equal(dw32, base[2])
    assert not torch.equal(z32, z)


class _EmulatedLinear(torch.autograd.Function):
    """the three products op by op: operands rounded to bf16 (the gradient too), multiplied in fp32"""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _r(x) @ _r(w).t()

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        x2, g2 = x.reshape(-1, x.shape[-1]), g.reshape(-1, g.shape[-1])
        return (_r(g2) @ _r(w)).reshape(x.shape), _r(g2).t() @ _r(x2)


def _r(t):
    return t.to(torch.bfloat16).float()


def _elu_bn(z, post):
    z2 = F.elu(z) if post.activation else z
    flat = z2.reshape(-1, z2.shape[-1])
    mu, var = flat.mean(0), flat.var(0, unbiased=False)
    return (z2 - mu) / torch.sqrt(var + 1e-3) * post.bn.weight + post.bn.bias


def _close(name, a, b):
    d = (a - b).detach().abs()
    print("%s: kernel vs emulation max |d| = %.3g (max |ref| %.3g)" % (name, float(d.max()), float(b.detach().abs().max())))
    assert bool((d <= 2e-3 + 5e-3 * b.abs()).all()), name


def _randomise_affine(bn, gen):
    with torch.no_grad():
        bn.weight.copy_((torch.randn(bn.num_features, generator=gen) * 0.5 + 1.0).cuda())
        bn.bias.copy_(torch.randn(bn.num_features, generator=gen).cuda())


@pytest.mark.parametrize("cin,cout", [(36, 260), (260, 36)])
def test_dense_in_training_mode_against_the_op_by_op_emulation(low_thresholds, cin, cout):
    mlp = low_thresholds
    from heterofusionrcnn_amd.pointcnn import Dense
    gen = torch.Generator().manual_seed(cin * 1000 + cout)
    torch.manual_seed(cin)
    d = Dense(cin, cout).cuda().train()
    _randomise_affine(d.post.bn, gen)
    x = (torch.randn(4, 75, cin, generator=gen) + 0.3).cuda().requires_grad_(True)
    go = torch.randn(4, 75, cout, generator=gen).cuda()
    params = list(d.parameters())
    with mlp.training_precision("bf16"):
        out, n = _routed(mlp, lambda: d(x))
        grads = torch.autograd.grad(out, [x] + params, go)
    assert n == 1 and out.shape == (4, 75, cout)
    ref = _elu_bn(_EmulatedLinear.apply(x, d.linear.weight), d.post)
    ref_grads = torch.autograd.grad(ref, [x] + params, go)
    _close("dense output", out, ref)
    for name, a, b in zip(["x"] + [nm for nm, _ in d.named_parameters()], grads, ref_grads):
        _close("dense grad " + name, a, b)


def test_separable_k_in_training_mode_against_the_op_by_op_emulation(low_thresholds):
    mlp = low_thresholds
    from heterofusionrcnn_amd import pointcnn
    gen = torch.Generator().manual_seed(5)
    torch.manual_seed(5)
    k, cin, mult, cout = 4, 36, 2, 132
    s = pointcnn.SeparableK(k, cin, cout, mult).cuda().train()
    _randomise_affine(s.post.bn, gen)
    x = torch.randn(1, 257, k, cin, generator=gen).cuda().requires_grad_(True)
    go = torch.randn(1, 257, cout, generator=gen).cuda()
    params = list(s.parameters())
    with mlp.training_precision("bf16"):
        out, n = _routed(mlp, lambda: s(x))
        grads = torch.autograd.grad(out, [x] + params, go)
    assert n == 1 and out.shape == (1, 257, cout)
    y = torch.einsum("bpkc,kcm->bpcm", x, s.depthwise).reshape(1, 257, cin * mult)
    ref = _elu_bn(_EmulatedLinear.apply(y, s.pointwise.weight), s.post)
    ref_grads = torch.autograd.grad(ref, [x] + params, go)
    _close("separable output", out, ref)
    for name, a, b in zip(["x"] + [nm for nm, _ in s.named_parameters()], grads, ref_grads):
        _close("separable grad " + name, a, b)


def test_layers_and_modes_that_stay_fp32(low_thresholds):
    mlp = low_thresholds
    from heterofusionrcnn_amd import pointcnn
    torch.manual_seed(13)
    head = pointcnn.Dense(36, 68, allow_bf16=False).cuda().train()
    d, s = pointcnn.Dense(36, 68).cuda(), pointcnn.SeparableK(4, 36, 68, 1).cuda()
    x = torch.randn(257, 36, device="cuda", requires_grad=True)
    xs = torch.randn(1, 257, 4, 36, device="cuda")
    base = head(x)
    with mlp.training_precision("bf16"):
        y, n = _routed(mlp, lambda: head(x))                  # a layer built with allow_bf16=False
        assert n == 0 and torch.equal(y.detach(), base.detach())   # batch statistics do not depend on the running estimates
        y.sum().backward()
        for m in (d, s):
            m.eval()
        _, n = _routed(mlp, lambda: (d(x), s(xs)))            # eval mode under the TRAINING switch alone: fp32, autograd on or off
        assert n == 0
        with torch.no_grad():
            _, n = _routed(mlp, lambda: (d(x), s(xs)))
        assert n == 0
        for m in (d, s):
            m.train()
        _, n = _routed(mlp, lambda: (d(x), s(xs)))
        assert n == 2
        with torch.no_grad():                                  # training mode without autograd: nothing to train
            _, n = _routed(mlp, lambda: (d(x), s(xs)))
        assert n == 0
    with mlp.inference_precision("bf16"):                     # the inference switch alone never changes a training step
        _, n = _routed(mlp, lambda: (d(x), s(xs)))
    assert n == 0
    narrow = pointcnn.Dense(28, 68).cuda().train()            # cin < 32 stays fp32 whatever the thresholds
    with mlp.training_precision("bf16"):
        _, n = _routed(mlp, lambda: narrow(torch.randn(257, 28, device="cuda")))
    assert n == 0


def test_a_weight_updated_between_two_steps_is_seen(low_thresholds):
    mlp = low_thresholds
    torch.manual_seed(11)
    w = (torch.randn(68, 36, device="cuda") * 0.5).requires_grad_(True)
    x = torch.randn(257, 36, device="cuda", requires_grad=True)
    go = torch.randn(257, 68, device="cuda")

    def step(inp, weight):
        z = mlp.linear_nobias(inp, weight, allow_bf16=True)
        dx, dw = torch.autograd.grad(z, (inp, weight), go)
        return z, dx, dw

    with mlp.training_precision("bf16"):
        (z0, dx0, dw0), n = _routed(mlp, lambda: step(x, w))
        assert n == 1 and getattr(w, "_hf_bf16", None) is None
        with torch.no_grad():
            w.mul_(2.0)                                      # doubling is exact in bf16 and in fp32
        z1, dx1, dw1 = step(x, w)
        assert torch.equal(z1, 2 * z0) and torch.equal(dx1, 2 * dx0) and torch.equal(dw1, dw0)
        # inside a captured graph the conversions are nodes: a replay sees the new weight.  The captured leaves are new tensors
        # whose first use is the warm-up on the capturing stream (PyTorch's recipe: autograd ties a leaf to the stream of its first
        # use, and a leaf first used on the default stream would draw that stream into the capture)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            static_x, static_w = x.detach().clone().requires_grad_(True), w.detach().clone().requires_grad_(True)
            step(static_x, static_w)
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = step(static_x, static_w)
        graph.replay()
        first = [t.clone() for t in out]
        assert all(torch.equal(a, b) for a, b in zip(first, (z1, dx1, dw1)))
        with torch.no_grad():
            static_w.mul_(0.5)
        graph.replay()
        assert torch.equal(out[0], z0) and torch.equal(out[1], dx0) and torch.equal(out[2], dw0)
    assert getattr(static_w, "_hf_bf16", None) is None


def _small_model_losses(mlp, precision, graph, steps, seed=4):
    from heterofusionrcnn_amd import rpn as R_
    from heterofusionrcnn_amd.graph_step import TrainStep
    cfg = _small_multiclass()
    inp = _frames(cfg, 2, 2048, seed=0)
    torch.manual_seed(seed)
    model = R_.RpnModel(cfg).cuda().train()
    opt = torch.optim.Adam(model.parameters(), lr=2e-3, fused=True, capturable=True)
    geo = model.geometry(inp["xyz"])
    with mlp.training_precision(precision):
        before = mlp.BF16_TRAIN_ROUTED_CALLS[0]
        step = TrainStep(model, opt, inp, geo, world=1, graph=graph, warmup=3 if graph else 0)
        losses = [float(step(geometry=geo)) for _ in range(steps)]
        routed = mlp.BF16_TRAIN_ROUTED_CALLS[0] - before
    assert (step.graph is not None) == graph
    return np.array(losses), routed


def test_captured_step_matches_eager_steps_under_bf16(low_thresholds):
    """the criterion tests/test_graph_step.py applies to the first three fp32 steps (the scatter gradients use atomics: rounding, not
    bits)"""
    mlp = low_thresholds
    e, n_eager = _small_model_losses(mlp, "bf16", False, 3)
    g, n_graph = _small_model_losses(mlp, "bf16", True, 3)
    print("eager", e.tolist(), "graph", g.tolist(), "routed launches", n_eager, n_graph)
    assert n_eager > 0 and n_eager % 3 == 0 and n_graph > 0
    assert np.all(np.isfinite(e)) and np.all(np.isfinite(g))
    np.testing.assert_allclose(g, e, rtol=1e-4)


def test_twenty_steps_on_one_batch(low_thresholds):
    mlp = low_thresholds
    fp32, n32 = _small_model_losses(mlp, "fp32", True, 20)
    bf16, n16 = _small_model_losses(mlp, "bf16", True, 20)
    assert n32 == 0 and n16 > 0
    print("fp32 loss curve: %s" % ", ".join("%.5f" % v for v in fp32))
    print("bf16 loss curve: %s" % ", ".join("%.5f" % v for v in bf16))
    print("max |bf16 - fp32| / fp32 over the twenty steps: %.3g (reported, not asserted)" % float(np.max(np.abs(bf16 - fp32) / fp32)))
    assert np.all(np.isfinite(bf16))
    assert bf16[-1] < bf16[0]
