"""mlp.inference_precision("bf16") on the device: the routed layers against the fp64 emulation with bf16-rounded operands (the bound of
tests/linear_bf16_cases.py), the per-weight bf16 cache, the guarantee that training mode and autograd never see the switch, and a small
RCNN against the same model with the wrapper replaced by a torch emulation.  The routing constants are lowered by monkeypatch so that
the small shapes used here take the kernel."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import linear_bf16_cases as lc  # noqa: E402

pytestmark = pytest.mark.gpu

ROWS = 257


@pytest.fixture
def low_thresholds(monkeypatch):
    from heterofusionrcnn_amd import mlp
    monkeypatch.setattr(mlp, "BF16_MIN_ROWS", 1)
    monkeypatch.setattr(mlp, "BF16_MIN_COUT", 4)
    assert mlp.inference_precision_name() == "fp32"
    return mlp


def _bn_tuple(bn):
    return (bn.weight.detach().cpu(), bn.bias.detach().cpu(), bn.running_mean.cpu(), bn.eval_invstd().cpu())


def _randomise(bn, g):
    with torch.no_grad():
        bn.weight.copy_(torch.randn(bn.num_features, generator=g) * 0.5 + 1.0)
        bn.bias.copy_(torch.randn(bn.num_features, generator=g))
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 4 + 0.5)


def _within(got, t, mode, name):
    ref = lc.reference(t, mode)
    diff = (got.detach().cpu().double() - ref["y"]).abs()
    ratio = float((diff / ref["err"].clamp(min=1e-300)).max())
    print("%s: max |got - ref64| / bound = %.3g" % (name, ratio))
    assert bool((diff <= ref["err"]).all()), (name, ratio)


def _routed(mlp, fn):
    before = mlp.BF16_ROUTED_CALLS[0]
    out = fn()
    return out, mlp.BF16_ROUTED_CALLS[0] - before


@pytest.mark.parametrize("activation", [True, False], ids=["elu", "no_activation"])
@pytest.mark.parametrize("cin,cout", [(36, 260), (260, 36), (132, 68)])
def test_dense_against_the_fp64_emulation(low_thresholds, activation, cin, cout):
    mlp = low_thresholds
    from heterofusionrcnn_amd.pointcnn import Dense
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    d = Dense(cin, cout, activation=activation).cuda().eval()
    _randomise(d.post.bn, g)
    x = (torch.randn(ROWS, cin, generator=g) + 0.3).cuda()
    with torch.no_grad(), mlp.inference_precision("bf16"):
        y, n = _routed(mlp, lambda: d(x))
    assert n == 1 and y.shape == (ROWS, cout)
    _within(y, dict(x=x.cpu(), w=d.linear.weight.detach().cpu(), bias=None, bn=_bn_tuple(d.post.bn)), 2 if activation else 0, "dense")
    with torch.no_grad():
        y32, n = _routed(mlp, lambda: d(x))
    assert n == 0 and not torch.equal(y32, y)
    # a 3-D input keeps its leading dimensions
    with torch.no_grad(), mlp.inference_precision("bf16"):
        assert torch.equal(d(x[:256].view(4, 64, cin)), y[:256].view(4, 64, cout))


def test_separable_k_pointwise_half(low_thresholds):
    mlp = low_thresholds
    from heterofusionrcnn_amd import pointcnn
    g = torch.Generator().manual_seed(5)
    k, cin, mult, cout = 4, 36, 2, 132
    s = pointcnn.SeparableK(k, cin, cout, mult).cuda().eval()
    _randomise(s.post.bn, g)
    x = torch.randn(1, ROWS, k, cin, generator=g).cuda()
    with torch.no_grad():
        d = pointcnn.depthwise_k(x, s.depthwise)              # fp32, untouched by the switch
        with mlp.inference_precision("bf16"):
            y, n = _routed(mlp, lambda: s(x))
            assert torch.equal(pointcnn.depthwise_k(x, s.depthwise), d)
    assert n == 1 and y.shape == (1, ROWS, cout)
    _within(y.view(ROWS, cout), dict(x=d.reshape(ROWS, cin * mult).cpu(), w=s.pointwise.weight.detach().cpu(), bias=None, bn=_bn_tuple(s.post.bn)),
            2, "separable")


@pytest.mark.parametrize("pool_k", [0, 1])
def test_two_layer_shared_mlp(low_thresholds, pool_k):
    """each layer against the emulation fed with what the layer before produced (the first layer run alone gives the same bits);
    pool_k: the last layer leaves its normalisation to the pooling kernel"""
    mlp = low_thresholds
    from heterofusionrcnn_amd.modules import SharedMLPLayer
    g = torch.Generator().manual_seed(7)
    l1, l2 = SharedMLPLayer(36, 260).cuda().eval(), SharedMLPLayer(260, 68).cuda().eval()
    for l in (l1, l2):
        _randomise(l.bn, g)
        with torch.no_grad():
            l.fc.bias.copy_(torch.randn(l.fc.out_features, generator=g))
    x = (torch.randn(ROWS, 36, generator=g) + 0.3).cuda()
    with torch.no_grad(), mlp.inference_precision("bf16"):
        y1, n1 = _routed(mlp, lambda: mlp.shared_mlp([l1], x))
        y2, n2 = _routed(mlp, lambda: mlp.shared_mlp([l1, l2], x, pool_k=pool_k))
    assert (n1, n2) == (1, 2)
    par = lambda l: dict(w=l.fc.weight.detach().cpu(), bias=l.fc.bias.detach().cpu(), bn=_bn_tuple(l.bn))
    _within(y1, dict(x=x.cpu(), **par(l1)), 1, "layer 1")
    _within(y2, dict(x=y1.cpu(), **par(l2)), 1, "layer 2")


def test_weight_cache_follows_the_weight(low_thresholds):
    mlp = low_thresholds
    from heterofusionrcnn_amd.pointcnn import Dense
    torch.manual_seed(11)
    d = Dense(36, 68).cuda().eval()
    x = torch.randn(ROWS, 36, device="cuda")
    with torch.no_grad(), mlp.inference_precision("bf16"):
        y0 = d(x)
        held = d.linear.weight._hf_bf16[1]
        assert torch.equal(d(x), y0) and d.linear.weight._hf_bf16[1] is held        # reused
        d.linear.weight.mul_(2.0)                                                   # in place: the version moves
        y1 = d(x)
        assert not torch.equal(y1, y0)
        state = {k: v.clone() for k, v in d.state_dict().items()}
        state["linear.weight"] = state["linear.weight"] * 0.5
        d.load_state_dict(state)
        assert torch.equal(d(x), y0)                                                # halving and doubling are exact
    # under stream capture nothing is cached, and the conversion is a node of the graph: a replay sees the new weight
    d2 = Dense(36, 68).cuda().eval()
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), mlp.inference_precision("bf16"):
        d2.post.bn.eval_invstd()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            out = d2(static_x)
        assert getattr(d2.linear.weight, "_hf_bf16", None) is None
        graph.replay()
        first = out.clone()
        assert torch.equal(first, d2(static_x))
        d2.linear.weight.mul_(2.0)
        graph.replay()
        assert torch.equal(out, d2(static_x)) and not torch.equal(out, first)


def test_training_mode_and_autograd_never_see_the_switch(low_thresholds):
    mlp = low_thresholds
    from heterofusionrcnn_amd import pointcnn
    from heterofusionrcnn_amd.modules import SharedMLPLayer
    torch.manual_seed(13)
    d, s = pointcnn.Dense(36, 68).cuda(), pointcnn.SeparableK(4, 36, 68, 1).cuda()
    layers = [SharedMLPLayer(36, 132).cuda(), SharedMLPLayer(132, 68).cuda()]
    x = torch.randn(ROWS, 36, device="cuda")
    xs = torch.randn(1, ROWS, 4, 36, device="cuda")

    def everything():
        out = {}
        for m in [d, s] + layers:
            m.eval()
        out["eval_grad"] = (d(x), s(xs), mlp.shared_mlp(layers, x))               # frozen BatchNorm inside a model that trains
        with torch.no_grad():
            out["eval_nograd"] = (d(x), s(xs), mlp.shared_mlp(layers, x))
        for m in [d, s] + layers:
            m.train()
        state = [{k: v.clone() for k, v in m.state_dict().items()} for m in [d, s] + layers]
        with torch.no_grad():
            out["train_nograd"] = (d(x), s(xs), mlp.shared_mlp(layers, x))
        for m, st in zip([d, s] + layers, state):                                  # running statistics back where they were
            m.load_state_dict(st)
        out["train_grad"] = (d(x), s(xs), mlp.shared_mlp(layers, x))
        for m, st in zip([d, s] + layers, state):
            m.load_state_dict(st)
        return out

    base, n = _routed(mlp, everything)
    assert n == 0
    with mlp.inference_precision("fp32"):
        off, n = _routed(mlp, everything)
    assert n == 0
    with mlp.inference_precision("bf16"):
        on, n = _routed(mlp, everything)
    assert n == 4                                                                  # eval + no_grad only: Dense, SeparableK, two MLP layers
    for key in base:
        for a, b, c in zip(base[key], off[key], on[key]):
            assert torch.equal(a, b), key
            assert torch.equal(a, c) == (key != "eval_nograd"), key
    with mlp.inference_precision("bf16"):           # backward still runs under the switch
        for m in (d, s):
            m.train()
        loss = d(x).sum() + s(xs).sum()
        loss.backward()
    assert d.linear.weight.grad is not None and s.pointwise.weight.grad is not None and torch.isfinite(d.linear.weight.grad).all()


# ------------------------------------------------------------------------------------------------ a small RCNN
def _rcnn_inputs(seed, rois):
    """the smallest second stage tests/test_rcnn.py builds (RcnnModel(), one frame of 16384 points) with a few RoIs on the points"""
    g = torch.Generator().manual_seed(seed)
    n = 16384
    xyz = torch.stack([torch.rand(n, generator=g) * 40 - 20, torch.rand(n, generator=g) * 2.5 - 1.0, torch.rand(n, generator=g) * 55 + 5], dim=1)
    prop = torch.zeros(1, rois, 7)
    prop[0, :, 0] = torch.linspace(-12, 12, rois)
    prop[0, :, 1] = 1.5
    prop[0, :, 2] = torch.linspace(12, 50, rois)
    prop[0, :, 3:6] = torch.tensor([3.9, 1.6, 1.5])
    calib = torch.tensor([[721.5377, 0.0, 609.5593, 44.85728], [0.0, 721.5377, 172.854, 0.2163791], [0.0, 0.0, 1.0, 0.002745884]])
    return dict(xyz=xyz[None].cuda(), fts=torch.randn(1, n, 288, generator=g).cuda(), inten=(torch.rand(1, n, 1, generator=g) - 0.5).cuda(),
                fg=(torch.rand(1, n, generator=g) < 0.3).cuda(), prop=prop.cuda(), img=torch.randn(1, 360, 1200, 32, generator=g).cuda(),
                calib=calib[None].cuda())


def _emulation(calls):
    def linear_bf16_emulated(x, weight, bias, bn, mode):
        """operands rounded to bf16, fp32 matmul, the epilogue's formula"""
        calls.append(weight)
        z = x.to(torch.bfloat16).float() @ weight.detach().to(torch.bfloat16).float().t()
        if bias is not None:
            z = z + bias
        if bn is None:
            return z
        if mode & 2:
            z = torch.where(z > 0, z, torch.exp(z) - 1.0)
        y = (bn.weight * bn.eval_invstd()) * (z - bn.running_mean) + bn.bias
        return torch.relu(y) if mode & 1 else y
    return linear_bf16_emulated


def test_small_rcnn_against_the_torch_emulation(low_thresholds, monkeypatch):
    mlp = low_thresholds
    from heterofusionrcnn_amd import pointcnn, rcnn as RC
    torch.manual_seed(4)
    m = RC.RcnnModel().cuda().eval()
    g = torch.Generator().manual_seed(5)
    for mod in m.modules():                      # running statistics of a trained model are not (0, 1)
        if isinstance(mod, mlp.BatchNormReLU):
            with torch.no_grad():
                mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
    t = _rcnn_inputs(4, 4)
    args = (t["xyz"], t["fts"], t["inten"], t["fg"], t["prop"], t["img"], t["calib"])
    real = mlp.linear_bf16_eval
    routed = []

    def recording(x, weight, bias, bn, mode):
        routed.append(weight)
        return real(x, weight, bias, bn, mode)

    with torch.no_grad():
        cls32, reg32, pool = m(*args)
        assert int(pool["non_empty"].sum()) == 4
        with mlp.inference_precision("bf16"):
            monkeypatch.setattr(mlp, "linear_bf16_eval", recording)
            monkeypatch.setattr(pointcnn, "linear_bf16_eval", recording)
            (cls16, reg16, _), n = _routed(mlp, lambda: m(*args))
            emulated = []
            monkeypatch.setattr(mlp, "linear_bf16_eval", _emulation(emulated))
            monkeypatch.setattr(pointcnn, "linear_bf16_eval", _emulation(emulated))
            (cls_e, reg_e, _), n_e = _routed(mlp, lambda: m(*args))
    assert n > 0 and n == len(routed) == len(emulated) and n_e == 0
    assert all(a is b for a, b in zip(routed, emulated))
    # the excluded layers: the output heads, the 6-channel local MLP input, the coordinate branches and the lifting chain (cin < 32)
    ids = {id(w) for w in routed}
    assert id(m.reg_out.linear.weight) not in ids and id(m.cls_logits.weight) not in ids and id(m.mlp.layers[0].linear.weight) not in ids
    assert all(w.shape[1] >= 32 for w in routed)
    for xc in m.encoder.enc:
        assert id(xc.lift0.linear.weight) not in ids and id(xc.lift1.linear.weight) not in ids and id(xc.x0.linear.weight) not in ids
        assert id(xc.conv.pointwise.weight) in ids
    last = m.encoder.enc[-1]
    assert id(last.g0.linear.weight) not in ids and id(last.g1.linear.weight) not in ids
    assert id(m.cls_fc.layers[0].linear.weight) in ids and id(m.reg_fc.layers[0].linear.weight) in ids
    # kernel against emulation: summation order only -- the tolerance of tests/test_graph_step.py for op-by-op forms
    for name, a, b in (("cls_logits", cls16, cls_e), ("reg", reg16, reg_e)):
        d = (a - b).abs()
        print("%s: kernel vs emulation max |d| = %.3g" % (name, float(d.max())))
        assert bool((d <= 2e-3 + 5e-3 * b.abs()).all()), name
    # drift against fp32: reported, not asserted (untrained weights)
    print("bf16 vs fp32 head outputs: max |d cls_logits| = %.4g (max |cls| %.4g), max |d reg| = %.4g (max |reg| %.4g)" % (
        float((cls16 - cls32).abs().max()), float(cls32.abs().max()), float((reg16 - reg32).abs().max()), float(reg32.abs().max())))
