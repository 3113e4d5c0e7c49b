"""GPU tests of the reference's train op in optim.MultiTensorAdam (csrc/optim.hip: hf_adam_sqnorm_partials + hf_adam_multi_sched):
per-tensor clip_by_norm of the averaged gradient and tf.train.exponential_decay, held against an fp64 restatement of
TensorFlow's clip_by_norm followed by tf.train.AdamOptimizer; the schedule under a captured graph; determinism; the off
position against hf_adam_multi; the optimizer's state_dict."""
import numpy as np
import pytest
import torch

from heterofusionrcnn_amd import _lib
from heterofusionrcnn_amd._lib import check, ptr, stream_ptr
from heterofusionrcnn_amd.optim import MultiTensorAdam

pytestmark = pytest.mark.gpu

SHAPES = [(3,), (64, 3), (16385,), (257, 129), (1, 1), (40000,), (7, 5, 3), (512, 512)]   # chunk edges, odd lengths, unaligned slices
CLIP = 1.0
SCALE = 0.25                       # grad_scale: the 1 / world factor the clipped norm must include


def _params(seed, shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(s, generator=g).cuda().requires_grad_(True) for s in shapes]


def _norm_factor(i, step):
    """the L2 norm of tensor i's averaged gradient at a step, in units of CLIP: 0.3, 0.999, 1.001 and 50 times the clip norm, an
    all-zero tensor, and norms that move between steps (so that clipping changes Adam's trajectory, not only its scale)"""
    return [0.3 * (1 + 4 * (step % 2)), 0.999, 1.001, 50.0 * (1 + step), 0.0, 0.3, 50.0 * (1 + step % 3), 1.001 * (1 + 2 * (step % 2))][i]


def _gradients(shapes, steps, seed=11):
    gen = torch.Generator().manual_seed(seed)
    out = []
    for t in range(steps):
        gs = []
        for i, s in enumerate(shapes):
            g = torch.randn(s, generator=gen, dtype=torch.float64)
            f = _norm_factor(i, t) * CLIP
            g = g / g.norm() * f / SCALE if f > 0 else torch.zeros(s, dtype=torch.float64)
            gs.append(g.float())
        out.append(gs)
    return out


def _tf_reference(p0, grads, lr, b1=0.9, b2=0.999, eps=1e-8, clip=CLIP, decay=None):
    """fp64: x = grad_scale g; tf.clip_by_norm(x, clip) per tensor (clip None: no clipping); tf.train.AdamOptimizer with
    lr = exponential_decay(lr, t - 1, *decay) (staircase)"""
    ref = [p.detach().cpu().double().numpy().copy() for p in p0]
    m = [np.zeros_like(r) for r in ref]
    v = [np.zeros_like(r) for r in ref]
    for t, gs in enumerate(grads, start=1):
        lr_t = lr if decay is None else lr * decay[1] ** np.floor((t - 1) / decay[0])
        for i, g in enumerate(gs):
            x = g.double().numpy() * SCALE
            if clip is not None:
                norm = np.sqrt((x * x).sum())
                x = x * clip / max(norm, clip)
            m[i] = b1 * m[i] + (1 - b1) * x
            v[i] = b2 * v[i] + (1 - b2) * x * x
            ref[i] -= lr_t * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m[i] / (np.sqrt(v[i]) + eps)
    return ref


def _run(ps, opt, grads):
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        opt.step()
    torch.cuda.synchronize()


def _close(ps, ref):
    return all(np.allclose(p.detach().cpu().numpy(), r, rtol=3e-5, atol=3e-6) for p, r in zip(ps, ref))


def test_clipping_matches_tensorflow_clip_by_norm_then_adam():
    grads = _gradients(SHAPES, 8)
    ps = _params(3, SHAPES)
    ref = _tf_reference(ps, grads, lr=1e-2)
    opt = MultiTensorAdam(ps, lr=1e-2, tf_epsilon=True, grad_scale=SCALE, clip_norm=CLIP)
    _run(ps, opt, grads)
    for p, r in zip(ps, ref):
        np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=3e-5, atol=3e-6)
    # the all-zero tensor's moments stay zero (its gradient stayed zero through the clip)
    assert float(opt.exp_avg[4].abs().max()) == 0.0 and float(opt.exp_avg_sq[4].abs().max()) == 0.0
    # control: the same run without clipping misses the bound
    qs = _params(3, SHAPES)
    _run(qs, MultiTensorAdam(qs, lr=1e-2, tf_epsilon=True, grad_scale=SCALE), grads)
    assert not _close(qs, ref)
    assert _close(qs, _tf_reference(_params(3, SHAPES), grads, lr=1e-2, clip=None))


def test_clipping_skips_tensors_without_a_gradient():
    grads = _gradients(SHAPES, 3)
    ps = _params(4, SHAPES)
    before = ps[3].detach().clone()
    opt = MultiTensorAdam(ps, lr=1e-2, tf_epsilon=True, grad_scale=SCALE, clip_norm=CLIP)
    for gs in grads:
        for p, g in zip(ps, gs):
            p.grad = g.cuda()
        ps[3].grad = None
        opt.step()
    torch.cuda.synchronize()
    assert torch.equal(ps[3].detach(), before)
    ref = _tf_reference(_params(4, SHAPES), grads, lr=1e-2)          # per tensor: index 3 is not compared
    for i, (p, r) in enumerate(zip(ps, ref)):
        if i != 3:
            np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=3e-5, atol=3e-6)


def test_schedule_and_clipping_follow_the_replays_of_one_capture():
    """one captured step replayed 10 times, decay_steps 3, factor 0.5: the learning rate halves at global steps 3, 6, 9 with the
    kernel arguments frozen at capture"""
    shapes = SHAPES[:6]
    grads = _gradients(shapes, 10, seed=21)
    ps = _params(7, shapes)
    p0 = [p.detach().clone() for p in ps]
    slots = [torch.zeros(s, device="cuda") for s in shapes]          # the gradients at fixed addresses, refilled per replay
    for p, g in zip(ps, slots):
        p.grad = g
    opt = MultiTensorAdam(ps, lr=1e-2, tf_epsilon=True, grad_scale=SCALE, clip_norm=CLIP, lr_decay=(3, 0.5))
    assert [opt.lr_at(g) for g in (0, 2, 3, 5, 6, 9)] == pytest.approx([1e-2, 1e-2, 5e-3, 5e-3, 2.5e-3, 1.25e-3])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        snap = opt.snapshot()
        opt.step()                                                   # outside the capture first (table upload, lazy state)
        opt.restore(snap)
        for p, q in zip(ps, p0):
            p.data.copy_(q)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    for t, gs in enumerate(grads, start=1):
        for slot, g in zip(slots, gs):
            slot.copy_(g)
        graph.replay()
        torch.cuda.synchronize()
        ref = _tf_reference(p0, grads[:t], lr=1e-2, decay=(3, 0.5))
        for p, r in zip(ps, ref):
            np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=3e-5, atol=3e-6, err_msg="replay %d" % t)
    assert float(opt.step_count) == 10.0
    assert not _close(ps, _tf_reference(p0, grads, lr=1e-2, decay=None))          # a constant rate misses it


def test_same_gradients_same_bits():
    grads = _gradients(SHAPES, 4, seed=5)
    out = []
    for _ in range(2):
        ps = _params(9, SHAPES)
        _run(ps, MultiTensorAdam(ps, lr=1e-2, tf_epsilon=True, grad_scale=SCALE, clip_norm=CLIP, lr_decay=(2, 0.8)), grads)
        out.append([p.detach().clone() for p in ps])
    assert all(torch.equal(a, b) for a, b in zip(*out))


def _step_through_sched_entry(opt):
    """one step through hf_adam_multi_sched with clipping and decay off (what step() would launch if it took the new path)"""
    opt._refresh()
    opt.step_count.add_(1.0)
    check(_lib.lib().hf_adam_multi_sched(opt._chunks, ptr(opt._dev_table), ptr(opt._dev_map), ptr(opt.step_count), None, 0.0, opt.lr,
                                         0, 0.0, 0.0, opt.betas[0], opt.betas[1], opt.eps, opt.grad_scale, 0 if opt.tf_epsilon else 1,
                                         stream_ptr()), "adam_multi_sched")


@pytest.mark.parametrize("tf_epsilon", [True, False])
def test_off_is_hf_adam_multi_bit_for_bit(tf_epsilon):
    grads = _gradients(SHAPES, 5, seed=8)
    a, b = _params(2, SHAPES), _params(2, SHAPES)
    oa = MultiTensorAdam(a, lr=3e-3, tf_epsilon=tf_epsilon, grad_scale=SCALE)
    ob = MultiTensorAdam(b, lr=3e-3, tf_epsilon=tf_epsilon, grad_scale=SCALE)
    for gs in grads:
        for pa, pb, g in zip(a, b, gs):
            pa.grad, pb.grad = g.cuda(), g.cuda()
        oa.step()
        _step_through_sched_entry(ob)
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    assert torch.equal(oa._exp_avg, ob._exp_avg) and torch.equal(oa._exp_avg_sq, ob._exp_avg_sq)


def test_state_dict_round_trip_continues_bit_for_bit(tmp_path):
    grads = _gradients(SHAPES, 6, seed=13)
    kw = dict(lr=1e-2, tf_epsilon=True, grad_scale=SCALE, clip_norm=CLIP, lr_decay=(2, 0.8))
    a = _params(6, SHAPES)
    oa = MultiTensorAdam(a, **kw)
    _run(a, oa, grads[:4])
    path = str(tmp_path / "opt.pt")
    torch.save({"opt": oa.state_dict(), "params": [p.detach().cpu() for p in a]}, path)
    _run(a, oa, grads[4:])
    saved = torch.load(path, map_location="cpu")
    b = [p.cuda().requires_grad_(True) for p in saved["params"]]
    ob = MultiTensorAdam(b, lr=5.0, grad_scale=SCALE)      # the hyper-parameters come from the state; grad_scale is the exchange's
    ob.load_state_dict(saved["opt"])
    assert float(ob.step_count) == 4.0 and ob.clip_norm == CLIP and ob.lr_decay == (2.0, 0.8, True) and ob.lr == pytest.approx(1e-2)
    _run(b, ob, grads[4:])
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    # a different parameter list is refused
    with pytest.raises(ValueError, match="tensors"):
        MultiTensorAdam(_params(6, SHAPES[:-1]), **kw).load_state_dict(saved["opt"])
    with pytest.raises(ValueError, match="tensors"):
        MultiTensorAdam(_params(6, SHAPES[:-1] + [(512, 511)]), **kw).load_state_dict(saved["opt"])
