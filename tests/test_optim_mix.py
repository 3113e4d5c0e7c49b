"""GPU tests of optim.MultiTensorAdam's bookkeeping: eager steps, captures and graph replays mixed on ONE optimizer, the scenarios of
tests/optim_mix_cases.py.  After every operation every parameter is held against the fp64 reference (rtol 3e-5, atol 3e-6: this
optimizer's tolerance against fp64 in tests/test_train_op.py and tests/test_optim.py), the device step counter against the number of
steps, a tensor without a gradient against its own bits, and the optimizer's count of host uploads against the documented cache rule.
tests/test_optim_mix_cases_cpu.py shows that a step which launched on the other form's table misses that tolerance a hundredfold.

Every gradient tensor, slot, graph and optimizer stays alive until the last synchronise: a wrong table still points at live memory, so
these tests fail on numbers, never on a fault."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_mix_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu

_RIGHT = {}


def _right(name):
    if name not in _RIGHT:
        _RIGHT[name] = mc.trajectories(name)[0]
    return _RIGHT[name]


def _key(ps):
    return tuple(p.grad.data_ptr() if p.grad is not None else 0 for p in ps)


def _run(name):
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    sc = mc.SCENARIOS[name]
    hyper, right, recs = sc["hyper"], _right(name), mc.walk(name)
    value = lambda seed, i: torch.from_numpy(np.array(mc.gradient(seed, i, hyper)))
    ps = [torch.from_numpy(a).cuda().requires_grad_(True) for a in mc.initial_params()]
    opt = MultiTensorAdam(ps, **hyper)
    slots = [torch.zeros(s, device="cuda") for s in mc.SHAPES]               # the eager steps' static gradients
    keep, graphs, saved = [slots], {}, None                                  # keep: everything a table may point at

    if sc["grads"] == "pool":                                                # lazy initialisations of the backward pass, outside any capture
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            sum((p * g).sum() for p, g in zip(ps, slots)).backward()
            for p in ps:
                p.grad = None
        torch.cuda.current_stream().wait_stream(s)

    for k, (op, rec) in enumerate(zip(sc["ops"], recs)):
        what = "operation %d (%s%s)" % (k, op.kind, " " + op.graph if op.graph else "")
        before = [p.detach().clone() for p in ps]
        live = mc.ALL
        if op.kind == "eager":
            live = op.live
            for i, p in enumerate(ps):
                if i not in op.live:
                    p.grad = None
                elif op.where == "slots":
                    slots[i].copy_(value(op.seed, i))
                    p.grad = slots[i]
                else:
                    p.grad = value(op.seed, i).cuda()
            keep.append([p.grad for p in ps])
            opt.step()
        elif op.kind == "capture":
            graph = torch.cuda.CUDAGraph()
            if sc["grads"] == "slots":
                for i, p in enumerate(ps):
                    p.grad = slots[i] if i in op.live else None
                inputs = slots
                if "capture_on_matching_key" in rec["tags"]:
                    assert _key(ps) == opt._key, "the key does not match at the capture: the scenario misses its path"
                with torch.cuda.graph(graph):
                    opt.step()
            else:
                inputs = [torch.zeros(s, device="cuda") for s in mc.SHAPES]
                with torch.cuda.graph(graph):
                    for p in ps:
                        p.grad = None
                    sum((ps[i] * inputs[i]).sum() for i in op.live).backward()
                    opt.step()
                assert all((p.grad is not None) == (i in op.live) for i, p in enumerate(ps))
            keep.append([inputs, [p.grad for p in ps]])
            graphs[op.graph] = (graph, inputs, op.live, [p.grad for p in ps])
        elif op.kind == "replay":
            graph, inputs, live, _ = graphs[op.graph]
            for i in live:
                inputs[i].copy_(value(op.seed, i))
            graph.replay()
        elif op.kind == "save":
            saved = (opt.state_dict(), [p.detach().clone() for p in ps])
        elif op.kind == "load":
            opt.load_state_dict(saved[0])
            with torch.no_grad():
                for p, q in zip(ps, saved[1]):
                    p.copy_(q)
        torch.cuda.synchronize()
        if op.kind == "replay" and sc["grads"] == "pool":                    # the captured backward left the slot's bits in the graph's pool
            assert all(torch.equal(graphs[op.graph][3][i], inputs[i]) for i in live), what
        for i, (p, r) in enumerate(zip(ps, right[k])):
            np.testing.assert_allclose(p.detach().cpu().numpy(), r, rtol=mc.RTOL, atol=mc.ATOL, err_msg="%s, tensor %d" % (what, i))
        assert float(opt.step_count) == rec["steps"], what
        if op.kind in ("eager", "replay"):
            for i in mc.ALL:
                assert (i in live) or torch.equal(ps[i].detach(), before[i]), "%s: tensor %d has no gradient and moved" % (what, i)
        elif op.kind != "load":
            assert all(torch.equal(p.detach(), b) for p, b in zip(ps, before)), "%s changed a parameter" % what
        assert opt.table_uploads == rec["uploads"], "%s: %d uploads from the host, the cache rule gives %d" % (what, opt.table_uploads, rec["uploads"])
    return opt, keep, graphs


def test_eager_replay_eager():
    """an eager step after a replay finds its key unchanged: it must still update from ITS gradients, not from the graph's pool"""
    _run("eager_replay_eager")


def test_capture_on_matching_key():
    """a capture whose key matches records its own upload all the same: a later eager step with one tensor less, or with gradients
    elsewhere, changes nothing a replay does"""
    _run("capture_on_matching_key")


def test_two_captures():
    """two graphs with different tensor sets (different chunk counts frozen in) and eager steps between their replays"""
    _run("two_captures")


def test_sched():
    """the clipped, scheduled route (hf_adam_sqnorm_partials + hf_adam_multi_sched) through the same mix"""
    _run("sched")


def test_reload():
    """load_state_dict() into an optimizer that a graph and eager steps share: both continue from the saved step"""
    opt, _, _ = _run("reload")
    assert opt.hyper_parameters()["lr"] == mc.PLAIN["lr"]


def test_steady_states_keep_their_cost():
    """eager steps on unmoved gradients upload once; a capture records one upload; replays upload nothing from Python; a moved
    gradient uploads again"""
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    ps = [torch.from_numpy(a).cuda().requires_grad_(True) for a in mc.initial_params()]
    opt = MultiTensorAdam(ps, **mc.PLAIN)
    slots = [torch.zeros(s, device="cuda") for s in mc.SHAPES]
    for p, g in zip(ps, slots):
        p.grad = g
    assert opt.table_uploads == 0
    for _ in range(5):
        opt.step()
    assert opt.table_uploads == 1
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    assert opt.table_uploads == 2
    for _ in range(5):
        graph.replay()
    assert opt.table_uploads == 2
    for _ in range(3):
        opt.step()
    assert opt.table_uploads == 2
    moved = torch.zeros(mc.SHAPES[2], device="cuda")
    ps[2].grad = moved
    opt.step()
    opt.step()
    assert opt.table_uploads == 3
    torch.cuda.synchronize()
    assert float(opt.step_count) == 15.0


def test_a_step_on_unmoved_gradients_is_two_launches(monkeypatch):
    """the counter's add_ (the only framework operation: no copy, no upload) and one hf_adam_multi"""
    from torch.utils._python_dispatch import TorchDispatchMode

    from heterofusionrcnn_amd import _lib
    from heterofusionrcnn_amd.optim import MultiTensorAdam

    class Ops(TorchDispatchMode):
        seen = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            self.seen.append(str(func))
            return func(*args, **(kwargs or {}))

    ps = [torch.from_numpy(a).cuda().requires_grad_(True) for a in mc.initial_params()]
    opt = MultiTensorAdam(ps, **mc.PLAIN)
    slots = [torch.ones(s, device="cuda") for s in mc.SHAPES]
    for p, g in zip(ps, slots):
        p.grad = g
    opt.step()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opt.step()
    graph.replay()
    opt.step()                                                               # the first eager step after a capture also replaces the
    graph.replay()                                                           # staging set that the capture took for good
    L, launches = _lib.lib(), []
    for name in ("hf_adam_multi", "hf_adam_multi_sched", "hf_adam_sqnorm_partials"):
        monkeypatch.setattr(L, name, lambda *a, _f=getattr(L, name), _n=name: launches.append(_n) or _f(*a))
    with Ops():
        opt.step()                                                           # after a replay, on the eager table: a cache hit
    torch.cuda.synchronize()
    assert Ops.seen == ["aten.add_.Tensor"] and launches == ["hf_adam_multi"]
    assert opt.table_uploads == 2 and float(opt.step_count) == 5.0


def test_train_step_graph_and_eager_calls_share_one_optimizer():
    """graph_step.TrainStep(graph=True) and TrainStep(graph=False) over one model and one MultiTensorAdam, called G E G E E G, each call
    on its own batch, against an fp64 twin stepped six times (TensorFlow's Adam).  Plain torch layers, no atomics: the captured and
    the eager route run the same kernels.  Nothing is asserted about addresses: the allocator decides whether the key repeats"""
    from heterofusionrcnn_amd.graph_step import TrainStep
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(8, 16), torch.nn.Tanh(), torch.nn.Linear(16, 4))
    twin = copy.deepcopy(model).double()
    model = model.cuda()
    gen = torch.Generator().manual_seed(1)
    batches = [(torch.randn(32, 8, generator=gen), torch.randn(32, 4, generator=gen)) for _ in range(6)]
    loss_fn = lambda m, inp, geo: ((m(inp["x"]) - inp["y"]) ** 2).mean()
    opt = MultiTensorAdam(list(model.parameters()), **mc.PLAIN)
    inputs = {"x": batches[0][0].cuda(), "y": batches[0][1].cuda()}
    steps = {"G": TrainStep(model, opt, inputs, geometry={}, world=1, graph=True, loss_fn=loss_fn, warmup=3),
             "E": TrainStep(model, opt, inputs, geometry={}, world=1, graph=False, loss_fn=loss_fn)}
    keep = []
    ref = mc.Ref([p.detach().numpy() for p in twin.parameters()], mc.PLAIN)
    for n, (which, (x, y)) in enumerate(zip("GEGEEG", batches)):
        loss = steps[which](x=x.cuda(), y=y.cuda())
        keep.append([p.grad for p in model.parameters()])
        torch.cuda.synchronize()
        for p in twin.parameters():
            p.grad = None
        want = loss_fn(twin, {"x": x.double(), "y": y.double()}, None)
        want.backward()
        after = ref.step({i: p.grad.numpy() for i, p in enumerate(twin.parameters())})
        with torch.no_grad():
            for p, a in zip(twin.parameters(), after):
                p.copy_(torch.from_numpy(a))
        what = "call %d (%s)" % (n, which)
        np.testing.assert_allclose(float(loss), float(want.detach()), rtol=mc.RTOL, atol=mc.ATOL, err_msg=what)
        for i, (p, a) in enumerate(zip(model.parameters(), after)):
            np.testing.assert_allclose(p.detach().cpu().numpy(), a, rtol=mc.RTOL, atol=mc.ATOL, err_msg="%s, tensor %d" % (what, i))
        assert float(opt.step_count) == n + 1, what
