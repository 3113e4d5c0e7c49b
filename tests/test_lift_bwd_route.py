"""The one-pass route of the lifting chain's backward (_dense_kernels.LIFT_BWD_ONE_PASS -> hf_onepass_lift_elu_bn_bwd) against the
two-pass route it replaces: pointcnn.dense_chain on local coordinates (B, P, K, 3) with B P K = 40 000 rows, in training mode, for the
widths of the RPN's (64) and the RCNN's (128) lifting layers.  The forward is untouched (same bits); dW1, dgamma0 and dbeta0 are the
same bits; dW0 differs between the routes by no more than the sum of the two routes' bounds against fp64 (gemm_cases.lift_bwd_bounds on
the arguments the node hands to the entry: the same bound for both, see tests/test_lift_bwd_onepass_abi.py).  Each route makes the four
calls it should, and the new entry has one call site in the package."""
import ast
import copy
import glob
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

B, P, K = 2, 2500, 8
NEW, OLD = "hf_onepass_lift_elu_bn_bwd", "hf_lift_elu_bn_bwd"


class _CountingLib:
    """libhfops.so with every hf_* call logged by name"""

    def __init__(self, real, log):
        self._real, self._log = real, log

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if not name.startswith("hf_"):
            return fn
        return lambda *a: (self._log.append(name), fn(*a))[1]


def _step(k, pointcnn, monkeypatch, d0, d1, x, go, one_pass):
    log, args = [], []
    real_lib, real_bwd = k.lib, k.lift_elu_bn_bwd
    monkeypatch.setattr(k, "LIFT_BWD_ONE_PASS", one_pass)
    monkeypatch.setattr(k, "lib", lambda: _CountingLib(real_lib(), log))
    monkeypatch.setattr(k, "lift_elu_bn_bwd", lambda *a: (args.append(a), real_bwd(*a))[1])
    out = pointcnn.dense_chain(d0, d1, x)
    out.backward(go)
    torch.cuda.synchronize()
    monkeypatch.setattr(k, "lib", real_lib)
    monkeypatch.setattr(k, "lift_elu_bn_bwd", real_bwd)
    grads = dict(w0=d0.linear.weight.grad, gamma0=d0.post.bn.weight.grad, beta0=d0.post.bn.bias.grad, w1=d1.linear.weight.grad,
                 gamma1=d1.post.bn.weight.grad, beta1=d1.post.bn.bias.grad)
    return out.detach(), grads, [n for n in log if not n.endswith("_workspace")], args


@pytest.mark.gpu
@pytest.mark.parametrize("c", [64, 128])
def test_one_pass_route_against_the_two_pass_route(monkeypatch, c):
    from heterofusionrcnn_amd import _dense_kernels as k, mlp, pointcnn
    assert k.LIFT_BWD_ONE_PASS is True, "the module switch defaults to the one-pass route"
    assert B * P * K == 40000 >= mlp.FUSED_FWD_MIN_ROWS and c <= k.LIFT_BWD_ONE_PASS_MAX_C0
    torch.manual_seed(11)
    x = (torch.randn(B, P, K, 3, device="cuda") * 0.5).contiguous()
    go = torch.randn(B, P, K, c, device="cuda")
    d0 = pointcnn.Dense(3, c, allow_bf16=False).cuda().train()
    d1 = pointcnn.Dense(c, c, allow_bf16=False).cuda().train()
    for mod in (d0, d1):      # BatchNorm parameters off their initial 1 / 0, so that every term of the backward is live
        with torch.no_grad():
            mod.post.bn.weight.uniform_(0.5, 1.5)
            mod.post.bn.bias.normal_(0.0, 0.1)
    n0, n1, o0, o1 = d0, d1, copy.deepcopy(d0), copy.deepcopy(d1)
    out_new, g_new, calls_new, args_new = _step(k, pointcnn, monkeypatch, n0, n1, x, go, True)
    out_old, g_old, calls_old, args_old = _step(k, pointcnn, monkeypatch, o0, o1, x, go, False)

    head = ["hf_lift_elu_bn_fwd", "hf_bn_relu_fwd_eval", "hf_bn_relu_bwd_ld"]
    assert calls_new == head + [NEW] and calls_old == head + [OLD]
    assert len(args_new) == len(args_old) == 1
    for a, b in zip(args_new[0], args_old[0]):
        assert torch.equal(a, b), "the two routes were handed different arguments"

    assert torch.equal(out_new, out_old), "forward: %d of %d elements differ" % (int((out_new != out_old).sum()), out_old.numel())
    for (name, a), (_, b) in zip(list(n0.named_buffers()) + list(n1.named_buffers()), list(o0.named_buffers()) + list(o1.named_buffers())):
        assert torch.equal(a, b), "running statistics %s differ after the step" % name
    for name in ("w1", "gamma0", "beta0", "gamma1", "beta1"):
        assert torch.equal(g_new[name], g_old[name]), name

    x3, w0, g0, b0, m0, i0, dz1, w1t = args_new[0]
    rows = x3.shape[0]
    _, _, rpc, chunks = gc.wgrad_plan(rows, c, c)
    bound = gc.lift_bwd_bounds(x3, w0, [g0, b0, m0.double(), i0.double()], w1t.t(), dz1, 16 * gc.tiles_per_workgroup(rows, gc.cdiv(c, 32)) + 4,
                               min(rows, rpc) + gc.cdiv(chunks, 16) + 15)["d_w0"]
    diff = (g_new["w0"].double() - g_old["w0"].double()).abs()
    print("c = %d: |dW0 one-pass - dW0 two-pass| max %.3g, largest share of the summed bounds %.3g, largest |dW0| %.3g" % (
        c, float(diff.max()), float((diff / (2.0 * bound)).max()), float(g_old["w0"].abs().max())))
    assert bool((diff <= 2.0 * bound).all())


def test_the_new_entry_has_one_call_site_in_the_launch_module():
    from heterofusionrcnn_amd import _lib
    pkg = os.path.dirname(os.path.abspath(_lib.__file__))
    sites = {NEW: [], NEW + "_workspace": [], OLD: []}
    for path in sorted(glob.glob(os.path.join(pkg, "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in sites:
                sites[node.func.attr].append(os.path.basename(path))
        strings = [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
        assert os.path.basename(path) == "_lib.py" or not [s for s in strings if s in sites], path      # not fetched by name either
    assert sites == {NEW: ["_dense_kernels.py"], NEW + "_workspace": ["_dense_kernels.py"], OLD: ["_dense_kernels.py"]}
