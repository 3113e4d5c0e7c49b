"""SURVEY.md 8f rank 2, FP half: the first layer of a feature-propagation MLP on three_nn rows read in place
(hf_linear_bn_fwd_interp / hf_linear_wgrad_interp, mlp.shared_mlp_interp) against
  1. an fp64 evaluation through the C ABI on inputs whose every partial sum is an exact fp32 number (dropped rows, stale prefetches
     and misindexed gathers show at any summation order),
  2. hf_linear_bn_fwd on the output of hf_three_interpolate_concat (the materialised operand): the same bits,
  3. the materialised route (three_interpolate_concat -> shared_mlp) and an fp64 autograd evaluation of
     pointnet_util.py:303-329 + conv2d [1,1] + batch norm + ReLU,
  4. the materialised route at inference, and modules.INTERP_ON_LOAD as the switch of a PointnetFPModule."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
from abi_harness import Arena, abi, place, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EPS, MOMENTUM = 1e-3, 0.1
TWO24 = float(2 ** 24)
DYADIC = torch.tensor([[1, 0, 0], [0, 0, 1], [.5, .25, .25], [.25, .5, .25], [.25, .25, .5]])


# ------------------------------------------------------------------------------------------------- 1. exact family, C ABI
def exact_inputs(seed, clouds, rows_per_cloud, m, c2, c1, cout, bias=True):
    """integer-valued points2 / skip in [-8, 8], sparse weight in {-1, 0, 1}, sparse +-1 grad_z, dyadic interpolation weights;
    idx hits 0, m - 1 and repeated indices"""
    g = torch.Generator().manual_seed(seed)
    rows, cin = clouds * rows_per_cloud, (c2 + c1 + 3) // 4 * 4
    idx = torch.randint(0, m, (rows, 3), generator=g, dtype=torch.int32)
    idx[0] = torch.tensor([0, m - 1, 0])
    idx[rows - 1] = torch.tensor([m - 1, m - 1, m - 1])
    idx[rows // 2] = torch.tensor([0, 0, m - 1])
    w3 = DYADIC[torch.randint(0, DYADIC.shape[0], (rows,), generator=g)].contiguous()
    w = torch.zeros(cout, cin)
    w[:, :c2 + c1] = gc.sparse_pm1(g, (cout, c2 + c1))
    return dict(points2=gc.ints(g, (clouds, m, c2), -8, 8), skip=gc.ints(g, (rows, c1), -8, 8) if c1 else None, idx=idx, w3=w3, w=w,
                bias=gc.ints(g, (cout,), -2, 2) if bias else None, gz=gc.sparse_pm1(g, (rows, cout)),
                rm=torch.randn(cout, generator=g), rv=torch.rand(cout, generator=g) + 0.5)


def operand64(t, rows_per_cloud, cin):
    """the (rows, cin) operand in fp64: [sum_t w_t points2[cloud, idx_t] | skip | zeros]"""
    idx, w3 = t["idx"].to(DEV).long(), t["w3"].to(DEV).double()
    rows = idx.shape[0]
    cloud = torch.arange(rows, device=DEV) // rows_per_cloud
    p = t["points2"].to(DEV).double()
    parts = [sum(w3[:, s:s + 1] * p[cloud, idx[:, s]] for s in range(3))]
    if t["skip"] is not None:
        parts.append(t["skip"].to(DEV).double())
    x = torch.cat(parts, 1)
    return torch.nn.functional.pad(x, (0, cin - x.shape[1]))


def run_fwd(t, rows_per_cloud, m, c2, c1, cout, mis=None, running=True):
    _lib, L = abi()
    ptr = _lib.ptr
    rows = t["idx"].shape[0]
    a = Arena(DEV)
    z, mean, invstd = a.out((rows, cout)), a.out((cout,)), a.out((cout,))
    rm, rv = (a.out((cout,), init=t["rm"]), a.out((cout,), init=t["rv"])) if running else (None, None)
    nbytes = L.hf_linear_bn_fwd_workspace(cout)
    ws = a.out((nbytes // 4,))          # exactly the bytes the library asks for, guarded like an output
    p2, skip, w = place(DEV, t["points2"], mis == "points2"), place(DEV, t["skip"], mis == "skip"), place(DEV, t["w"], mis == "weight")
    idx, w3, bias = place(DEV, t["idx"]), place(DEV, t["w3"]), place(DEV, t["bias"])
    _lib.check(L.hf_linear_bn_fwd_interp(rows, c2, c1, cout, ptr(p2), m, rows_per_cloud, ptr(idx), ptr(w3), ptr(skip), ptr(w), ptr(bias), ptr(z), EPS,
                                         MOMENTUM, ptr(rm), ptr(rv), ptr(mean), ptr(invstd), ptr(ws), nbytes, _lib.stream_ptr()),
               "hf_linear_bn_fwd_interp")
    a.check()
    return dict(z=z, mean=mean, invstd=invstd, rm=rm, rv=rv)


def run_wgrad(t, rows_per_cloud, m, c2, c1, cout, mis=None):
    _lib, L = abi()
    ptr = _lib.ptr
    rows, cin = t["idx"].shape[0], (c2 + c1 + 3) // 4 * 4
    a = Arena(DEV)
    dw = a.out((cout, cin))
    nbytes = L.hf_linear_wgrad_workspace(rows, cout, cin)
    ws = a.out((nbytes // 4,))
    gz, p2, skip = place(DEV, t["gz"], mis == "grad_z"), place(DEV, t["points2"], mis == "points2"), place(DEV, t["skip"], mis == "skip")
    idx, w3 = place(DEV, t["idx"]), place(DEV, t["w3"])
    _lib.check(L.hf_linear_wgrad_interp(rows, cout, c2, c1, ptr(gz), ptr(p2), m, rows_per_cloud, ptr(idx), ptr(w3), ptr(skip), ptr(dw), ptr(ws),
                                        nbytes, _lib.stream_ptr()), "hf_linear_wgrad_interp")
    a.check()
    return dw


def check_fwd_exact(t, got, rows_per_cloud, c2, c1, cout):
    """z bit for bit; mean / invstd / running estimates with the statistics tolerance of tests/test_gemm_abi.py (check_statistics:
    one rounding of the cast where every per-workgroup sum is an integer below 2^24, gemm_cases.stats_bounds otherwise)"""
    rows, cin, nt = t["idx"].shape[0], (c2 + c1 + 3) // 4 * 4, gc.cdiv(cout, 32)
    x = operand64(t, rows_per_cloud, cin)
    ref = gc.ref_linear_fwd(x, None, t["w"].to(DEV), None if t["bias"] is None else t["bias"].to(DEV), False,
                            16 * gc.tiles_per_workgroup(rows, nt) + 4, EPS)
    assert float(ref["z"].abs().max()) * 4 < TWO24          # multiples of 1/4 below 2^22: every partial sum is an fp32 number
    same(got["z"], ref["z"], "z")
    d_mean, d_var, d_invstd = ref["d_mean"], ref["d_var"], ref["d_invstd"]
    s64 = ref["z"]
    if gc.tiles_per_workgroup(rows, nt) * gc.FWD_ROWS * float(s64.abs().max()) ** 2 < TWO24 and bool((s64 == s64.round()).all()):
        d_mean, d_var, d_invstd = gc.U * ref["mean"].abs(), gc.U * ref["var"], 2 * gc.U * ref["invstd"]
    within(got["mean"], ref["mean"], d_mean, "mean")
    within(got["invstd"], ref["invstd"], d_invstd, "invstd")
    if got["rm"] is not None:
        want, b = gc.running_bounds(t["rm"].to(DEV), ref["mean"], d_mean, MOMENTUM)
        within(got["rm"], want, b, "running_mean")
        want, b = gc.running_bounds(t["rv"].to(DEV), ref["var"], d_var, MOMENTUM)
        within(got["rv"], want, b, "running_var")


def check_wgrad_exact(t, dw, rows_per_cloud, c2, c1, cout):
    cin = (c2 + c1 + 3) // 4 * 4
    want = t["gz"].to(DEV).double().t() @ operand64(t, rows_per_cloud, cin)
    assert float(want.abs().max()) * 4 < TWO24
    same(dw, want, "grad_weight")
    assert float(dw[:, c2 + c1:].abs().max()) == 0.0 if cin > c2 + c1 else True          # padding columns: exactly zero


SHAPES = ((4, 0), (32, 0), (7, 0), (36, 1), (64, 64), (30, 5), (1020, 4), (4, 1024))
COUTS = (31, 64, 96, 128, 160, 192, 224, 256)               # one per accumulator-tile count of the forward kernel
ROWS_PER_CLOUD = (1, 129, 645)                              # two clouds: a tile spans both, the last tile is ragged
# every (c2, c1) at every rows_per_cloud; the couts and the two cloud sizes m rotate through them, so that each cout meets three
# shapes (both access widths among them) and each shape meets both m
EXACT_CASES = [(c2, c1, COUTS[(i + j) % 8], rpc, (3, 64)[(i + j) % 2])
               for i, (c2, c1) in enumerate(SHAPES) for j, rpc in enumerate(ROWS_PER_CLOUD)]


@pytest.mark.parametrize("c2,c1,cout,rpc,m", EXACT_CASES)
def test_interp_fwd_exact(c2, c1, cout, rpc, m):
    t = exact_inputs(1000 * c2 + 10 * c1 + rpc, 2, rpc, m, c2, c1, cout, bias=(c2 + rpc) % 2 == 0)
    check_fwd_exact(t, run_fwd(t, rpc, m, c2, c1, cout, running=rpc != 129), rpc, c2, c1, cout)


@pytest.mark.parametrize("c2,c1,cout,rpc,m", EXACT_CASES)
def test_interp_wgrad_exact(c2, c1, cout, rpc, m):
    t = exact_inputs(1000 * c2 + 10 * c1 + rpc + 1, 2, rpc, m, c2, c1, cout)
    check_wgrad_exact(t, run_wgrad(t, rpc, m, c2, c1, cout), rpc, c2, c1, cout)


def test_interp_fwd_exact_every_workgroup_walks_two_tiles():
    """rows from the launcher's grid rule (gemm_cases.multi_tile_rows): every workgroup of the persistent grid walks two tiles,
    workgroup 0 a ragged third -- the prefetch of the next tile's indices, weights and first stage"""
    rows = gc.multi_tile_rows(1)
    assert rows % 5 == 0 and gc.tiles_per_workgroup(rows, 1) == 3
    t = exact_inputs(77, 5, rows // 5, 64, 4, 0, 32)
    check_fwd_exact(t, run_fwd(t, rows // 5, 64, 4, 0, 32), rows // 5, 4, 0, 32)


def test_interp_wgrad_exact_200003_rows():
    """many chunks, a ragged last stage in the last chunk"""
    t = exact_inputs(78, 1, 200003, 64, 36, 1, 64)
    assert gc.wgrad_plan(200003, 64, 40)[3] > 16
    check_wgrad_exact(t, run_wgrad(t, 200003, 64, 36, 1, 64), 200003, 36, 1, 64)


@pytest.mark.parametrize("mis", ["points2", "skip", "weight"])
def test_interp_fwd_exact_misaligned(mis):
    """each pointer whose alignment the launcher inspects, 4 bytes off a 16-byte boundary in turn (the single-column paths)"""
    t = exact_inputs(79, 2, 645, 64, 64, 64, 96)
    check_fwd_exact(t, run_fwd(t, 645, 64, 64, 64, 96, mis=mis), 645, 64, 64, 96)


@pytest.mark.parametrize("mis", ["grad_z", "points2", "skip"])
def test_interp_wgrad_exact_misaligned(mis):
    t = exact_inputs(80, 2, 645, 64, 64, 64, 96)
    check_wgrad_exact(t, run_wgrad(t, 645, 64, 64, 64, 96, mis=mis), 645, 64, 64, 96)


# ------------------------------------------------------------------------------------------------- 2. the materialised operand
@pytest.mark.parametrize("c2,c1,cout,n", [(32, 0, 31, 645), (64, 1, 128, 645), (256, 64, 224, 300), (36, 5, 256, 129)])
def test_interp_fwd_same_bits_as_materialised_operand(c2, c1, cout, n):
    """c2 % 4 == 0, N(0,1) data: hf_linear_bn_fwd on the rows hf_three_interpolate_concat writes, same weight.  The new kernel keeps
    the ascending-k accumulation of linear_fwd_kernel, builds the operand with the concat kernel's expression and runs on the
    same grid, so z and the statistics are EQUAL, not merely within the 2e-5 x scale that two fp32 routes are allowed"""
    _lib, L = abi()
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    b, m = 2, 50
    g = torch.Generator().manual_seed(c2 + c1)
    rows, cin = b * n, (c2 + c1 + 3) // 4 * 4
    p2 = torch.randn(b, m, c2, generator=g).to(DEV)
    skip = torch.randn(b, n, c1, generator=g).to(DEV) if c1 else None
    idx = torch.randint(0, m, (b, n, 3), generator=g, dtype=torch.int32).to(DEV)
    w3 = torch.rand(b, n, 3, generator=g)
    w3 = (w3 / w3.sum(2, keepdim=True)).to(DEV)
    w = torch.nn.functional.pad(torch.randn(cout, c2 + c1, generator=g) * 0.3, (0, cin - c2 - c1)).to(DEV)
    bias = torch.randn(cout, generator=g).to(DEV)
    nbytes = L.hf_linear_bn_fwd_workspace(cout)
    ws = torch.empty(nbytes // 4, device=DEV)
    outs = []
    for route in ("in place", "materialised"):
        z, mean, invstd = torch.empty(rows, cout, device=DEV), torch.empty(cout, device=DEV), torch.empty(cout, device=DEV)
        if route == "in place":
            _lib.check(L.hf_linear_bn_fwd_interp(rows, c2, c1, cout, ptr(p2), m, n, ptr(idx), ptr(w3), ptr(skip), ptr(w), ptr(bias), ptr(z), EPS,
                                                 MOMENTUM, None, None, ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_linear_bn_fwd_interp")
        else:
            x = torch.empty(rows, cin, device=DEV)
            _lib.check(L.hf_three_interpolate_concat(b, m, c2, n, c1, cin, ptr(p2), ptr(idx), ptr(w3), ptr(skip), ptr(x), sp), "concat")
            _lib.check(L.hf_linear_bn_fwd(rows, cin, cout, ptr(x), None, None, None, None, None, ptr(w), ptr(bias), ptr(z), EPS, MOMENTUM, None,
                                          None, ptr(mean), ptr(invstd), ptr(ws), nbytes, sp), "hf_linear_bn_fwd")
        outs.append((z, mean, invstd))
    for a_, b_, name in zip(outs[0], outs[1], ("z", "mean", "invstd")):
        print("%s: max |in place - materialised| = %.3g" % (name, float((a_ - b_).abs().max())))
        assert torch.equal(a_, b_), name


# ------------------------------------------------------------------------------------------------- 3. the chain
def _setup(b, n, m, c2, c1, widths, seed):
    from heterofusionrcnn_amd.modules import PointnetFPModule, SharedMLPLayer
    rng = np.random.default_rng(seed)
    xyz1 = rng.random((b, n, 3), dtype=np.float32)
    xyz2 = np.stack([xyz1[i, rng.permutation(n)[:m]] for i in range(b)])          # known points are a subset: zero distances
    idx, weight, inverse = PointnetFPModule.geometry(torch.from_numpy(xyz1).cuda(), torch.from_numpy(xyz2).cuda())
    p2 = torch.from_numpy(rng.standard_normal((b, m, c2)).astype(np.float32)).cuda().requires_grad_(True)
    p1 = torch.from_numpy(rng.standard_normal((b, n, c1)).astype(np.float32)).cuda().requires_grad_(True) if c1 else None
    torch.manual_seed(seed)
    layers, cin = [], c2 + c1
    for w in widths:
        layers.append(SharedMLPLayer(cin, w).cuda().train())
        cin = w
    for l in layers:                                              # non-trivial BatchNorm parameters
        with torch.no_grad():
            l.bn.weight.uniform_(0.5, 1.5)
            l.bn.bias.uniform_(-0.3, 0.3)
            l.fc.bias.uniform_(-0.1, 0.1)
    return idx, weight, inverse, p2, p1, layers


def _fp64_reference(idx, weight, p2, p1, layers, dout):
    """pointnet_util.py:303-329 in fp64 torch ops with autograd: interpolate, concat, then conv2d [1,1] + batch norm + ReLU"""
    b, n, _ = idx.shape
    q2 = p2.detach().double().requires_grad_(True)
    q1 = p1.detach().double().requires_grad_(True) if p1 is not None else None
    bi = torch.arange(b, device=idx.device)[:, None]
    interp = sum(weight.double()[:, :, s:s + 1] * q2[bi, idx[:, :, s].long()] for s in range(3))
    x = (torch.cat([interp, q1], 2) if q1 is not None else interp).reshape(b * n, -1)
    ws = []
    for l in layers:
        w, bb = l.fc.weight.detach().double().requires_grad_(True), l.fc.bias.detach().double().requires_grad_(True)
        g, be = l.bn.weight.detach().double().requires_grad_(True), l.bn.bias.detach().double().requires_grad_(True)
        ws += [w, bb, g, be]
        z = x @ w.t() + bb
        mu, var = z.mean(0), z.var(0, unbiased=False)
        x = torch.relu(g * (z - mu) / torch.sqrt(var + l.bn.eps) + be)
    x.backward(dout.double())
    return x.detach(), q2.grad, (q1.grad if q1 is not None else None), [w.grad for w in ws]


@pytest.mark.parametrize("c2,c1,widths", [(16, 0, (32, 64)), (64, 1, (64, 128)), (67, 5, (96,)), (128, 64, (128, 256)), (256, 1, (16, 224))])
def test_interp_mlp_in_place_matches_materialised_route_and_fp64(c2, c1, widths):
    from heterofusionrcnn_amd.interpolate import three_interpolate_concat
    from heterofusionrcnn_amd.mlp import interp_mlp_fusable, shared_mlp, shared_mlp_interp
    b, n, m = 2, 1500, 200
    idx, weight, inverse, p2, p1, layers = _setup(b, n, m, c2, c1, widths, 200 + c2)
    assert interp_mlp_fusable(layers, p2, p1, idx)
    torch.manual_seed(0)
    dout = torch.randn(b * n, widths[-1], device="cuda")
    params = [p for l in layers for p in (l.fc.weight, l.fc.bias, l.bn.weight, l.bn.bias)]
    inputs = [p2] + ([p1] if p1 is not None else [])

    def run(fn):
        for p in params + inputs:
            p.grad = None
        for l in layers:
            l.bn.running_mean.zero_(); l.bn.running_var.fill_(1.0)
        out = fn()
        out.backward(dout)
        return (out.detach().clone(), [p.grad.clone() for p in inputs], [p.grad.clone() for p in params],
                [(l.bn.running_mean.clone(), l.bn.running_var.clone()) for l in layers])

    in_place = lambda: shared_mlp_interp(layers, p2, p1, idx, weight, inverse)
    got = run(in_place)

    def materialised():
        x = three_interpolate_concat(p2, p1, idx, weight, inverse)
        return shared_mlp(layers, x.reshape(-1, x.shape[-1]))
    want = run(materialised)

    ref_out, ref_d2, ref_d1, ref_dw = _fp64_reference(idx, weight, p2, p1, layers, dout)
    # against fp64: forward 1e-4 of the output scale (fp32 GEMM + batch statistics), gradients 2e-3 of their scale
    scale = float(ref_out.abs().max())
    print("forward: |got - fp64| = %.3g, |got - materialised| = %.3g, scale %.3g" % (
        float((got[0].double() - ref_out).abs().max()), float((got[0] - want[0]).abs().max()), scale))
    assert float((got[0].double() - ref_out).abs().max()) <= 1e-4 * max(scale, 1.0)
    assert float((got[0] - want[0]).abs().max()) <= 2e-5 * max(scale, 1.0)            # the two fp32 routes against each other
    for a, r, name in zip(got[1], [ref_d2] + ([ref_d1] if p1 is not None else []), ("d points2", "d points1")):
        gs = float(r.abs().max())
        print("%s: |got - fp64| = %.3g, scale %.3g" % (name, float((a.double() - r).abs().max()), gs))
        assert float((a.double() - r).abs().max()) <= 2e-3 * gs, name
    for gi, (a, r) in enumerate(zip(got[2], ref_dw)):
        if gi % 4 == 1:
            assert float(a.abs().max()) == 0.0                                        # a bias under a BatchNorm: exactly zero
            continue
        rs = float(r.abs().max())
        assert float((a.double() - r).abs().max()) <= 3e-3 * rs + 1e-6, (gi, float((a.double() - r).abs().max()), rs)
    for (m1, v1), (m2, v2) in zip(got[3], want[3]):                                   # running statistics updated the same way
        assert torch.allclose(m1, m2, rtol=1e-4, atol=1e-6) and torch.allclose(v1, v2, rtol=1e-4, atol=1e-6)
    # no atomics anywhere in the route: a second call gives the same bits in every output and gradient
    again = run(in_place)
    assert torch.equal(got[0], again[0])
    for a, r in zip(got[1] + got[2], again[1] + again[2]):
        assert torch.equal(a, r)
    for (m1, v1), (m2, v2) in zip(got[3], again[3]):
        assert torch.equal(m1, m2) and torch.equal(v1, v2)


# ------------------------------------------------------------------------------------------------- 4. inference and the switch
def test_interp_mlp_eval_mode_matches_materialised_route():
    from heterofusionrcnn_amd.interpolate import three_interpolate_concat
    from heterofusionrcnn_amd.mlp import shared_mlp, shared_mlp_interp
    idx, weight, inverse, p2, p1, layers = _setup(2, 1500, 200, 64, 5, (32, 64), 7)
    for l in layers:
        l.bn.running_mean.normal_(0, 0.1); l.bn.running_var.uniform_(0.5, 1.5)
        l.eval()
    with torch.no_grad():
        a = shared_mlp_interp(layers, p2.detach(), p1.detach(), idx, weight, None)
        x = three_interpolate_concat(p2.detach(), p1.detach(), idx, weight, inverse)
        bb = shared_mlp(layers, x.reshape(-1, x.shape[-1]))
    assert torch.allclose(a, bb, rtol=1e-5, atol=1e-5)


def _run_fp_module(fp, xyz1, xyz2, p1, p2):
    """(output, input gradients, parameter gradients, calls of _InterpLinear.apply) of one training step of the module"""
    from heterofusionrcnn_amd import mlp
    calls = [0]
    orig = mlp._InterpLinear.apply

    def counting(*args):
        calls[0] += 1
        return orig(*args)
    mlp._InterpLinear.apply = counting
    try:
        for l in fp.mlp:
            l.bn.running_mean.zero_(); l.bn.running_var.fill_(1.0)
        a, c = p1.detach().clone().requires_grad_(True), p2.detach().clone().requires_grad_(True)
        f = fp(xyz1, xyz2, a, c)
        f.square().sum().backward()
        out = (f.detach(), [a.grad.clone(), c.grad.clone()], [q.grad.clone() for q in fp.parameters()], calls[0])
        fp.zero_grad()
    finally:
        del mlp._InterpLinear.apply          # the inherited classmethod is visible again
    return out


def test_interp_module_switch():
    """modules.INTERP_ON_LOAD switches a PointnetFPModule between the routes at a shape the default predicate accepts (32768 rows);
    with the flag off, or at 2048 rows, the module takes the materialised path"""
    from heterofusionrcnn_amd import modules
    b, n, m, c2, c1 = 2, 16384, 64, 32, 1
    rng = np.random.default_rng(11)
    xyz1 = torch.from_numpy(rng.random((b, n, 3), dtype=np.float32)).cuda()
    xyz2 = xyz1[:, :m].contiguous()
    p2 = torch.from_numpy(rng.standard_normal((b, m, c2)).astype(np.float32)).cuda()
    p1 = torch.from_numpy(rng.standard_normal((b, n, c1)).astype(np.float32)).cuda()
    torch.manual_seed(3)
    fp = modules.PointnetFPModule(c2 + c1, [32]).cuda().train()
    assert modules.INTERP_ON_LOAD is True
    outs = []
    try:
        for flag in (True, False):
            modules.INTERP_ON_LOAD = flag
            outs.append(_run_fp_module(fp, xyz1, xyz2, p1, p2))
        modules.INTERP_ON_LOAD = True
        small = _run_fp_module(fp, xyz1[:, :1024].contiguous(), xyz2, p1[:, :1024].contiguous(), p2)
    finally:
        modules.INTERP_ON_LOAD = True
    assert outs[0][3] == 1 and outs[1][3] == 0 and small[3] == 0          # the True run really took the new route, the others did not
    assert torch.allclose(outs[0][0], outs[1][0], rtol=1e-4, atol=1e-5)
    for a_, b_ in zip(outs[0][1], outs[1][1]):
        assert torch.allclose(a_, b_, rtol=1e-3, atol=1e-4 * float(b_.abs().max()))
    for a_, b_ in zip(outs[0][2], outs[1][2]):
        assert torch.allclose(a_, b_, rtol=2e-3, atol=2e-3 * float(b_.abs().max()) + 1e-7)
