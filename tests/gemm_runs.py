"""The lifting family's inputs and the call of hf_lift_elu_bn_bwd through the C ABI, as a plain module: tests/test_gemm_abi.py checks
the entry against fp64 with them, tests/test_lift_bwd_onepass_abi.py holds the one-pass entry to the same inputs and to its bits."""
import torch

import gemm_cases as gc
from abi_harness import Arena, abi, call, place

DEV = "cuda"
UNSET = ("HF_GEMM_ROUNDS",)         # gemm_cases.resident_grid restates the product library's two rounds


def lift_inputs(c):
    g = gc.generator(c)
    rows, c0, c1, exact = c["rows"], c["c0"], c["c1"], c["family"] == "exact"
    if exact:       # non-negative x3 W0^T, gamma0 = invstd0 = 1, y0 >= 0; eval_bn: W1 >= 0 too, so that the epilogue's ELU is the identity
        t = dict(x3=gc.ints(g, (rows, 3), 0, 2), w0=gc.ints(g, (c0, 3), 0, 2), bn0=gc.bn_consts(g, c0, True, nonneg=True),
                 w1=gc.ints(g, (c1, c0), 0 if c["kind"] != "lift_eval" else -2, 2), bn1=gc.bn_consts(g, c1, True), dz1=gc.ints(g, (rows, c1), -2, 2))
    else:
        t = dict(x3=torch.randn(rows, 3, generator=g) * 0.5, w0=torch.randn(c0, 3, generator=g), bn0=gc.bn_consts(g, c0, False),
                 w1=torch.randn(c1, c0, generator=g) * 0.3, bn1=gc.bn_consts(g, c1, False), dz1=torch.randn(rows, c1, generator=g))
    for k in ("rm0", "rm1"):
        t[k] = torch.randn(c0 if k == "rm0" else c1, generator=g)
    for k in ("rv0", "rv1"):
        t[k] = torch.rand(c0 if k == "rv0" else c1, generator=g) + 0.5
    return t


def run_lift_bwd(c, t, stats):
    _lib, L = abi(UNSET)
    ptr, sp = _lib.ptr, _lib.stream_ptr()
    rows, c0, c1, mis = c["rows"], c["c0"], c["c1"], c["misalign"]
    a = Arena(DEV)
    x3, w0, g0, b0 = place(DEV, t["x3"]), place(DEV, t["w0"]), place(DEV, t["bn0"][0]), place(DEV, t["bn0"][1])
    mean0, invstd0 = place(DEV, stats[0]), place(DEV, stats[1])
    dz1, w1t = place(DEV, t["dz1"], mis == "dz1"), place(DEV, t["w1"].t().contiguous(), mis == "w1_t")
    gw0t, gw1, dg0, db0 = a.out((3, c0)), a.out((c1, c0)), a.out((c0,)), a.out((c0,))
    nbytes = L.hf_lift_elu_bn_bwd_workspace(rows, c0, c1)
    ws = a.out((nbytes // 4,))
    call(L.hf_lift_elu_bn_bwd(rows, c0, c1, ptr(x3), ptr(w0), ptr(g0), ptr(b0), ptr(mean0), ptr(invstd0), ptr(dz1), ptr(w1t), ptr(gw0t), ptr(gw1),
                              ptr(dg0), ptr(db0), ptr(ws), nbytes, sp), "hf_lift_elu_bn_bwd")
    a.check()
    return dict(grad_w0_t=gw0t, grad_w1=gw1, dgamma0=dg0, dbeta0=db0)
