"""The references and bounds of tests/gemm_cases.py checked on the host: a plain fp32 torch evaluation of every entry point of
csrc/gemm.hip (same formulas, torch's own summation order) takes the place of the library call in the checks of tests/test_gemm_abi.py,
at the sweep cases of at most 1000 rows.  The exact family must come out bit for bit and the rounding family inside the derived bounds:
a reference or a bound that is wrong fails here, without a GPU, before it can be blamed on a kernel."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402
import test_gemm_abi as T  # noqa: E402

EPS, MOM = T.EPS, T.MOMENTUM
f32 = torch.float32
MAX_ROWS = 1000


def stats(s, rm, rv):
    mean = s.double().mean(0)
    var = (s.double() ** 2).mean(0) - mean ** 2
    var = var.clamp(min=0)
    mean32, inv32 = mean.float(), (1 / torch.sqrt(var + float(torch.tensor(EPS, dtype=f32)))).float()
    o = dict(mean=mean32, invstd=inv32, rm=None, rv=None)
    m = torch.tensor(MOM, dtype=f32)
    if rm is not None:
        o["rm"] = (1 - m) * rm + m * mean32
    if rv is not None:
        o["rv"] = (1 - m) * rv + m * var.float()
    return o


def onload(x, bn, elu):
    if bn is None:
        return x
    a = bn[0] * bn[3]
    e = F.elu(x) if elu else x
    h = a * (e - bn[2]) + bn[1]
    return h if elu else h.clamp(min=0)


def emu_fwd(c, t):
    h = onload(t["x"], t["bn"], c["elu"])
    z = h @ t["w"].t()
    if t["bias"] is not None:
        z = z + t["bias"]
    s = F.elu(z) if c["elu"] else z
    o = stats(s, t["rm"] if c["running"] in (1, 2) else None, t["rv"] if c["running"] in (1, 3) else None)
    o.update(z=z, x_act=h if c["xact"] else None)
    return o


def emu_bwd(c, t):
    rows, form = c["rows"], c["form"]
    o = dict(dx=None, dz_out=None, p_dgamma=None, p_dbeta=None)
    if t["z"] is not None:
        g, b, mu, istd = t["bn"]
        a = g * istd
        dh = torch.where(a * (t["z"] - mu) + b > 0, t["dy"], torch.zeros(()))
        xhat = (t["z"] - mu) * istd
        inv_r = torch.tensor(1.0 / rows, dtype=f32)
        dz = a * (dh - t["dbeta"] * inv_r - xhat * (t["dgamma"] * inv_r))
        o["dz_out"] = dz
    else:
        dz = t["dy"]
    dx = dz @ t["wt"].t()
    if "dx" in form:
        o["dx"] = dx
    if t["zprev"] is not None:
        pg, pb, pm, pis = t["pbn"]
        if c["elu"]:
            dh2, e = dx, F.elu(t["zprev"])
        else:
            e = t["zprev"]
            dh2 = torch.where(pg * pis * (e - pm) + pb > 0, dx, torch.zeros(()))
        o["p_dbeta"] = dh2.double().sum(0).float()
        o["p_dgamma"] = (dh2 * ((e - pm) * pis)).double().sum(0).float()
    return o


def emu_wgrad(c, t):
    return dict(dw=t["g"].t() @ onload(t["x"], t["bn"], False))


def emu_gather_fwd(c, t):
    a = gc.gather_operand(t["points"], t["idx"], t["gxyz"], c["rows_per_cloud"])
    z = a @ t["w"].t()
    if t["bias"] is not None:
        z = z + t["bias"]
    o = stats(z, None, None)
    o["z"] = z
    return o


def emu_gather_wgrad(c, t):
    a = gc.gather_operand(t["points"], t["idx"], t["gxyz"], c["rows_per_cloud"])
    return dict(dw=t["g"].t() @ a)


def lift_e0(t):
    x, w = t["x3"], t["w0"]
    z0 = (x[:, 0:1] * w[:, 0] + x[:, 1:2] * w[:, 1]) + x[:, 2:3] * w[:, 2]
    return z0, torch.where(z0 > 0, z0, torch.exp(z0) - 1)


def emu_lift_eval(c, t):
    _, e0 = lift_e0(t)
    g, b, mu, istd = t["bn0"]
    z1 = ((g * istd) * (e0 - mu) + b) @ t["w1"].t()
    if c["kind"] == "lift_eval":
        return dict(out=z1)
    g1, b1, m1, i1 = t["bn1"]
    e1 = torch.where(z1 > 0, z1, torch.exp(z1) - 1)
    return dict(out=(g1 * i1) * (e1 - m1) + b1)


def emu_lift_train(c, t):
    _, e0 = lift_e0(t)
    s0 = stats(e0, t["rm0"], t["rv0"])
    z1 = ((t["bn0"][0] * s0["invstd"]) * (e0 - s0["mean"]) + t["bn0"][1]) @ t["w1"].t()
    e1 = torch.where(z1 > 0, z1, torch.exp(z1) - 1)
    s1 = stats(e1, t["rm1"], t["rv1"])
    return dict(z1=z1, mean0=s0["mean"], invstd0=s0["invstd"], mean1=s1["mean"], invstd1=s1["invstd"], rm0=s0["rm"], rv0=s0["rv"],
                rm1=s1["rm"], rv1=s1["rv"])


def emu_lift_bwd(c, t, st):
    rows = c["rows"]
    z0, e0 = lift_e0(t)
    g0, b0 = t["bn0"][0], t["bn0"][1]
    mu, istd = st
    a = g0 * istd
    y0 = a * (e0 - mu) + b0
    gw1 = t["dz1"].t() @ y0
    dy0 = t["dz1"] @ t["w1"]
    xhat = (e0 - mu) * istd
    db = dy0.double().sum(0).float()
    dg = (dy0 * xhat).double().sum(0).float()
    inv_r = torch.tensor(1.0 / rows, dtype=f32)
    dz0 = a * (dy0 - db * inv_r - xhat * (dg * inv_r)) * torch.where(z0 > 0, torch.ones(()), torch.exp(z0))
    gw0t = (t["x3"].t().double() @ dz0.double()).float()
    return dict(grad_w0_t=gw0t, grad_w1=gw1, dgamma0=dg, dbeta0=db)


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(T, "DEV", "cpu")
    for name, fn in (("run_fwd", emu_fwd), ("run_bwd", emu_bwd), ("run_wgrad", emu_wgrad), ("run_gather_fwd", emu_gather_fwd),
                     ("run_gather_wgrad", emu_gather_wgrad), ("run_lift_eval", emu_lift_eval), ("run_lift_train", emu_lift_train),
                     ("run_lift_bwd", emu_lift_bwd)):
        monkeypatch.setattr(T, name, fn)


CHECKS = dict(fwd=T.test_linear_bn_fwd, bwd=T.test_linear_bn_bwd, wgrad=T.test_linear_wgrad, gather_fwd=T.test_linear_bn_fwd_gather,
              gather_wgrad=T.test_linear_wgrad_gather, lift_eval=T.test_lift_elu_fwd_eval, lift_eval_bn=T.test_lift_elu_fwd_eval,
              lift_train=T.test_lift_elu_bn_fwd, lift_bwd=T.test_lift_elu_bn_bwd)


@pytest.mark.parametrize("kind", sorted(CHECKS))
def test_fp32_evaluation_passes_the_checks_of_the_gpu_suite(on_host, kind):
    ran = 0
    for c in gc.sweep_cases(kind):
        if c.get("rows", c.get("clouds", 0) * c.get("rows_per_cloud", 0)) <= MAX_ROWS:
            try:
                CHECKS[kind](c)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (gc.case_id(c), e))
            ran += 1
    assert ran >= 10
