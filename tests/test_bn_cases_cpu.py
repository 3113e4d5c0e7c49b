"""The references and bounds of tests/bn_cases.py checked on the host: a plain fp32 torch evaluation of every entry point of
csrc/mlp.hip (same formulas, sums in fp64 as the kernels' last stage) takes the place of the library call in the checks of
tests/test_bn_abi.py, at the cases of at most 1100 rows.  The exact family must come out bit for bit and the rounding family inside the
derived bounds: a reference or a bound that is wrong fails here, without a GPU, before it can be blamed on a kernel.  The dropout mask of
the stand-in is bn_cases.drop_keep itself, so this module says nothing about the mask; it checks the seed arithmetic against a second,
plain-integer splitmix64 and that the 64-bit vector index reaches the hash."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as bc  # noqa: E402
import test_bn_abi as T  # noqa: E402

f32 = torch.float32
MAX_ROWS = 1100


def elu32(x, on):
    return torch.where(x > 0, x, torch.exp(x) - 1.0) if on else x


def stats32(e, rm, rv, mom):
    rows = e.shape[0]
    mean = e.double().sum(0) / rows
    var = ((e * e).double().sum(0) / rows - mean * mean).clamp(min=0)
    o = dict(mean=mean.float(), invstd=(1.0 / torch.sqrt(var + float(np.float32(bc.EPS)))).float(), rm=None, rv=None)
    m = torch.tensor(mom, dtype=f32)
    if rm is not None:
        o["rm"], o["rv"] = (1 - m) * rm + m * mean.float(), (1 - m) * rv + m * var.float()
    return o


def apply32(x, gamma, beta, mean, invstd, relu, mult=None):
    h = (gamma * invstd) * (elu32(x, relu & 2) - mean) + beta
    if relu & 1:
        h = h.clamp(min=0)
    return h if mult is None else h * mult


def bwd32(x, dy, gamma, beta, mean, invstd, relu, dgamma=None, dbeta=None, mult=None):
    rows = x.shape[0]
    e, a = elu32(x, relu & 2), gamma * invstd
    dh = dy if mult is None else dy * mult
    if relu & 1:
        dh = torch.where(a * (e - mean) + beta > 0, dh, torch.zeros(()))
    xhat = (e - mean) * invstd
    if dgamma is None:
        dbeta, dgamma = dh.double().sum(0).float(), (dh * xhat).double().sum(0).float()
    inv_r = torch.tensor(1.0, dtype=f32) / torch.tensor(float(rows), dtype=f32)
    d = a * (dh - dbeta * inv_r - xhat * (dgamma * inv_r))
    if relu & 2:
        d = d * torch.where(x > 0, torch.ones(()), torch.exp(x))
    return dict(dx=d, dgamma=dgamma, dbeta=dbeta, colsum=d.double().sum(0).float())


def emu_stats(c, t, mom=None):
    return stats32(t["x"], t["rm"], t["rv"], T.momentum(c) if mom is None else mom)


def emu_train(c, t):
    o = stats32(elu32(t["x"], c["relu"] & 2), t["rm"], t["rv"], T.momentum(c))
    o["y"] = apply32(t["x"], t["gamma"], t["beta"], o["mean"], o["invstd"], c["relu"])
    return o


def emu_eval(c, t):
    return dict(y=apply32(t["x"], *t["bn"], c["relu"]))


def emu_bwd(c, t):
    o = bwd32(t["x"], t["dy"], *t["bn"], c["relu"])
    if not c["colsum"]:
        o["colsum"] = None
    return o


def emu_bwd_dx(c, t):
    return dict(dx=bwd32(t["x"], t["dy"], *t["bn"], c["relu"], t["dgamma"], t["dbeta"])["dx"])


def emu_drop(c, t):
    rows, ch = c["rows"], c["c"]
    thresh, scale = bc.drop_threshold(c["rate"])
    seeds = [bc.drop_seed(T.STATE0 + ch, c["salt"], T.CALLS_BEFORE + n) for n in (1, 2)]
    mults = [torch.from_numpy(bc.drop_keep(rows, ch, s, thresh)).float() * float(scale) for s in seeds]
    o = stats32(elu32(t["x"], c["relu"] & 2), None, None, 0.0)
    for n in (1, 2):
        o["y%d" % n] = apply32(t["x"], t["gamma"], t["beta"], o["mean"], o["invstd"], c["relu"], mults[n - 1])
        o["seed%d" % n] = torch.tensor([T._i64(seeds[n - 1])], dtype=torch.int64)
    b = bwd32(t["x"], t["dy"], *t["bn"], c["relu"], mult=mults[1])
    o.update(dx=b["dx"], dgamma=b["dgamma"], dbeta=b["dbeta"], state=torch.tensor([T._i64(T.STATE0 + ch), T.CALLS_BEFORE + 2], dtype=torch.int64))
    return o


def emu_pool(c, t):
    g, k, ch = c["groups"], c["k"], c["c"]
    o = dict(mean=None, invstd=None, rm=None, rv=None)
    if c["training"]:
        o = stats32(t["z"], t["rm"], t["rv"], T.momentum(c))
        used = (t["gamma"], t["beta"], o["mean"], o["invstd"])
    else:
        used = t["bn"]
    o["pooled"], idx = T.first_argmax(apply32(t["z"], *used, 1).view(g, k, ch))
    o["argmax"] = idx.to(torch.uint8)
    _, _, idx_b = T.pool_reference(c, t["z"], *t["bn"])
    onehot = torch.zeros(g, k, ch).scatter_(1, idx_b[:, None, :], t["dp"][:, None, :]).view(g * k, ch)
    b = bwd32(t["z"], onehot, *t["bn"], 1)
    o.update(dx=b["dx"], dgamma=b["dgamma"], dbeta=b["dbeta"], colsum=b["colsum"] if c["colsum"] else None)
    return o


def emu_narrow(c, t):
    acc = t["g"][:, :1] * t["w"][0][None, :]
    for j in range(1, c["cout"]):
        acc = acc + t["g"][:, j:j + 1] * t["w"][j][None, :]
    return dict(dx=acc)


@pytest.fixture
def on_host(monkeypatch):
    monkeypatch.setattr(T, "DEV", "cpu")
    for name, fn in (("run_stats", emu_stats), ("run_train", emu_train), ("run_eval", emu_eval), ("run_bwd", emu_bwd), ("run_bwd_dx", emu_bwd_dx),
                     ("run_drop", emu_drop), ("run_pool", emu_pool), ("run_narrow", emu_narrow)):
        monkeypatch.setattr(T, name, fn)


CHECKS = dict(stats=T.test_bn_stats, train=T.test_bn_relu_fwd_train, eval=T.test_bn_relu_fwd_eval, bwd=T.test_bn_relu_bwd, bwd_dx=T.test_bn_relu_bwd_dx,
              drop=T.test_bn_dropout, pool=T.test_bn_relu_maxpool, narrow=T.test_narrow_linear_dx)


@pytest.mark.parametrize("kind", sorted(CHECKS))
def test_fp32_evaluation_passes_the_checks_of_the_gpu_suite(on_host, kind):
    ran = 0
    for c in bc.cases_of(kind):
        if c.get("rows", c.get("groups", 0) * c.get("k", 0)) <= MAX_ROWS:
            try:
                CHECKS[kind](c)
            except AssertionError as e:
                raise AssertionError("%s: %s" % (bc.case_id(c), e))
            ran += 1
    assert ran >= 4


def test_a_wrong_stand_in_fails_the_checks(on_host, monkeypatch):
    """the checks are not vacuous on the host either: `>=` for `>` in the backward mask, and a last row left out of the sums"""
    c = bc._case("bwd", rows=300, c=7, relu=1, ld=0, colsum=0)

    def loose_mask(c, t):
        e, a = t["x"], t["bn"][0] * t["bn"][3]
        dh = torch.where(a * (e - t["bn"][2]) + t["bn"][1] >= 0, t["dy"], torch.zeros(()))
        o = emu_bwd(c, t)
        o["dbeta"] = dh.double().sum(0).float()
        return o

    monkeypatch.setattr(T, "run_bwd", loose_mask)
    with pytest.raises(AssertionError):
        T.test_bn_relu_bwd(c)
    monkeypatch.setattr(T, "run_stats", lambda c, t, mom=None: stats32(t["x"][:-1], t["rm"], t["rv"], T.momentum(c)))
    with pytest.raises(AssertionError):
        T.test_bn_stats(bc._case("stats", rows=300, c=7))


def test_seed_and_wide_index_of_the_restated_dropout():
    """splitmix64 against its published test vector (seed 1234567: first output 6457827717110365317), and rows 2^32 / cv apart draw
    different masks: the high word of the vector index reaches the hash"""
    assert bc.drop_seed(1234567, 0, 1) == 6457827717110365317
    seed = bc.drop_seed(7, 3, 1)
    for ch in (8, 7):
        cv = ch // 4 if ch % 4 == 0 else ch
        near, far = bc.drop_keep(64, ch, seed, 32768), bc.drop_keep(64, ch, seed, 32768, row0=(1 << 32) // cv * cv // cv)
        if (1 << 32) % cv == 0:
            assert not np.array_equal(near, far)
        assert 0.3 < near.mean() < 0.7 and 0.3 < far.mean() < 0.7
    assert bc.drop_threshold(0.0)[0] == 0 and bc.drop_threshold(0.99999)[0] == 65535 and bc.drop_threshold(0.999995)[0] == 65535
    assert bc.drop_threshold(0.25) == (16384, np.float32(1.0) / np.float32(0.75))
