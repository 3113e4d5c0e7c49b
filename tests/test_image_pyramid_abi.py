"""Kernel-level parity of csrc/conv_nhwc.hip through the C ABI (ctypes on _lib.lib(), no Python routing in between) against the
references and bounds of tests/image_pyramid_cases.py.  Inputs sit between NaN bands, outputs are slices of sentinel-filled buffers
and are pre-filled with NaN: a read or a write outside a tensor, or an element never written, shows.  An output slice is the
column range [y_col, y_col + cout) of rows y_stride wide: the other columns hold the sentinel before the call and must hold it
afterwards.  Every call is made twice and repeats its bits.  The exact family and the launch-regime cases (persistent grids whose
workgroups walk two and three tiles, grid-stride pool launches) are compared bit for bit, abi_harness.same."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402
from abi_harness import NAN, SENTINEL, Arena, In, abi, call, dev64, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def inp(a):
    """the tables are read-only arrays: torch wants a writable one"""
    return None if a is None else In(DEV, a.copy())


def p_of(i):
    return None if i is None else i.p


def run_conv(kind, name):
    """-> the (rows, cout) slice the call wrote; the arena and the columns beside the slice are checked"""
    _lib, L = abi()
    c = (pc.CONV_CASES if kind == "conv" else pc.UPCONV_CASES)[name]
    t = pc.conv_inputs(kind, name)
    stride, col = pc.slice_of(c)
    rows = c["b"] * c["h"] * c["w"] * (4 if kind == "upconv" else 1)
    a = Arena(DEV)
    wide = a.out((rows, stride))
    wide[:, col:col + c["cout"]] = NAN
    x, wt, sub, scale, shift = (inp(t[k]) for k in ("x", "wt", "in_sub", "scale", "shift"))
    y = ctypes.c_void_p(wide.data_ptr())
    if kind == "conv":
        call(L.hf_conv3x3_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), wt.p, p_of(scale), p_of(shift), int(c["relu"]),
                               y, stride, col, _lib.stream_ptr()), "hf_conv3x3_nhwc")
    else:
        call(L.hf_upconv3x3s2_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, wt.p, p_of(scale), p_of(shift), int(c["relu"]), y,
                                   stride, col, _lib.stream_ptr()), "hf_upconv3x3s2_nhwc")
    a.check()
    beside = torch.cat([wide[:, :col], wide[:, col + c["cout"]:]], dim=1)
    assert bool((beside == SENTINEL).all()), "a column outside [y_col, y_col + cout) was written"
    return wide[:, col:col + c["cout"]].clone()


def check_conv(kind, name):
    c = (pc.CONV_CASES if kind == "conv" else pc.UPCONV_CASES)[name]
    r = pc.conv_reference(kind, name)
    got = run_conv(kind, name)
    assert torch.equal(got, run_conv(kind, name)), "two calls differ"
    within(got, dev64(DEV, r["y"].numpy()), dev64(DEV, r["bound"].numpy()),
           "hf_conv3x3_nhwc" if kind == "conv" else "hf_upconv3x3s2_nhwc", "cin %d" % c["cin"])
    if c["relu"]:
        assert bool((got >= 0).all())


@pytest.mark.parametrize("name", list(pc.CONV_CASES))
def test_conv3x3(name):
    check_conv("conv", name)


@pytest.mark.parametrize("name", list(pc.UPCONV_CASES))
def test_upconv3x3s2(name):
    check_conv("upconv", name)


def test_conv3x3_off_the_16_byte_boundary_takes_the_scalar_path():
    """x one float past a 16-byte boundary: the scalar staging path, the same sums in the same order, the same bits"""
    _lib, L = abi()
    name = "b1h12w22_ci36_co40"
    c, t = pc.CONV_CASES[name], pc.conv_inputs("conv", name)
    stride, col = pc.slice_of(c)
    rows = c["b"] * c["h"] * c["w"]
    outs = []
    for off in (False, True):
        a = Arena(DEV)
        wide = a.out((rows, stride))
        wide[:, col:col + c["cout"]] = NAN
        x = In(DEV, t["x"].copy(), off)
        wt, sub, scale, shift = (inp(t[k]) for k in ("wt", "in_sub", "scale", "shift"))
        call(L.hf_conv3x3_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), wt.p, p_of(scale), p_of(shift), int(c["relu"]),
                               ctypes.c_void_p(wide.data_ptr()), stride, col, _lib.stream_ptr()), "hf_conv3x3_nhwc")
        a.check()
        outs.append(wide[:, col:col + c["cout"]].clone())
    assert not torch.isnan(outs[0]).any() and torch.equal(outs[0], outs[1])


def check_pool(name, c, x):
    _lib, L = abi()
    want = torch.nn.functional.max_pool2d(torch.from_numpy(x.copy()).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous()
    assert torch.equal(want, pc.pool_ref(torch.from_numpy(x.copy())))
    for stride, col in ((2 * c["c"] + 4, c["c"]), (c["c"], 0)):
        rows = x.reshape(-1, c["c"])
        wide = np.full((rows.shape[0], stride), np.nan, dtype=np.float32)      # a read beside the slice is a NaN, and a NaN wins
        wide[:, col:col + c["c"]] = rows
        results = []
        for _ in range(2):
            a = Arena(DEV)
            y = a.out((want.numel(),))
            y.fill_(NAN)
            src = In(DEV, wide)
            call(L.hf_maxpool2x2_nhwc(c["b"], c["h"], c["w"], c["c"], src.p, stride, col, ctypes.c_void_p(y.data_ptr()),
                                      _lib.stream_ptr()), "hf_maxpool2x2_nhwc")
            a.check()
            results.append(y.clone().reshape(want.shape))
        assert torch.equal(results[0], results[1]), "two calls differ"
        assert torch.equal(results[0].cpu(), want), (name, stride, col)


@pytest.mark.parametrize("name", list(pc.POOL_CASES))
def test_maxpool2x2_is_torch_bit_for_bit(name):
    check_pool(name, pc.POOL_CASES[name], pc.pool_inputs(name))


@pytest.mark.parametrize("name", list(pc.REGIME_POOL_CASES))
def test_maxpool2x2_grid_stride_regime_is_torch_bit_for_bit(name):
    """more items than the capped grid has lanes: every lane takes a second item, from a slice and dense"""
    c = pc.REGIME_POOL_CASES[name]
    assert pc.pool_strides(c, True) and pc.pool_strides(c, False)
    check_pool(name, c, pc.regime_pool_inputs(name)["x"])


# ------------------------------------------------------------------------------------------------ the exact family
def run_exact(c, t):
    """one call of an exact-family case (mode "conv" or "up") -> the (rows, cout) slice it wrote; c["off"]: the operand that sits
    one float past a 16-byte boundary"""
    _lib, L = abi(unset=("HF_GEMM_ROUNDS",))
    stride, col = pc.slice_of(c)
    rows = pc.conv_rows(c) * (4 if c["mode"] == "up" else 1)
    a = Arena(DEV)
    wide = a.out((rows, stride))
    wide[:, col:col + c["cout"]] = NAN
    x, wt = In(DEV, t["x"], c["off"] == "x"), In(DEV, t["wt"], c["off"] == "wt")
    sub, scale, shift = (None if t[k] is None else In(DEV, t[k]) for k in ("in_sub", "scale", "shift"))
    y = ctypes.c_void_p(wide.data_ptr())
    if c["mode"] == "conv":
        call(L.hf_conv3x3_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), wt.p, p_of(scale), p_of(shift), int(c["relu"]),
                               y, stride, col, _lib.stream_ptr()), "hf_conv3x3_nhwc")
    else:
        call(L.hf_upconv3x3s2_nhwc(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, wt.p, p_of(scale), p_of(shift), int(c["relu"]), y,
                                   stride, col, _lib.stream_ptr()), "hf_upconv3x3s2_nhwc")
    a.check()
    if col:
        assert bool((wide[:, :col] == SENTINEL).all()) and bool((wide[:, col + c["cout"]:] == SENTINEL).all()), \
            "a column outside [y_col, y_col + cout) was written"
    return wide[:, col:col + c["cout"]].clone()


def check_exact(mode, name):
    c, t, y, smax = pc.exact_conv_case(mode, name)
    assert pc.exact_condition(smax)
    got = run_exact(c, t)
    assert torch.equal(got, run_exact(c, t)), "two calls differ"
    same(got, y.to(DEV), "%s %s %s" % (pc.conv_instantiation(c, c["off"]), mode, name))


@pytest.mark.parametrize("name", list(pc.EXACT_CONV_CASES))
def test_conv3x3_exact(name):
    check_exact("conv", name)


@pytest.mark.parametrize("name", list(pc.EXACT_UPCONV_CASES))
def test_upconv3x3s2_exact(name):
    check_exact("up", name)


def check_regime(c, name):
    """exact inputs at a production grid size; the fp64 tap sums are formed on the device by torch, not by this library"""
    fewest, most = pc.conv_tiles(c)
    assert fewest >= 2 and most >= 3 and pc.conv_rows(c) % pc.FWD_ROWS
    t = pc.exact_conv_inputs(name, c)
    got = run_exact(c, t)
    assert torch.equal(got, run_exact(c, t)), "two calls differ"
    y, smax = pc.exact_conv_reference(c, t, device=DEV)
    assert pc.exact_condition(smax)
    same(got, y, "%s %s regime %s" % (pc.conv_instantiation(c), c["mode"], name))


@pytest.mark.parametrize("name", list(pc.REGIME_CONV_CASES))
def test_conv3x3_persistent_grid_regime_exact(name):
    check_regime(pc.REGIME_CONV_CASES[name], name)


@pytest.mark.parametrize("name", list(pc.REGIME_UPCONV_CASES))
def test_upconv3x3s2_persistent_grid_regime_exact(name):
    check_regime(pc.REGIME_UPCONV_CASES[name], name)
