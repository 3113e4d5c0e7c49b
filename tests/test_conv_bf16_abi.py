"""Kernel-level parity of csrc/conv_nhwc_bf16.hip through the C ABI (ctypes on _lib.lib(), no Python routing in between) against the
references and bounds of tests/conv_bf16_cases.py.  Inputs sit between NaN bands, the output is a slice of a sentinel-filled buffer
pre-filled with NaN: a read or a write outside a tensor, or an element never written, shows; the columns beside
[y_col, y_col + cout) must keep the sentinel.  The weights reach the kernel through hf_f32_to_bf16.  Every call is made twice and
repeats its bits.  The rounding family is held to its derived bound (the worst ratio is printed), the exact family and the launch-regime
cases are compared bit for bit."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bf16_cases as cb  # noqa: E402
from abi_harness import NAN, SENTINEL, Arena, In, abi, call, same, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def p_of(i):
    return None if i is None else i.p


def bf16_weights(wt, off):
    """wt (9, cout, cin) float32 array -> (the device buffer, a pointer to its bf16 copy made by hf_f32_to_bf16); off: the copy sits
    one element past a 16-byte boundary"""
    _lib, L = abi()
    src = In(DEV, wt)
    buf = torch.zeros(wt.size + 16, dtype=torch.bfloat16, device=DEV)
    p = buf.data_ptr() + (2 if off else 0)
    assert p % 16 == (2 if off else 0)
    call(L.hf_f32_to_bf16(wt.size, src.p, ctypes.c_void_p(p), _lib.stream_ptr()), "hf_f32_to_bf16")
    return buf, ctypes.c_void_p(p)


def run(c, t):
    """one call of a case -> the (rows, cout) slice it wrote"""
    _lib, L = abi()
    stride, col = cb.slice_of(c)
    rows = c["b"] * c["h"] * c["w"] * (4 if c["mode"] == "up" else 1)
    a = Arena(DEV)
    wide = a.out((rows, stride))
    wide[:, col:col + c["cout"]] = NAN
    x = In(DEV, t["x"], c["off"] == "x")
    wbuf, wp = bf16_weights(t["wt"], c["off"] == "wt")
    sub, scale, shift = (None if t[k] is None else In(DEV, t[k].astype("float32")) for k in ("in_sub", "scale", "shift"))
    y = ctypes.c_void_p(wide.data_ptr())
    if c["mode"] == "conv":
        call(L.hf_conv3x3_nhwc_bf16(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, p_of(sub), wp, p_of(scale), p_of(shift),
                                    int(c["relu"]), y, stride, col, _lib.stream_ptr()), "hf_conv3x3_nhwc_bf16")
    else:
        call(L.hf_upconv3x3s2_nhwc_bf16(c["b"], c["h"], c["w"], c["cin"], c["cout"], x.p, wp, p_of(scale), p_of(shift), int(c["relu"]), y,
                                        stride, col, _lib.stream_ptr()), "hf_upconv3x3s2_nhwc_bf16")
    a.check()
    beside = torch.cat([wide[:, :col], wide[:, col + c["cout"]:]], dim=1)
    assert bool((beside == SENTINEL).all()), "a column outside [y_col, y_col + cout) was written"
    del wbuf
    return wide[:, col:col + c["cout"]].clone()


def entry(c):
    return "hf_conv3x3_nhwc_bf16" if c["mode"] == "conv" else "hf_upconv3x3s2_nhwc_bf16"


def check_round(mode, name):
    c, t, y, bound, _ = cb.small_case("round", mode, name)
    got = run(c, t)
    assert torch.equal(got, run(c, t)), "two calls differ"
    within(got, y.to(DEV), bound.to(DEV), entry(c), "cin %d" % c["cin"])
    if c["relu"]:
        assert bool((got >= 0).all())


def check_exact(mode, name):
    c, t, y, _, smax = cb.small_case("exact", mode, name)
    assert cb.exact_condition(smax, t)
    got = run(c, t)
    assert torch.equal(got, run(c, t)), "two calls differ"
    same(got, y.to(DEV), "%s %s %s" % (cb.instantiation(c), mode, name))


@pytest.mark.parametrize("name", list(cb.ROUND_CONV_CASES))
def test_conv3x3_bf16(name):
    check_round("conv", name)


@pytest.mark.parametrize("name", list(cb.ROUND_UPCONV_CASES))
def test_upconv3x3s2_bf16(name):
    check_round("up", name)


@pytest.mark.parametrize("name", list(cb.EXACT_CONV_CASES))
def test_conv3x3_bf16_exact(name):
    check_exact("conv", name)


@pytest.mark.parametrize("name", list(cb.EXACT_UPCONV_CASES))
def test_upconv3x3s2_bf16_exact(name):
    check_exact("up", name)


@pytest.mark.parametrize("name", list(cb.REGIME_CASES))
def test_bf16_large_grid_regime_exact(name):
    """exact inputs on a grid of more workgroups than the chip holds at once, the last tile ragged; the fp64 tap sums are formed on
    the device by torch, not by this library"""
    c = cb.REGIME_CASES[name]
    assert cb.workgroups(c) > 8 * cb.NUM_CU and (c["b"] * c["h"] * c["w"]) % cb.ROW_TILE
    t = cb.exact_inputs(name, c)
    got = run(c, t)
    assert torch.equal(got, run(c, t)), "two calls differ"
    y, _, smax = cb.case_reference(c, t, device=DEV)
    assert cb.exact_condition(smax, t)
    same(got, y, "%s regime %s" % (cb.instantiation(c), name))


def test_scalar_path_for_alignment_alone_gives_the_vector_path_bits():
    """x, then wt_bf16, one element past a 16-byte boundary: the same sums in the same order, the same bits as the aligned call"""
    for name in ("b1h12w22_ci36_co40_off_x", "b1h12w22_ci36_co40_off_wt"):
        c, t, _, _, _ = cb.small_case("round", "conv", name)
        aligned = dict(c, off=None)
        assert cb.instantiation(aligned) != cb.instantiation(c)
        assert torch.equal(run(c, t), run(aligned, t)), name
