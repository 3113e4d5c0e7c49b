"""tests/conv_bf16_cases.py checked against itself on any machine with the library built, and what of the bf16 image pyramid needs no
GPU: the case ids, the reference against a host emulation of the kernel's arithmetic, the restated dispatch rule against the source,
the image_precision scope, the refusals of the public entry points and the HF_EINVAL cases of both entry points."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_bf16_cases as cb  # noqa: E402
from kernel_asm import CSRC  # noqa: E402


def test_case_ids_are_unique_and_every_family_is_present():
    ids = [c["id"] for c in cb.abi_cases()]
    assert len(ids) == len(set(ids))
    assert {c["family"] for c in cb.abi_cases()} == {"round", "exact", "regime"}


def test_tables_hold_what_they_must():
    couts = {c["cout"] for c in cb.ROUND_CONV_CASES.values()}
    for edge in cb.COL_TILES:
        assert {edge - 1, edge} <= couts and (edge == 256 or edge + 1 in couts)
    assert {32, 40, 256} <= couts
    assert {c["cin"] for c in cb.ROUND_CONV_CASES.values()} == {3, 4, 36, 64, 256}
    assert {(c["b"], c["h"], c["w"]) for c in cb.ROUND_CONV_CASES.values()} == {(2, 5, 7), (1, 12, 22), (3, 1, 1)}
    assert {(c["sub"], c["affine"], c["relu"], c["slice"]) for c in cb.ROUND_CONV_CASES.values()} == {tuple(map(bool, f)) for f in cb.FLAG_PATTERNS}
    assert {c["off"] for c in cb.ROUND_CONV_CASES.values()} == {None, "x", "wt"}
    assert all(c["slice"] for c in cb.ROUND_UPCONV_CASES.values())
    assert {(c["b"], c["h"], c["w"], c["cin"], c["cout"]) for c in cb.ROUND_UPCONV_CASES.values()} == \
        {(b, h, w, ci, co) for b, h, w in ((2, 3, 5), (1, 1, 1)) for ci in (36, 256) for co in (32, 128)}
    assert cb.stages(dict(mode="conv", cin=3)) == (1,) and cb.stages(dict(mode="conv", cin=36)) == (6,)


def test_restated_dispatch_rules_stand_in_the_source():
    with open(os.path.join(CSRC, cb.SOURCE)) as f:
        text = f.read()
    for rule in cb.SOURCE_RULES:
        assert rule in text, rule


ROUND_SAMPLE = (("conv", "b2h5w7_ci3_co1"), ("conv", "b1h12w22_ci36_co40"), ("conv", "b1h12w22_ci256_co256"), ("conv", "b1h12w22_ci36_co40_off_x"),
                ("up", "b2h3w5_ci36_co32"), ("up", "b1h1w1_ci256_co128"))


@pytest.mark.parametrize("mode,name", ROUND_SAMPLE)
def test_fp32_emulation_lies_inside_the_bound(mode, name):
    c, t, y, bound, _ = cb.small_case("round", mode, name)
    got = cb.emulate(c, t)
    ratio = float(((got.double() - y).abs() / bound).max())
    print("%s %s: max |emulation - ref64| / bound = %.3g" % (mode, name, ratio))
    assert ratio <= 1.0
    # and the bound is one: the same sums on operands that are not rounded to bf16 lie outside it
    plain = dict(t, in_sub=None)
    if c["cin"] >= 36 and not c["sub"]:
        z, _ = (cb.upconv_tap_sum if mode == "up" else cb.conv_tap_sum)(torch.from_numpy(t["x"].astype(np.float64)), torch.from_numpy(t["wt"].astype(np.float64)))
        sc = 1.0 if plain["scale"] is None else torch.from_numpy(t["scale"].astype(np.float64))
        sh = 0.0 if plain["shift"] is None else torch.from_numpy(t["shift"].astype(np.float64))
        full = (z * sc + sh).reshape(-1, c["cout"])
        full = full.clamp(min=0.0) if c["relu"] else full
        assert float(((full - y).abs() / bound).max()) > 1.0


@pytest.mark.parametrize("mode", ["conv", "up"])
def test_exact_family_emulation_is_bit_equal(mode):
    table = cb.TABLES["exact"][mode]
    for name in list(table)[::7] + [n for n in table if "_off_" in n][:2]:
        c, t, y, _, smax = cb.small_case("exact", mode, name)
        assert cb.exact_condition(smax, t), name
        xb, wb = cb.operands(torch.from_numpy(t["x"]), torch.from_numpy(t["wt"]), None if t["in_sub"] is None else torch.from_numpy(t["in_sub"]))
        assert torch.equal(wb, torch.from_numpy(t["wt"])), "the exact family's weights are bf16 numbers"
        assert float(xb.abs().max()) <= 10.0 and torch.equal(xb, xb.round())
        assert torch.equal(cb.emulate(c, t), y.float()), name


def test_every_exact_and_regime_case_meets_the_partial_sum_condition():
    # S <= 80 * 9 cin whatever the draw; the regime cases' own S is asserted on the device next to their reference
    for table in (cb.EXACT_CONV_CASES, cb.EXACT_UPCONV_CASES, cb.REGIME_CASES):
        for c in table.values():
            assert 2 * (80 * 9 * c["cin"]) + 8 < 2 ** 24


# ------------------------------------------------------------------------------------------------ the scope
def test_image_precision_scope():
    from heterofusionrcnn_amd import image_pyramid as ip
    assert ip.IMAGE_PRECISIONS == ("fp32", "bf16") and ip.IMAGE_BRANCHES == ("torch", "native")
    assert ip.image_precision_name() == "fp32" and ip._IMAGE_PRECISION == ["fp32"]
    with ip.image_precision("bf16"):
        assert ip.image_precision_name() == "bf16" and ip.image_branch_name() == "torch"
        with ip.image_precision("fp32"):
            assert ip.image_precision_name() == "fp32"
        assert ip.image_precision_name() == "bf16"
    assert ip.image_precision_name() == "fp32"
    with pytest.raises(KeyError):
        with ip.image_precision("bf16"):
            raise KeyError("inside")
    assert ip.image_precision_name() == "fp32"
    with pytest.raises(ValueError, match="image precision"):
        ip.image_precision("fp16")
    with pytest.raises(ValueError):
        ip.image_branch("bf16")
    assert ip.NATIVE_BF16_LAUNCHES == [ip.NATIVE_BF16_LAUNCHES[0]]


def _no_model(*a, **k):
    raise AssertionError("a model was touched before the refusal")


def test_public_functions_refuse_bf16_on_the_torch_branch(monkeypatch, tmp_path):
    from heterofusionrcnn_amd import detect, export_rpn, image_pyramid, validate
    monkeypatch.setattr(export_rpn, "load_rpn", _no_model)
    monkeypatch.setattr(detect, "load_models", _no_model)
    monkeypatch.setattr(detect, "load_rpn", _no_model)
    monkeypatch.setattr(validate, "load_rcnn", _no_model)
    d = str(tmp_path)
    for call in (lambda **k: detect.detect(d, "rpn.pt", "rcnn.pt", d, **k), lambda **k: export_rpn.export(d, "rpn.pt", d, **k),
                 lambda **k: validate.validate_rpn(d, "rpn.pt", **k), lambda **k: validate.validate_rcnn(d, d, "rcnn.pt", **k)):
        with pytest.raises(ValueError, match="image_branch='native'"):
            call(image_precision="bf16")
        with pytest.raises(ValueError, match="image_branch='native'"):
            call(image_precision="bf16", image_branch="torch")
        with pytest.raises(ValueError, match="image precision"):
            call(image_precision="fp16", image_branch="native")
    assert image_pyramid.image_precision_name() == "fp32" and image_pyramid.image_branch_name() == "torch"


def test_parsers_refuse_bf16_on_the_torch_branch(monkeypatch, capsys):
    from heterofusionrcnn_amd import detect, export_rpn, validate
    monkeypatch.setattr(detect, "detect", _no_model)
    monkeypatch.setattr(export_rpn, "export", _no_model)
    monkeypatch.setattr(validate, "validate_rpn", _no_model)
    monkeypatch.setattr(validate, "validate_rcnn", _no_model)
    for main, argv in ((detect.main, ["d", "rpn.pt", "rcnn.pt", "out"]), (export_rpn.main, ["d", "rpn.pt", "out"]),
                       (validate.main, ["rpn", "d", "rpn.pt"]), (validate.main, ["rcnn", "d", "handoff", "rcnn.pt"])):
        for extra in (["--image-precision", "bf16"], ["--image-precision", "bf16", "--image-branch", "torch"], ["--image-precision", "fp16"]):
            with pytest.raises(SystemExit) as e:
                main(argv + extra)
            assert e.value.code == 2
            assert "--image-precision" in capsys.readouterr().err
    assert detect.build_parser().parse_args(["d", "a", "b", "o"]).image_precision == "fp32"
    assert detect.build_parser().parse_args(["d", "a", "b", "o", "--image-branch", "native", "--image-precision", "bf16"]).image_precision == "bf16"
    assert validate.build_parser().parse_args(["rpn", "d", "m"]).image_precision == "fp32"


def test_einval_before_any_hip_call():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    one = ctypes.c_void_p(16)
    bad = cb.einval_calls(L, one)
    assert len(bad) == 2 * 14 + 1
    for what, status in bad.items():
        assert status == _lib.HF_EINVAL, what
