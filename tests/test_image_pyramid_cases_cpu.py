"""CPU checks of tests/image_pyramid_cases.py and of what the image pyramid's native route does without a GPU: the fp64 tap-sum
restatements against torch's own convolutions, image_pyramid.pack against the module's layers in eval mode, the case tables, the
HF_EINVAL paths of the three entry points (they return before any HIP call), the scope and its refusals."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402

RESTATEMENT = 1e-12          # fp64 against fp64 in another summation order: measured 4e-15 on sums of at most 9 * 256 terms of size ~1


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 5, 7, 3, 4), (1, 12, 22, 36, 40), (3, 1, 1, 5, 2), (1, 2, 9, 8, 3)])
def test_conv_tap_sum_is_conv2d(b, h, w, cin, cout):
    x, wt, sub = _rand(b, h, w, cin), _rand(9, cout, cin, seed=1), _rand(cin, seed=2)
    weight = wt.reshape(3, 3, cout, cin).permute(2, 3, 0, 1)                 # wt[3 ky + kx][co][ci] = weight[co, ci, ky, kx]
    for s in (None, sub):
        z, S = pc.conv_tap_sum(x, wt, s)
        xs = x if s is None else x - s
        want = F.conv2d(xs.permute(0, 3, 1, 2), weight, padding=1).permute(0, 2, 3, 1)
        assert float((z - want).abs().max()) <= RESTATEMENT
        assert float((S - F.conv2d(xs.abs().permute(0, 3, 1, 2), weight.abs(), padding=1).permute(0, 2, 3, 1)).abs().max()) <= RESTATEMENT
    # in_sub is not applied to the padding: subtracting it from a zero-padded image would differ at the border
    z, _ = pc.conv_tap_sum(x, wt, sub)
    if h > 1 or w > 1:
        padded = F.conv2d(F.pad(x.permute(0, 3, 1, 2), (1, 1, 1, 1)) - sub.view(1, -1, 1, 1), weight).permute(0, 2, 3, 1)
        assert float((z - padded).abs().max()) > 1e-3


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 3, 5, 6, 4), (1, 1, 1, 36, 8), (1, 4, 1, 3, 2)])
def test_upconv_tap_sum_is_conv_transpose2d(b, h, w, cin, cout):
    x, wt = _rand(b, h, w, cin), _rand(9, cout, cin, seed=1)
    weight = wt.reshape(3, 3, cout, cin).permute(3, 2, 0, 1)                 # wt[3 ky + kx][co][ci] = weight[ci, co, ky, kx]
    z, S = pc.upconv_tap_sum(x, wt)
    want = F.conv_transpose2d(x.permute(0, 3, 1, 2), weight, stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    assert z.shape == (b, 2 * h, 2 * w, cout) and float((z - want).abs().max()) <= RESTATEMENT
    want_s = F.conv_transpose2d(x.abs().permute(0, 3, 1, 2), weight.abs(), stride=2, padding=1, output_padding=1).permute(0, 2, 3, 1)
    assert float((S - want_s).abs().max()) <= RESTATEMENT


@pytest.mark.parametrize("b,h,w,c", [(2, 6, 10, 3), (1, 5, 7, 4), (1, 1, 4, 2)])
def test_pool_ref_is_max_pool2d(b, h, w, c):
    x = _rand(b, h, w, c)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) if h > 1 and w > 1 else x.new_zeros((b, h // 2, w // 2, c))
    assert torch.equal(pc.pool_ref(x), want)


def test_epilogue_and_bound():
    z, s = _rand(2, 3, 4, 5), _rand(2, 3, 4, 5, seed=1).abs() + 1.0
    scale, shift = _rand(5, seed=2), _rand(5, seed=3)
    y, bound = pc.epilogue(z, s, 7, scale, shift, relu=True)
    assert torch.equal(y, (z * scale + shift).clamp(min=0.0))
    want = scale.abs() * (9 * 7 + 2) * pc.U * s + 2 * pc.U * ((scale * z).abs() + shift.abs()) + pc.FLOOR
    assert torch.equal(bound, want) and bool((bound > 0).all())
    y, bound = pc.epilogue(z, s, 7)
    assert torch.equal(y, z) and torch.equal(bound, (9 * 7 + 2) * pc.U * s + 2 * pc.U * z.abs() + pc.FLOOR)


def test_case_tables_cover_what_the_kernels_branch_on():
    cases = pc.CONV_CASES
    assert {(c["b"], c["h"], c["w"]) for c in cases.values()} == {(2, 5, 7), (1, 12, 22), (3, 1, 1)}
    assert {c["cin"] for c in cases.values()} == {3, 36, 64, 256} and {c["cout"] for c in cases.values()} == {32, 40, 256}
    for key in ("cin", "cout"):          # every flag takes both values at every cin and every cout
        for v in {c[key] for c in cases.values()}:
            for flag in ("sub", "affine", "relu", "slice"):
                assert {c[flag] for c in cases.values() if c[key] == v} == {False, True}, (key, v, flag)
    assert 2 * 5 * 7 < 128 < 12 * 22 and 12 * 22 % 128 != 0                 # less than a tile; two full tiles and a partial one
    for c in pc.UPCONV_CASES.values():
        assert c["slice"] and pc.slice_of(c) == (2 * c["cout"] + 4, c["cout"])
    assert {(c["h"], c["w"]) for c in pc.UPCONV_CASES.values()} == {(3, 5), (1, 1)}
    assert {c["c"] for c in pc.POOL_CASES.values()} == {3, 32, 40} and any(c["h"] % 2 and c["w"] % 2 for c in pc.POOL_CASES.values())
    r = pc.conv_reference("conv", "first_layer_0")
    assert r["y"].shape == (70, 32) and bool((r["y"] >= 0).all()) and bool((r["bound"] > 0).all())
    assert pc.conv_reference("upconv", "b2h3w5_ci36_co32")["y"].shape == (2 * 6 * 10, 32)


# ---------------------------------------------------------------------------------------------- the restated dispatch rules
def _source(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "heterofusionrcnn_amd", "csrc", name)) as f:
        return f.read()


@pytest.mark.parametrize("name,constant,value", pc.SOURCE_CONSTANTS, ids=lambda v: str(v))
def test_constants_are_those_of_the_sources(name, constant, value):
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % constant, _source(name))
    assert found == [str(value)], "%s of %s changed: the restated rules of image_pyramid_cases.py and the regimes of its cases depend on it" % (constant, name)


@pytest.mark.parametrize("name,text", pc.SOURCE_RULES, ids=lambda v: v[:40].replace(" ", "_"))
def test_rule_literals_are_those_of_the_sources(name, text):
    assert _source(name).count(text) == 1, "the dispatch rule of %s changed: restate it in image_pyramid_cases.py (%r)" % (name, text)


def test_restated_rules():
    assert [pc.conv_nt(c) for c in (1, 32, 33, 64, 65, 128, 129, 256)] == [1, 1, 2, 2, 4, 4, 8, 8]
    assert [pc.resident_grid(nt, 10 ** 6) for nt in (1, 2, 4, 8)] == [2048, 2048, 1536, 1024] and pc.resident_grid(1, 3) == 3
    c = dict(mode="up", b=1, h=2, w=2, cin=36, cout=40)
    assert pc.conv_instantiation(c) == ("conv3x3_kernel", (2, True, 1)) and pc.conv_instantiation(c, "wt") == ("conv3x3_kernel", (2, False, 1))
    assert pc.conv_instantiation(dict(c, cin=3, mode="s2")) == ("conv3x3_kernel", (2, False, 2))
    assert pc.conv_stages(c) == (2, 3, 3, 5) and pc.conv_stages(dict(c, mode="conv")) == (11,) and pc.conv_stages(dict(cin=3)) == (1,)
    assert pc.conv_tiles(dict(b=1, h=12, w=22, cout=32)) == (1, 1) and pc.conv_tiles(dict(b=2, h=192, w=320, cout=32)) == (1, 1)
    p = dict(b=2, h=6, w=10, c=32)
    assert pc.pool_instantiation(p, True) == ("maxpool2x2_kernel", (4,)) and pc.pool_instantiation(p, False, "x") == ("maxpool2x2_kernel", (1,))
    assert pc.pool_instantiation(dict(p, c=3), True, backward=True) == ("maxpool2x2_bwd_kernel", (1,))
    assert pc.pool_items(p) == 2 * 3 * 5 * 8 and pc.pool_items(dict(b=1, h=5, w=7, c=3), backward=True) == 3 * 4 * 3 and not pc.pool_strides(p)


# ---------------------------------------------------------------------------------------------- the exact family
EXACT_TABLES = (("conv", pc.EXACT_CONV_CASES), ("up", pc.EXACT_UPCONV_CASES), ("s2", pc.EXACT_S2_CASES))


@pytest.mark.parametrize("mode,cases", EXACT_TABLES, ids=[m for m, _ in EXACT_TABLES])
def test_exact_family_is_exact_and_reaches_every_form(mode, cases):
    assert len(cases) == len(pc.EXACT_CIN) * len(pc.EXACT_COUT) + 2 * len(pc.EXACT_ALIGN_COUT)
    for name, c in cases.items():
        _, t, y, smax = pc.exact_conv_case(mode, name)
        assert c["mode"] == mode and pc.exact_condition(smax) and smax <= 9 * 256 * 10, name
        assert float((y * 8).frac().abs().max()) == 0 and torch.equal(y.float().double(), y), name
        assert set(np.unique(t["wt"])) <= {-1.0, 0.0, 1.0} and float(np.abs(t["x"]).max()) <= 8 and np.array_equal(t["x"], np.round(t["x"]))
        if c["affine"]:
            assert set(np.unique(np.abs(t["scale"]))) <= {0.5, 1.0, 2.0} and float(np.abs(t["shift"]).max()) <= 4
            assert np.array_equal(t["shift"] * 4, np.round(t["shift"] * 4))
    # all eight instantiations of the mode; the scalar form by shape and, at cin % 4 == 0, by x and by wt off the boundary
    reach = {pc.conv_instantiation(c, c["off"])[1] for c in cases.values()}
    assert reach == {(nt, vec, pc.CONV_MODES.index(mode)) for nt in (1, 2, 4, 8) for vec in (False, True)}
    for nt in (1, 2, 4, 8):
        scalar = [c for c in cases.values() if pc.conv_instantiation(c, c["off"])[1][:2] == (nt, False)]
        assert {c["off"] for c in scalar if c["cin"] % 4 == 0} == {"x", "wt"} and any(c["cin"] % 4 for c in scalar), nt
    plain = [c for c in cases.values() if c["off"] is None]
    assert {c["cin"] for c in plain} == set(pc.EXACT_CIN) and {c["cout"] for c in plain} == set(pc.EXACT_COUT)
    for key, values in (("cin", pc.EXACT_CIN), ("cout", pc.EXACT_COUT)):
        for v in values:           # every cin and every cout meets every geometry and every flag pattern the entry point has
            mine = [c for c in plain if c[key] == v]
            assert {(c["b"], c["h"], c["w"]) for c in mine} == set(pc.CONV_SHAPES), (key, v)
            for flag in ("affine", "relu", "slice") + (("sub",) if mode == "conv" else ()):
                assert {c[flag] for c in mine} == {False, True}, (key, v, flag)
    # the K axis: one stage, whole stages, a 4-wide tail, a scalar quad over two taps
    assert {pc.conv_stages(c) for c in plain if c["cin"] == 3} == ({(1,)} if mode != "up" else {(1, 1, 1, 1)})
    assert all((9 * c["cin"]) % pc.FWD_KC == 0 for c in plain if c["cin"] in (32, 256))
    assert all(c["cin"] % 4 and (2 * c["cin"]) % 4 for c in plain if c["cin"] in (5, 33))


def test_exact_references_are_torch_convolutions():
    """integers: the restatements and torch's own fp64 convolutions agree exactly, whatever order either sums in"""
    for mode, name in (("conv", "b2h5w7_ci3_co1"), ("conv", "b1h12w22_ci36_co40_off_wt"), ("up", "b2h5w7_ci3_co1"), ("up", "b1h12w22_ci36_co128_off_x"),
                       ("s2", "b2h5w7_ci3_co1"), ("s2", "b1h12w22_ci36_co256_off_x")):
        c, t, y, _ = pc.exact_conv_case(mode, name)
        x, wt = torch.from_numpy(t["x"]).double(), torch.from_numpy(t["wt"]).double()
        if c["sub"]:
            x = F.pad((x - torch.from_numpy(t["in_sub"]).double()).permute(0, 3, 1, 2), (1, 1, 1, 1)).permute(0, 2, 3, 1)
        k = wt.reshape(3, 3, c["cout"], c["cin"])
        if mode == "up":
            z = F.conv_transpose2d(x.permute(0, 3, 1, 2), k.permute(3, 2, 0, 1), stride=2, padding=1, output_padding=1)
        else:
            z = F.conv2d(x.permute(0, 3, 1, 2), k.permute(2, 3, 0, 1), stride=2 if mode == "s2" else 1, padding=0 if c["sub"] else 1)
        z = z.permute(0, 2, 3, 1)
        if c["affine"]:
            z = z * torch.from_numpy(t["scale"]).double() + torch.from_numpy(t["shift"]).double()
        z = z.clamp(min=0.0) if c["relu"] else z
        assert torch.equal(z.reshape(-1, c["cout"]), y) and bool((y != 0).any()), (mode, name)


def test_regime_cases_walk_the_persistent_grid_and_the_grid_stride_loops():
    for table in (pc.REGIME_CONV_CASES, pc.REGIME_UPCONV_CASES, pc.REGIME_S2_CASES):
        for name, c in table.items():
            fewest, most = pc.conv_tiles(c)
            # every workgroup prefetches a next tile under its last K stage, some twice; a ragged last tile; rows and images end inside tiles
            assert fewest >= 2 and most >= 3 and pc.conv_rows(c) % pc.FWD_ROWS and c["w"] % pc.FWD_ROWS and (c["h"] * c["w"]) % pc.FWD_ROWS, name
            assert pc.exact_condition(9 * c["cin"] * 10), name                 # S <= 9 cin max|x'|
    assert {pc.conv_instantiation(c) for c in pc.REGIME_CONV_CASES.values()} == {("conv3x3_kernel", a) for a in ((1, True, 0), (1, False, 0), (8, True, 0))}
    assert pc.conv_rows(pc.REGIME_CONV_CASES["nt1_vec"]) == 524547 and pc.conv_rows(pc.REGIME_CONV_CASES["nt8_vec"]) == 262654
    for table, backward in ((pc.REGIME_POOL_CASES, False), (pc.REGIME_POOL_BWD_CASES, True)):
        assert {pc.pool_instantiation(c, s, backward=backward)[1] for c in table.values() for s in (False, True)} == {(1,), (4,)}
        for name, c in table.items():
            for sliced in (False, True):
                lanes = pc.POOL_MAX_GRID * pc.POOL_THREADS
                assert lanes < pc.pool_items(c, sliced, backward) < 2 * lanes and pc.pool_strides(c, sliced, backward), name
    assert all(c["h"] % 2 and c["w"] % 2 for c in pc.REGIME_POOL_BWD_CASES.values()) and pc.REGIME_POOL_CASES["vec1"]["w"] % 2
    assert not any(pc.pool_strides(c, s) or pc.pool_strides(c, s, True) for c in pc.POOL_CASES.values() for s in (False, True))
    t = pc.regime_pool_inputs("vec1")
    assert 0.3 < float((t["x"] == 0).mean()) < 0.7


def _layer_tap_sum(layer, x):
    """x (b,h,w,cin) fp64 through a packed layer: tap sum, folded scale and shift, relu -> (b,h',w',cout)"""
    wt, scale, shift = layer["wt"].double(), layer["scale"].double(), layer["shift"].double()
    z, s = pc.upconv_tap_sum(x, wt) if layer["up"] else pc.conv_tap_sum(x, wt)
    return pc.epilogue(z, s, layer["cin"], scale, shift, relu=True)[0]


def test_pack_folds_the_module_layers():
    """the packed weights and the folded BatchNorm of every layer equal the layer itself in eval mode, in fp64"""
    from heterofusionrcnn_amd import image_pyramid
    net = pc.make_model().double()
    p = image_pyramid.pack(net)
    assert p["mean"].dtype == torch.float64 and p["mean"].tolist() == pytest.approx([92.8403, 97.7996, 93.5843])
    layers = [l for block in p["blocks"] for l in block] + p["up"] + p["fusion"]
    modules = [m for block in (net.conv1, net.conv2, net.conv3, net.conv4) for m in block] + \
        [net.upconv3, net.upconv2, net.upconv1, net.fusion3, net.fusion2, net.fusion1]
    assert len(layers) == len(modules) == 5 + 3 + 3
    assert [l["up"] for l in layers] == [False] * 5 + [True] * 3 + [False] * 3
    with torch.no_grad():
        for i, (layer, module) in enumerate(zip(layers, modules)):
            assert layer["wt"].shape == (9, layer["cout"], layer["cin"]) and layer["wt"].is_contiguous()
            x = _rand(2, 3, 5, layer["cin"], seed=i)
            want = module(x.permute(0, 3, 1, 2)).permute(0, 2, 3, 1)
            got = _layer_tap_sum(layer, x)
            assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), i


def test_pack_is_cached_until_the_state_changes():
    from heterofusionrcnn_amd import image_pyramid
    net = pc.make_model()
    p = image_pyramid.pack(net)
    assert image_pyramid.pack(net) is p
    other = pc.make_model(seed=5)
    net.load_state_dict(other.state_dict())
    q = image_pyramid.pack(net)
    assert q is not p and image_pyramid.pack(net) is q
    assert torch.equal(q["fusion"][-1]["scale"], image_pyramid.pack(other)["fusion"][-1]["scale"])
    assert not torch.equal(q["fusion"][-1]["scale"], p["fusion"][-1]["scale"])
    with torch.no_grad():
        net.fusion1[1].running_var.add_(1.0)                                  # an in-place write bumps _version
    assert image_pyramid.pack(net) is not q


def test_scope_default_and_refusals():
    from heterofusionrcnn_amd import image_pyramid
    assert image_pyramid.IMAGE_BRANCHES == ("torch", "native") and image_pyramid.image_branch_name() == "torch"
    with image_pyramid.image_branch("native"):
        assert image_pyramid.image_branch_name() == "native"
        with image_pyramid.image_branch("torch"):
            assert image_pyramid.image_branch_name() == "torch"
        assert image_pyramid.image_branch_name() == "native"
    assert image_pyramid.image_branch_name() == "torch"
    with pytest.raises(ValueError, match="image branch"):
        image_pyramid.image_branch("miopen")


def test_host_tensors_keep_the_torch_form_under_the_scope():
    """same module, same state_dict keys, same bits: a host tensor under the scope takes the default route, training mode included"""
    from heterofusionrcnn_amd import image_pyramid
    from heterofusionrcnn_amd.inference import ImgVggPyr
    net, image = pc.make_model(), pc.make_image()
    assert sorted(net.state_dict()) == sorted(ImgVggPyr(pc.MODEL_CONV).state_dict())
    with torch.no_grad():
        want = net(image)
        with image_pyramid.image_branch("native"):
            got = net(image)
    assert torch.equal(got, want)
    assert torch.equal(pc.module_forward(net, image), want)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        image_pyramid.forward_native(net, image)


def test_flows_take_the_image_branch_flag():
    import inspect
    from heterofusionrcnn_amd import detect, export_rpn, inference, validate
    for fn in (detect.detect, export_rpn.export, validate.validate_rpn, validate.validate_rcnn, inference.run_kitti_inference):
        assert inspect.signature(fn).parameters["image_branch"].default == "torch", fn
    assert detect.build_parser().parse_args(["d", "a", "b", "o", "--image-branch", "native"]).image_branch == "native"
    assert detect.build_parser().parse_args(["d", "a", "b", "o"]).image_branch == "torch"
    for stage, extra in (("rpn", []), ("rcnn", ["h"])):
        assert validate.build_parser().parse_args([stage, "d"] + extra + ["m", "--image-branch", "native"]).image_branch == "native"


def test_model_condition_holds_for_the_seed():
    """the model-level tolerance is measured against the reference (8 x the fp32 host route's own error) and must be able to see a
    swapped concat at every level: each swap moves the fp64 output by more than 10 tolerances"""
    r = pc.model_reference()
    print("max|ref64| %.3g, fp32 host error %.3g, tolerance %.3g, swaps (level 3, 2, 1) %s" % (r["max"], r["fp32_err"], r["tol"], r["swaps"]))
    assert r["tol"] > 0 and all(s > pc.SWAP_FACTOR * r["tol"] for s in r["swaps"]), r


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    wrong = {k: v for k, v in pc.einval_calls(L, ctypes.c_void_p(256)).items() if v != _lib.HF_EINVAL}
    assert not wrong, wrong
    # a pool of a single row or column has no output: nothing is launched
    assert L.hf_maxpool2x2_nhwc(1, 1, 4, 8, ctypes.c_void_p(256), 8, 0, ctypes.c_void_p(256), None) == _lib.HF_OK
