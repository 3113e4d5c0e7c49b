"""CPU checks of tests/image_pyramid_train_cases.py and of what the image pyramid's training route does without a GPU: the fp64
restatements against torch's own autograd, the adjoint identity of the stride-2 convolution, the pool rule against torch, the three
conditions that make the module-level tolerances meaningful, the HF_EINVAL paths of the five new entry points (they return before
any HIP call), the training scope and the flows' flag."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_pyramid_cases as pc  # noqa: E402
import image_pyramid_train_cases as tc  # noqa: E402

REL = 1e-12                  # fp64 against fp64 in another summation order, relative to the largest reference element


def _rand(*shape, seed=0):
    return torch.randn(*shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed))


def _close(got, want):
    return float((got - want).abs().max()) <= REL * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 5, 7, 3, 4), (1, 12, 22, 36, 40), (3, 1, 1, 5, 2), (1, 2, 9, 8, 3)])
def test_conv_gradients_are_torch_autograd(b, h, w, cin, cout):
    x, wt, sub, dz = _rand(b, h, w, cin), _rand(9, cout, cin, seed=1), _rand(cin, seed=2), _rand(b, h, w, cout, seed=3)
    for s in (None, sub):
        weight = wt.reshape(3, 3, cout, cin).permute(2, 3, 0, 1).contiguous().requires_grad_()
        xin = ((x if s is None else x - s).permute(0, 3, 1, 2)).contiguous().requires_grad_()
        F.conv2d(xin, weight, padding=1).backward(dz.permute(0, 3, 1, 2))
        dwt, S = tc.conv_wgrad_sum(x, dz, s)
        want = weight.grad.permute(2, 3, 0, 1).reshape(9, cout, cin)
        assert _close(dwt, want) and bool((S >= dwt.abs() - 1e-9).all())
        # the input gradient: the forward tap sum of dz with the flipped, transposed weights
        wd = wt.flip(0).transpose(1, 2).contiguous()
        dx, _ = pc.conv_tap_sum(dz, wd)
        assert _close(dx, xin.grad.permute(0, 2, 3, 1))
    if h == 1 and w == 1:      # one pixel: only the centre tap sees it
        dwt, _ = tc.conv_wgrad_sum(x, dz)
        assert all(bool((dwt[t] == 0).all()) for t in range(9) if t != 4) and bool((dwt[4] != 0).any())
    # and it is the autograd gradient of the project's own forward restatement
    xr = x.clone().requires_grad_()
    wr = wt.clone().requires_grad_()
    z, _ = pc.conv_tap_sum(xr, wr, sub)
    (z * dz).sum().backward()
    assert _close(tc.conv_wgrad_sum(x, dz, sub)[0], wr.grad) and _close(pc.conv_tap_sum(dz, wt.flip(0).transpose(1, 2).contiguous())[0], xr.grad)


@pytest.mark.parametrize("b,h,w,cin,cout", [(2, 3, 5, 6, 4), (1, 1, 1, 36, 8), (1, 4, 1, 3, 2)])
def test_upconv_gradients_are_torch_autograd(b, h, w, cin, cout):
    x, wt, dz = _rand(b, h, w, cin), _rand(9, cout, cin, seed=1), _rand(b, 2 * h, 2 * w, cout, seed=3)
    weight = wt.reshape(3, 3, cout, cin).permute(3, 2, 0, 1).contiguous().requires_grad_()
    xin = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    F.conv_transpose2d(xin, weight, stride=2, padding=1, output_padding=1).backward(dz.permute(0, 3, 1, 2))
    dwt, S = tc.upconv_wgrad_sum(x, dz)
    assert _close(dwt, weight.grad.permute(2, 3, 1, 0).reshape(9, cout, cin)) and bool((S >= dwt.abs() - 1e-9).all())
    # the input gradient: the stride-2 convolution of dz with w[t][ci][co] = wt[t][co][ci]
    dx, _ = tc.conv_s2_tap_sum(dz, wt.transpose(1, 2).contiguous())
    assert dx.shape == (b, h, w, cin) and _close(dx, xin.grad.permute(0, 2, 3, 1))


@pytest.mark.parametrize("name", list(tc.S2_CASES))
def test_stride2_reference_is_the_adjoint_of_the_upconvolution(name):
    """<conv_s2(g), x> = <g, upconv(x)> in fp64, with the existing upconv_tap_sum"""
    c, t = tc.S2_CASES[name], tc.s2_inputs(name)
    g, wt = torch.from_numpy(t["x"].astype(np.float64)), torch.from_numpy(t["wt"].astype(np.float64))
    x = _rand(c["b"], c["h"], c["w"], c["cout"], seed=7)
    lhs = float((tc.conv_s2_tap_sum(g, wt)[0] * x).sum())
    rhs = float((g * pc.upconv_tap_sum(x, wt.transpose(1, 2).contiguous())[0]).sum())
    scale = float((tc.conv_s2_tap_sum(g.abs(), wt.abs())[0] * x.abs()).sum())
    assert abs(lhs - rhs) <= REL * scale, (lhs, rhs)
    want = F.conv2d(g.permute(0, 3, 1, 2), wt.reshape(3, 3, c["cout"], c["cin"]).permute(2, 3, 0, 1), stride=2, padding=1).permute(0, 2, 3, 1)
    assert _close(tc.conv_s2_tap_sum(g, wt)[0], want)
    r = tc.s2_reference(name)
    assert r["y"].shape == (c["b"] * c["h"] * c["w"], c["cout"]) and bool((r["bound"] > 0).all())


def test_dgrad_reference_is_the_autograd_gradient_of_conv_tap_sum():
    for name in tc.DGRAD_CASES:
        c, t = pc.CONV_CASES[name], tc.dgrad_inputs(name)
        x = torch.zeros((c["b"], c["h"], c["w"], c["cin"]), dtype=torch.float64, requires_grad=True)
        z, _ = pc.conv_tap_sum(x, torch.from_numpy(t["wt"].astype(np.float64)))
        (z * torch.from_numpy(t["dz"].astype(np.float64))).sum().backward()
        r = tc.dgrad_reference(name)
        assert _close(r["dx"], x.grad.reshape(-1, c["cin"])) and bool((r["bound"] > 0).all())


@pytest.mark.parametrize("name", list(tc.POOL_BWD_CASES))
def test_pool_rule_is_torch(name):
    t, e = tc.pool_bwd_inputs(name), tc.pool_bwd_expected(name)
    mine = tc.pool_bwd_rule(t["x"], t["g"])
    assert np.array_equal(mine.view(np.uint32), e["grad"].view(np.uint32)), name
    c = tc.POOL_BWD_CASES[name]
    if c["h"] % 2:
        assert not e["grad"][:, -1].any() and not e["grad"][:, :, -1].any()
    x = t["x"]
    assert 0.3 < float((x == 0).mean()) < 0.7                                  # ReLU-like
    win = x[:, :c["h"] // 2 * 2, :c["w"] // 2 * 2].reshape(c["b"], c["h"] // 2, 2, c["w"] // 2, 2, c["c"])
    top = np.sort(np.nan_to_num(win.transpose(0, 1, 3, 5, 2, 4).reshape(-1, 4), nan=1e9), axis=1)
    assert ((top[:, 3] == top[:, 2]) & (top[:, 3] > 0)).any(), "no duplicated positive maximum in a window"
    assert ((top[:, 3] == 0)).any(), "no all-zero window"
    assert np.isnan(x).any() == (name == tc.POOL_NAN_CASE)


def test_case_tables_cover_what_the_kernels_branch_on():
    cases = tc.WGRAD_CASES
    assert len(cases) == 48 and {(c["b"], c["h"], c["w"]) for c in cases.values()} == set(tc.WGRAD_SHAPES)
    for key in ("cin", "cout"):
        for v in {c[key] for c in cases.values()}:
            assert {c["sub"] for c in cases.values() if c[key] == v} == {False, True}, (key, v)
    assert 2 * 5 * 7 < 256 < 12 * 22 < 512 and 40 * 52 > 4 * 256              # one chunk; two; several
    assert {(c["h"], c["w"]) for c in tc.UPWGRAD_CASES.values()} == {(3, 5), (1, 1), (12, 22)} and len(tc.UPWGRAD_CASES) == 12
    assert len(tc.S2_CASES) == 12 and all(c["slice"] for c in tc.S2_CASES.values())
    for key in ("cin", "cout"):
        for v in {c[key] for c in tc.S2_CASES.values()}:
            assert {c["affine"] for c in tc.S2_CASES.values() if c[key] == v} == {False, True}
    assert all(n in pc.CONV_CASES for n in tc.DGRAD_CASES)
    assert {c["c"] for c in tc.POOL_BWD_CASES.values()} == {3, 32, 40} and any(c["h"] % 2 and c["w"] % 2 for c in tc.POOL_BWD_CASES.values())
    r = tc.wgrad_reference("conv", "b3h1w1_ci36_co32")
    assert r["dwt"].shape == (9, 32, 36) and all(bool((r["dwt"][t] == 0).all()) for t in range(9) if t != 4)
    assert bool((r["bound"] > 0).all())


@pytest.mark.parametrize("name,text", tc.SOURCE_RULES, ids=lambda v: v[:40].replace(" ", "_"))
def test_rule_literals_are_those_of_the_sources(name, text):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "heterofusionrcnn_amd", "csrc", name)) as f:
        assert f.read().count(text) == 1, "the dispatch rule of %s changed: restate it in image_pyramid_train_cases.py (%r)" % (name, text)


def test_restated_wgrad_rules_agree_with_the_library():
    """the workspace query is the one piece of the plan the library shows without a GPU"""
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    for up, table in ((False, tc.EXACT_WGRAD_CASES), (True, tc.EXACT_UPWGRAD_CASES)):
        query = L.hf_upconv3x3s2_nhwc_wgrad_workspace if up else L.hf_conv3x3_nhwc_wgrad_workspace
        for name, c in table.items():
            assert query(c["b"], c["h"], c["w"], c["cin"], c["cout"]) == tc.conv_wgrad_plan(c)["workspace"], name
    c = dict(b=1, h=40, w=52, cin=65, cout=7)
    assert tc.wgrad_instantiation(c) == ("conv_wgrad_kernel", (2, False, False, False))
    assert tc.wgrad_instantiation(dict(c, cin=68, cout=8, up=True), "dz") == ("conv_wgrad_kernel", (2, False, True, True))
    p = tc.conv_wgrad_plan(c)
    assert p["forced"] and (p["mtiles"], p["ntiles"], p["wn"]) == (1, 1, 2) and p["rows_per_chunk"] == 256 and p["chunks"] == 9
    assert not tc.conv_wgrad_plan(dict(c, cout=8))["forced"] and tc.conv_wgrad_plan(dict(c, cout=128))["mtiles"] == 9


@pytest.mark.parametrize("up", (False, True), ids=("conv", "up"))
def test_exact_wgrad_family_is_exact_and_reaches_every_form(up):
    cases = tc.EXACT_UPWGRAD_CASES if up else tc.EXACT_WGRAD_CASES
    assert len(cases) == len(tc.EXACT_WGRAD_CIN) * len(tc.EXACT_WGRAD_COUT) + 4
    for name, c in cases.items():
        _, t, dwt, smax = tc.exact_wgrad_case(up, name)
        assert smax < 2 ** 24 and smax <= 10 * c["b"] * c["h"] * c["w"] and torch.equal(dwt, dwt.round()), name
        assert set(np.unique(t["dz"])) <= {-1.0, 0.0, 1.0} and float(np.abs(t["x"]).max()) <= 8 and np.array_equal(t["x"], np.round(t["x"]))
        if (c["h"], c["w"]) == (1, 1):
            live = (4, 5, 7, 8) if up else (4,)
            assert all(bool((dwt[k] == 0).all()) for k in range(9) if k not in live), name
    reach = {tc.wgrad_instantiation(c, c["off"])[1] for c in cases.values()}
    assert reach == {(wn, g, x, up) for wn in (1, 2) for g in (False, True) for x in (False, True)}
    plain = [c for c in cases.values() if c["off"] is None]
    for key, values in (("cin", tc.EXACT_WGRAD_CIN), ("cout", tc.EXACT_WGRAD_COUT)):
        for v in values:
            assert {(c["b"], c["h"], c["w"]) for c in plain if c[key] == v} == set(tc.WGRAD_SHAPES), (key, v)
    assert {c["cout"] for c in plain if tc.conv_wgrad_plan(c)["forced"]} == {1, 5, 7}
    assert {tc.conv_wgrad_plan(c)["chunks"] for c in plain} == {1, 2, 9}                  # 70 rows and one pixel; 264; 2080
    assert {c["sub"] for c in plain} == ({False} if up else {False, True})
    for wn in (1, 2):              # dz, then x, off the boundary where the shape alone would take both float4 paths
        moved = {c["off"]: tc.wgrad_instantiation(c, c["off"])[1] for c in cases.values() if c["off"] and (c["cin"] > 64) == (wn == 2)}
        assert moved == {"dz": (wn, False, True, up), "x": (wn, True, False, up)}


def test_exact_wgrad_references_are_torch_autograd():
    for up, name in ((False, "b1h12w22_ci36_co32_off_dz"), (False, "b2h5w7_ci3_co1"), (True, "b1h12w22_ci68_co128_off_x"), (True, "b2h5w7_ci3_co1")):
        c, t, dwt, _ = tc.exact_wgrad_case(up, name)
        x, dz = torch.from_numpy(t["x"]).double(), torch.from_numpy(t["dz"]).double()
        weight = torch.zeros((c["cin"], c["cout"], 3, 3) if up else (c["cout"], c["cin"], 3, 3), dtype=torch.float64, requires_grad=True)
        if up:
            out = F.conv_transpose2d(x.permute(0, 3, 1, 2), weight, stride=2, padding=1, output_padding=1)
            perm = (2, 3, 1, 0)
        else:
            xs = x if t["in_sub"] is None else x - torch.from_numpy(t["in_sub"]).double()
            out = F.conv2d(F.pad(xs.permute(0, 3, 1, 2), (1, 1, 1, 1)), weight)
            perm = (2, 3, 0, 1)
        out.backward(dz.permute(0, 3, 1, 2))
        assert torch.equal(weight.grad.permute(*perm).reshape(9, c["cout"], c["cin"]), dwt) and bool((dwt != 0).any()), name


def test_module_conditions_hold_for_the_seed():
    """the module-level tolerances (8 x the fp32 host route's own error, per tensor) must be above zero, must see a dropped skip or
    pooled path at every level, and must not be decided by a ReLU mask or an argmax that the fp32 rounding could flip"""
    r = tc.train_reference()
    layers = sum(n for n, _ in pc.MODEL_CONV) + 6         # the small model: eleven layers, where the shipped widths have sixteen
    assert len([k for k in r["tol"] if k.startswith("grad.")]) == 3 * layers and len([k for k in r["tol"] if k.startswith("buf.")]) == 2 * layers
    print("tolerances: out %.3g, gradients %.3g .. %.3g, running statistics %.3g .. %.3g" % (
        r["tol"]["out"], min(v for k, v in r["tol"].items() if k.startswith("grad.")), max(v for k, v in r["tol"].items() if k.startswith("grad.")),
        min(v for k, v in r["tol"].items() if k.startswith("buf.")), max(v for k, v in r["tol"].items() if k.startswith("buf."))))
    print("detached paths move a gradient by (tolerances): %s" % {k: "%.3g" % v for k, v in r["moves"].items()})
    print("smallest |pre-ReLU activation| / tolerance %.3g, smallest pool gap / tolerance %.3g" % (r["relu_margin"], r["pool_margin"]))
    cond = tc.train_conditions(r)
    assert all(cond.values()), cond
    assert tc.find_seed() == tc.TRAIN_SEED, "TRAIN_SEED is not the first seed that satisfies the conditions"
    assert set(r["tracked"].values()) == {1}


def test_train_scope():
    from heterofusionrcnn_amd import image_pyramid
    assert image_pyramid.TRAIN_BRANCHES == ("torch", "native") and image_pyramid.train_branch_name() == "torch"
    assert image_pyramid.IMAGE_BRANCHES == ("torch", "native")
    with image_pyramid.train_branch("native"):
        assert image_pyramid.train_branch_name() == "native" and image_pyramid.image_branch_name() == "torch"
        with image_pyramid.train_branch("torch"):
            assert image_pyramid.train_branch_name() == "torch"
        assert image_pyramid.train_branch_name() == "native"
    assert image_pyramid.train_branch_name() == "torch"
    with pytest.raises(ValueError, match="image train branch"):
        image_pyramid.train_branch("miopen")


def test_host_tensors_keep_the_torch_route_under_the_train_scope():
    from heterofusionrcnn_amd import image_pyramid
    image, cot = pc.make_image(tc.TRAIN_SEED), tc.make_cotangent()
    calls = image_pyramid.NATIVE_TRAIN_CALLS[0]
    want = tc._step(tc.make_train_model(), image, cot)
    with image_pyramid.train_branch("native"):
        got = tc._step(tc.make_train_model(), image, cot)
    assert image_pyramid.NATIVE_TRAIN_CALLS[0] == calls
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    with pytest.raises(RuntimeError, match="no CPU implementation"):
        image_pyramid.forward_train(tc.make_train_model(), image)


def test_layer_order_restates_the_package():
    from heterofusionrcnn_amd import image_pyramid
    net = tc.make_train_model()
    recs = image_pyramid._train_layers(net)
    assert [r["seq"] for r in recs] == [s for _, s in tc.layer_sequences(net)] and len(recs) == 5 + 6
    assert [r["dst"] for r in recs if r["dst"][0] == "cat"] == [("cat", 0, 0), ("cat", 1, 0), ("cat", 2, 0), ("cat", 2, 1), ("cat", 1, 1), ("cat", 0, 1)]


def test_flows_take_the_image_train_branch_flag():
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    for mod, args in ((train_rpn, ["d"]), (train_rcnn, ["d", "h"])):
        assert inspect.signature(mod.train).parameters["image_train_branch"].default == "torch"
        assert mod.build_parser().parse_args(args).image_train_branch == "torch"
        assert mod.build_parser().parse_args(args + ["--image-train-branch", "native"]).image_train_branch == "native"
        with pytest.raises(SystemExit):
            mod.build_parser().parse_args(args + ["--image-train-branch", "miopen"])


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    wrong = {k: v for k, v in tc.einval_calls(L, ctypes.c_void_p(256)).items() if v != _lib.HF_EINVAL}
    assert not wrong, wrong
    nonzero = {k: v for k, v in tc.workspace_queries(L).items() if v != 0}
    assert not nonzero, nonzero
    # 1 x 20 x 20 pixels are two chunks of the (9 cout, cin) matrix
    assert L.hf_conv3x3_nhwc_wgrad_workspace(1, 20, 20, 8, 32) == L.hf_upconv3x3s2_nhwc_wgrad_workspace(1, 20, 20, 8, 32) == 2 * 9 * 32 * 8 * 4
    # an accumulating pool gradient without a whole window has nothing to add
    assert L.hf_maxpool2x2_nhwc_bwd(1, 1, 4, 8, ctypes.c_void_p(256), 8, 0, None, ctypes.c_void_p(256), 8, 0, 1, None) == _lib.HF_OK
