"""tests/glue_cases.py checked on any machine: the restated constants against the text of glue.hip, every case's declared regime against
the restated launch rule, the branch accounting of the encode families, the fp32 restatements against their fp64 evaluation and against
the CPU oracle, the host's own fp32 trigonometry inside the derived bound, the redraw of undecided rows, and the argument checks of the
seven entry points before any launch (those of hf_project_gather_grad_ordered are in tests/test_ordered_grad_cases_cpu.py)."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heterofusionrcnn_amd", "csrc")
CASES = gc.all_cases()
SMALL = lambda op: [c for c in gc.cases_of(op) if c.get("rows", 0) <= 5000 and c.get("p", 0) <= 5000]
U = gc.U


def test_case_ids_are_unique_and_counted():
    ids = [gc.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    assert len(ids) == 104, "a case was added or removed: update this number when you add a case"


# ------------------------------------------------------------------------------------------------- the restated facts
def test_source_constants_against_the_text_of_the_kernels():
    text = {}
    for name, pattern, value, count in gc.SOURCE_CONSTANTS:
        if name not in text:
            with open(os.path.join(CSRC, name)) as f:
                text[name] = f.read()
        found = re.findall(pattern, text[name])
        assert len(found) == count, (pattern, found)
        assert all(float(v) == float(value) for v in found), (pattern, found)
    assert gc.GRID_CAP == 4096 and gc.STRIDE == 1048576
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "-ffp-contract=off" in f.read()


def test_launch_rule():
    assert [gc.grid(n) for n in (0, 1, 256, 257, gc.STRIDE, gc.STRIDE + 1, 10 ** 9)] == [1, 1, 1, 2, 4096, 4096, 4096]
    assert [gc.trips(n) for n in (1, 257, gc.STRIDE, gc.STRIDE + 1, 2 * gc.STRIDE, 2 * gc.STRIDE + 1)] == [1, 1, 1, 2, 2, 3]
    assert gc.gather_vec(4) == 4 and gc.gather_vec(32) == 4 and gc.gather_vec(3) == 1 and gc.gather_vec(4, True) == 1 and gc.gather_vec(8, False, True) == 1
    assert gc.concat_vec(4, 4) == 4 and gc.concat_vec(256, 32, False, False, False) == 4 and gc.concat_vec(4, 3) == 1 and gc.concat_vec(3, 4) == 1
    assert gc.concat_vec(4, 4, False, True, False) == 1


def test_every_case_declares_the_regime_the_rule_gives_it():
    for c in CASES:
        assert gc.regime(c) == c["expect"], gc.case_id(c)


def test_every_kernel_vec_and_trip_count_has_a_case():
    seen = {gc.regime(c) for c in CASES} - {None}
    want = set()
    for kernel in gc.KERNELS:
        vecs = (1, 4) if kernel in ("project_gather_kernel", "fuse_concat_kernel", "fuse_concat_grad_kernel") else (0,)
        want |= {(kernel, v, t) for v in vecs for t in (1, 2)}
    assert seen == want, sorted(seen ^ want)
    assert any(c["expect"] is None for c in gc.cases_of("gather_grad")) and any(c["expect"] is None for c in gc.cases_of("concat_grad"))
    # the scalar fallback is reached through a misaligned pointer at a vec4-eligible shape, each pointer in turn
    assert {c["off"] for c in gc.cases_of("gather") if c["c"] % 4 == 0 and c["off"]} == {"img", "out"}
    assert {c["off"] for c in gc.cases_of("concat") if c["off"]} == {"a", "b", "out"}
    assert {c["off"] for c in gc.cases_of("concat_grad") if c["off"] and not c["null"]} == {"grad_out", "grad_a", "grad_b"}
    assert {c["null"] for c in gc.cases_of("concat_grad")} == {None, "grad_a", "grad_b", "both"}
    assert {(c["c1"], c["c2"]) for c in gc.cases_of("concat")} >= set(gc.CONCAT_SHAPES) and {c["masks"] for c in gc.cases_of("concat")} == set(gc.MASKS)
    assert {c["c"] for c in gc.cases_of("gather")} == set(gc.GATHER_CHANNELS) and not all(c["pix"] for c in gc.cases_of("gather"))
    assert {c["bins"] for c in gc.cases_of("head")} == set(gc.HEAD_BINS) and {gc.n_classes(c) for c in gc.cases_of("decode") + gc.cases_of("head")} == {1, 2, 3}
    for bins in gc.HEAD_BINS:
        assert {c["cls"] for c in gc.cases_of("head") if c["bins"] == bins} == {False, True}


def test_parameter_sets_are_those_of_the_package():
    from heterofusionrcnn_amd import rcnn, rpn
    a = rpn.rpn_multiclass_heads(rpn.rpn_stack_config2())
    p = gc.PARAMS["rpn_config"]
    assert (p["ss"], p["deltas"], p["r"], p["delta_theta"], p["nbt"]) == (a.xz_search_range, a.xz_bin_len, a.r_theta, a.delta_theta, a.theta_bin_num)
    r = rcnn.RcnnConfig()
    p = gc.PARAMS["rcnn"]
    assert (p["ss"], p["deltas"], p["r"], p["delta_theta"], p["nbt"]) == (r.xz_search_range, r.xz_bin_len, r.r_theta, r.delta_theta, r.num_bin_theta)
    assert gc.consts("rcnn")["nbx"] == r.num_bin_xz == 6 and gc.consts("rpn")["nbx"] == a.num_bin_xz == 12 and gc.consts("k1")["k"] == 1
    for name in gc.PARAMS:                  # the largest bin is nb - 1 at the upper clamp
        c = gc.consts(name)
        assert (np.floor(c["hi_xz"] / c["deltas"]) == c["nbx"] - 1).all() and np.floor(c["hi_theta"] / c["delta_theta"]) == c["nbt"] - 1


# ------------------------------------------------------------------------------------------------- encode
@pytest.fixture(scope="module")
def encode_data():
    return {gc.case_id(c): gc.encode_inputs(c) for c in SMALL("encode")}


def enc(c, t, dt=np.float32, heading=True):
    return gc.encode(c["rcnn"], t["ref_pts"], t["ref_theta"] if heading else None, t["boxes"], t["mean_sizes"], t["cst"], dt)


@pytest.mark.parametrize("c", SMALL("encode"), ids=gc.case_id)
def test_encode_case_reaches_what_it_declares(c, encode_data):
    t = encode_data[gc.case_id(c)]
    n = gc.accounting(c, t)
    print(n)
    assert n["bins_in_range"], "a bin outside [0, nb)"
    for key in gc.ENCODE_REACHES[c["family"]][c["rcnn"]]:
        assert n[key] > 0, (key, n)
    if c["family"] == "dyadic":
        assert n["x_edges"] == n["z_edges"] == t["cst"]["nbx"] - 1, "every interior bin edge of every class, exactly"
        if c["rcnn"]:
            assert n["t_below"] > 0 and n["t_above"] > 0      # the lower clamp 1e-3 and the upper one
    if c["family"] == "background":
        assert not t["boxes"].any() and n["x_interior"] + n["z_interior"] < 0.2 * 2 * c["rows"] * t["cst"]["k"]
    if c["family"] == "random" and c["rcnn"] and c["heading"] == "random":
        assert n["th0_negative"] > 0 and n["th0_past_2pi"] > 0
    if c["family"] == "nonfinite":
        bad = ~np.isfinite(np.concatenate([t["boxes"], t["ref_pts"]], axis=1)).all(axis=1)
        assert bad.sum() >= 30


@pytest.mark.parametrize("c", SMALL("encode"), ids=gc.case_id)
def test_encode_restatement_against_fp64_and_the_host_trig_inside_the_bound(c, encode_data):
    t = encode_data[gc.case_id(c)]
    o32, t32 = enc(c, t)
    o64, t64 = enc(c, t, np.float64)
    assert all(o32[n].dtype == (np.int32 if n.startswith("bin") else np.float32) for n in gc.ENCODE_OUT)
    if c["heading"] == "zero":              # sin(0) = 0 and cos(0) = 1: the rotation branch changes no bit
        o_none, _ = enc(c, t, heading=False)
        for n in gc.ENCODE_OUT:
            assert np.array_equal(o32[n], o_none[n], equal_nan=True), n
    if c["heading"] == "random":
        b = gc.encode_bounds(o64, t64, t["cst"])
        ex = gc.exact_rows(t64)
        assert np.array_equal(ex, gc.exact_rows(t32))
        assert not (gc.undecided_bins(o64, t64, t["cst"]) & ~ex).any(), "a row the redraw left undecided"
        for a in ("x", "z"):
            assert np.array_equal(o32["bin_" + a], o64["bin_" + a]), "bins differ between the host fp32 and the fp64 evaluation"
            ratio = np.abs(o32["res_" + a].astype(np.float64) - o64["res_" + a])[~ex] / b["res_" + a][~ex]
            print("res_%s: host fp32 trig, worst |fp32 - fp64| / bound = %.3g" % (a, ratio.max()))
            assert ratio.max() <= 1.0
            assert np.array_equal(o32["res_" + a][ex], o64["res_" + a][ex].astype(np.float32), equal_nan=True)
        print("redrawn rows: %d of %d" % (t["redraws"], c["rows"]))
        assert t["ref_pts"].shape[0] == c["rows"] and t["redraws"] < c["rows"] // 10
    # everything that does not pass through trig: the fp32 value is the fp64 one within a few roundings wherever the bins agree
    with np.errstate(invalid="ignore"):
        agree = (o32["bin_t"] == o64["bin_t"]) & np.isfinite(o64["res_t"]) & np.isfinite(t64["pre_t"])
        if c["rcnn"]:                       # a fold decided the other way moves the bin too: those rows are in `agree` already
            agree &= np.abs(t32["d0"] - t64["d0"]) < 1e-3
        assert agree.mean() > 0.8
        err = np.abs(o32["res_t"].astype(np.float64) - o64["res_t"])[agree]
        assert (err <= 64 * U * (np.abs(t64["pre_t"][agree]) + 8.0) / float(t["cst"]["half_delta_theta"])).all()
        fin = np.isfinite(o64["res_size"])
        assert (np.abs(o32["res_size"].astype(np.float64) - o64["res_size"])[fin] <= 4 * U * (np.abs(o64["res_size"][fin]) + 1)).all()
        if c["heading"] == "none":
            for a in ("x", "z"):
                ok = (o32["bin_" + a] == o64["bin_" + a]) & np.isfinite(o64["res_" + a]) & np.isfinite(t64["t" + a])
                assert ok.mean() > (0.9 if c["family"] == "nonfinite" else 0.95)
                err = np.abs(o32["res_" + a].astype(np.float64) - o64["res_" + a])
                lim = 4 * U * (np.abs(t64["t" + a]) + 8.0) / t["cst"]["deltas"].astype(np.float64)
                assert (err[ok] <= np.broadcast_to(lim, err.shape)[ok]).all()


def test_the_redraw_condition_sees_a_row_on_a_bin_edge(encode_data):
    """a row planted so that its rotated offset lies a few 1e-8 from an interior bin edge is reported as undecided (the seeded cases
    happen to need few redraws or none); a row deep inside a clamp or a bin is not; the generator keeps the row count either way"""
    c = next(c for c in SMALL("encode") if c["family"] == "random" and c["heading"] == "random" and c["params"] == "rpn")
    t = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in encode_data[gc.case_id(c)].items()}
    cst = t["cst"]
    th = np.float64(t["ref_theta"][0])
    # (x, z) offsets after the rotation by -th: x on the edge 2 of class 0; x inside a bin and z = 0 (0 + Ss is the edge nb / 2); both deep
    for i, (tx, tz) in enumerate(((1.0 - 3.0, 0.1), (0.3 - 3.0, 0.0), (-9.0, 0.1))):
        dx, dz = np.cos(th) * tx + np.sin(th) * tz, -np.sin(th) * tx + np.cos(th) * tz
        t["ref_theta"][i] = t["ref_theta"][0]
        t["ref_pts"][i] = (1.0, 0.5, 2.0)
        t["boxes"][i, 0], t["boxes"][i, 2] = np.float32(1.0 + dx), np.float32(2.0 + dz)
    o64, t64 = enc(c, t, np.float64)
    assert abs(t64["rx"][0] + 2.0) < 1e-6 and abs(t64["rx"][1] + 2.7) < 1e-6 and abs(t64["rz"][1]) < 1e-6 and t64["rx"][2] < -8.9
    bad = gc.undecided_bins(o64, t64, cst)
    assert bad[0] and bad[1] and not bad[2]


@pytest.mark.parametrize("c", SMALL("encode"), ids=gc.case_id)
def test_encode_restatement_against_the_cpu_oracle(c, encode_data, oracle_mod):
    """no heading tensor: bit for bit (bins, residuals, NaN for NaN).  With one the oracle's libm sinf / cosf stand in for the device's:
    its bins equal the restatement's and its residuals lie inside the bound of the fp64 evaluation"""
    t = encode_data[gc.case_id(c)]
    p = gc.PARAMS[c["params"]]
    got = oracle_mod.bin_box_encode(t["ref_pts"], t["ref_theta"], t["boxes"], t["mean_sizes"], p["ss"], p["deltas"], p["r"], p["delta_theta"], t["cst"]["k"],
                                    c["rcnn"])
    o32, t32 = enc(c, t)
    trig = c["heading"] == "random"
    for n, g in zip(gc.ENCODE_OUT, got):
        if trig and n in ("res_x", "res_z"):
            o64, t64 = enc(c, t, np.float64)
            ex = gc.exact_rows(t64)
            b = gc.encode_bounds(o64, t64, t["cst"])[n]
            assert (np.abs(g.astype(np.float64) - o64[n])[~ex] <= b[~ex]).all(), n
            assert np.array_equal(g[ex], o32[n][ex], equal_nan=True), n
        else:
            assert np.array_equal(g, o32[n], equal_nan=True), (n, int((g != o32[n]).sum()))


# ------------------------------------------------------------------------------------------------- decode, head decode
def check_decode_pair(c, t, b32, t32, b64, t64):
    assert b32.dtype == np.float32
    if c["heading"] == "random":
        e = gc.decode_bounds(b64, t64)
        for col in gc.DECODE_TRIG:
            ratio = np.abs(b32[..., col].astype(np.float64) - b64[..., col]) / e[..., col]
            print("column %d: host fp32 trig, worst |fp32 - fp64| / bound = %.3g" % (col, ratio.max()))
            assert ratio.max() <= 1.0
    cols = [1, 3, 4, 5, 6] + ([] if c["heading"] == "random" else [0, 2])
    err = np.abs(b32.astype(np.float64) - b64)[..., cols]
    assert (err <= 6 * U * (np.abs(b64[..., cols]) + 48.0)).all()


@pytest.mark.parametrize("c", SMALL("decode"), ids=gc.case_id)
def test_decode_restatement(c, oracle_mod):
    t = gc.decode_inputs(c)
    cst = t["cst"]
    assert (t["bin_x"] == 0).any() and (t["bin_x"] == cst["nbx"] - 1).any() and (t["bin_t"] == cst["nbt"] - 1).any()
    for n in ("res_x", "res_z", "res_t"):
        assert all((t[n] == v).any() for v in (0.5, -0.5, 0.75, -0.75))
    b32, t32 = gc.decode_ref(t)
    b64, t64 = gc.decode_ref(t, np.float64)
    check_decode_pair(c, t, b32, t32, b64, t64)
    if c["heading"] == "zero":
        assert np.array_equal(b32, gc.decode_ref(t, heading=False)[0])
    p = gc.PARAMS[c["params"]]
    got = oracle_mod.bin_box_decode(t["ref_pts"], t["ref_theta"], *[t[n] for n in gc.DECODE_ARGS], p["ss"], p["deltas"], p["r"], p["delta_theta"])
    if c["heading"] == "random":
        e = gc.decode_bounds(b64, t64)
        assert (np.abs(got.astype(np.float64) - b64)[..., gc.DECODE_TRIG] <= e[..., gc.DECODE_TRIG]).all()
        keep = [1, 3, 4, 5, 6]
        assert np.array_equal(got[..., keep], b32[..., keep])
    else:
        assert np.array_equal(got, b32)


@pytest.mark.parametrize("c", SMALL("head"), ids=gc.case_id)
def test_head_decode_restatement(c, oracle_mod):
    t = gc.head_inputs(c)
    b32, t32, bins = gc.head_ref(c, t)
    b64, t64, bins64 = gc.head_ref(c, t, np.float64)
    assert np.isfinite(t["head"]).all() and t["head"].shape[-1] == gc.head_width(*c["bins"])
    for s, (b, nb) in enumerate(zip(bins, c["bins"])):
        assert np.array_equal(b, bins64[s]) and b.min() >= 0 and b.max() <= nb - 1
        planted = t["planted"][s]
        m = planted >= 0
        assert np.array_equal(b[m], np.broadcast_to(planted[:, None], b.shape)[m]), "a tie must go to the first maximum, a strict maximum in the last position to it"
        if nb > 2:
            assert set(planted[m].tolist()) == {0, (nb - 1) // 2, nb - 1}
    check_decode_pair(c, t, b32, t32, b64, t64)
    if c["heading"] == "zero":
        assert np.array_equal(b32, gc.head_ref(c, t, heading=False)[0])
    if c["cls"]:
        k = c["k"]
        if c["rows"] >= 50:                  # the three-row case keeps its last row valid: a row written at e 7 would land in the guard band
            assert (t["cls"] == -1).any() and (t["cls"] == k).any() and all((t["cls"] == j).any() for j in range(k))
        picked, valid = gc.gather_cls(b32, t["cls"])
        assert valid[-1] and np.isnan(picked[~valid]).all() and not np.isnan(picked[valid]).any()
    p = gc.PARAMS[c["params"]]
    got = oracle_mod.bin_head_decode(t["head"], t["ref_pts"], t["ref_theta"], t["mean_sizes_k"], *c["bins"], p["ss"], p["deltas"], p["r"], p["delta_theta"])
    if c["heading"] == "random":
        e = gc.decode_bounds(b64, t64)
        assert (np.abs(got.astype(np.float64) - b64)[..., gc.DECODE_TRIG] <= e[..., gc.DECODE_TRIG]).all()
        keep = [1, 3, 4, 5, 6]
        assert np.array_equal(got[..., keep], b32[..., keep])
    else:
        assert np.array_equal(got, b32)


# ------------------------------------------------------------------------------------------------- projection, concat
@pytest.mark.parametrize("c", SMALL("gather"), ids=gc.case_id)
def test_projection_restatement(c, oracle_mod):
    t = gc.gather_inputs(c)
    b, p, h, w = c["b"], c["p"], c["h"], c["w"]
    out, pix = gc.gather_ref(c, t)
    ok = gc.inside(pix, h, w)
    assert not out[~ok].any() and 0.2 < ok.mean() < 0.98
    _, uf, vf = gc.project(t["pts"], t["calib"])
    _, u64, v64 = gc.project(t["pts"], t["calib"], np.float64)
    if c["family"] == "exact":
        sp = gc.special_pixels(h, w)
        for i in range(b):
            for n, (u, v, d, _) in enumerate(sp):
                assert uf[i, n] == u and vf[i, n] == v, "the exact family's quotients are exact"
                big = max(abs(u), abs(v)) >= 2.0 ** 31
                want_in = not big and 0 <= int(u) < w and 0 <= int(v) < h           # int() truncates toward zero: -0.5 is column 0
                assert bool(ok[i, n]) == want_in, (u, v)
                assert tuple(pix[i, n]) == ((-1, -1) if big else (int(u), int(v)))
            n = len(sp)
            assert uf[i, n] == np.inf and np.isnan(uf[i, n + 1]) and uf[i, n + 7] == -np.inf
            assert uf[i, n + 2] == np.inf, "a depth of -0.0 does not survive the sum with the row's zero terms: -0.0 + 0.0 = +0.0"
            assert tuple(pix[i, n + 3]) == (2, 1) and ok[i, n + 3], "a point behind the camera still has a pixel"
            assert (pix[i, [n, n + 1, n + 2, n + 4, n + 5, n + 6, n + 7]] == -1).all()
        assert np.array_equal(uf, u64.astype(np.float32), equal_nan=True)
    else:
        P, x = t["calib"].astype(np.float64)[:, None, :], t["pts"].astype(np.float64)
        mag = np.abs(P[..., 0] * x[..., 0]) + np.abs(P[..., 2] * x[..., 2]) + np.abs(P[..., 3])
        d = x[..., 2] + P[..., 11]
        assert (np.abs(uf - u64) <= 4 * U * mag / np.abs(d) + 4 * U * np.abs(u64)).all()
        assert (pix == np.trunc(np.stack([u64, v64], -1)))[np.abs(np.stack([u64, v64], -1) - np.rint(np.stack([u64, v64], -1))).min(-1) > 1e-3].all()
    o_out, o_pix = oracle_mod.project_gather(t["pts"], t["calib"].reshape(b, 3, 4), t["img"])
    assert np.array_equal(o_pix, pix) and np.array_equal(o_out, out)
    if b == 2:                              # a wrong frame index shows: the two frames disagree on most points
        other = gc.gather(t["img"][::-1], pix)
        assert (other != out)[ok].mean() > 0.9


@pytest.mark.parametrize("c", SMALL("gather_grad"), ids=gc.case_id)
def test_gradient_scatter_reference(c, oracle_mod):
    t = gc.gather_grad_inputs(c)
    b, p, h, w, ch = c["b"], c["p"], c["h"], c["w"], c["c"]
    g = gc.gather_grad(t["grad_out"], t["pix"], b, h, w, ch)
    assert g.shape == (b, h, w, ch) and not g[:, h - 1].any() and not g[1, 0, 0].any()
    if p:
        assert np.array_equal(g, np.rint(g)) and gc.inside(t["pix"], h, w).sum() > 5 * b * (h - 1) * w, "integer sums of many points per pixel"
        assert not gc.inside(t["pix"], h, w).all()
        assert np.array_equal(oracle_mod.project_gather_grad((b, h, w, ch), t["pix"], t["grad_out"]), g)
    else:
        assert not g.any()


def test_concat_reference():
    a, b = np.arange(6, dtype=np.float32).reshape(2, 3), -np.arange(4, dtype=np.float32).reshape(2, 2)
    assert gc.concat(a, b, None).tolist() == [[0, 1, 2, 0, -1], [3, 4, 5, -2, -3]]
    assert gc.concat(a, b, (0.5, 2.0)).tolist() == [[0, 0.5, 1, 0, -2], [1.5, 2, 2.5, -4, -6]]
    ga, gb = gc.concat_grad(gc.concat(a, b, None), 3, (1.0, 0.0))
    assert np.array_equal(ga, a) and not gb.any() and gb.shape == (2, 2)


# ------------------------------------------------------------------------------------------------- argument checks, no launch
def test_argument_matrix_before_any_launch():
    gc.check_arguments()
