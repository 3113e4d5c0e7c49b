"""Kernel-level parity of the box codec, the projection gather and the fusion concat of csrc/glue.hip through the C ABI:
hf_bin_box_encode, hf_bin_box_decode, hf_bin_head_decode, hf_project_gather, hf_project_gather_grad, hf_fuse_concat and
hf_fuse_concat_grad at every launch regime, clamp and branch (the case table, the restated launch rule, the fp32 restatements of the
reference's text, their fp64 evaluation and the bounds are in tests/glue_cases.py), ctypes on _lib.lib() with no Python routing.

Every float input lies between NaN bands (a read outside it that reaches a result shows).  Every output is a slice of a sentinel-filled
buffer, pre-filled with NaN (integers: INT_FILL) and checked after the call: a write outside it, an element never written and a write
into a row that cls excludes show.  Integer outputs and every float output that does not pass through sinf / cosf are compared with
np.array_equal against the fp32 restatement (NaN for NaN); the x / z outputs of a case with a heading tensor lie within the derived
bound of the fp64 evaluation, with equal bins on every row.  A zero heading tensor gives the bits of the call without one.  Every call
but the atomic gradient is made twice and must give the same bits."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as gc  # noqa: E402
from abi_harness import INT_FILL, SENTINEL, Arena, Hold, IntOut, Out, abi, call, parity_report, twice, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
parity_report = parity_report("GLUE_PARITY_OUT", tuple(gc.ENTRY.values()))       # the source of profiles/glue_parity.md


def host(o, shape):
    return o.view.cpu().numpy().reshape(shape)


def exact(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    if got.dtype == np.int32:
        assert not (got == INT_FILL).any(), "%s: %d elements never written" % (name, int((got == INT_FILL).sum()))
        assert np.array_equal(got, want), "%s: %d of %d integers differ" % (name, int((got != want).sum()), got.size)
    else:
        assert np.array_equal(got, want, equal_nan=True), "%s: %d of %d floats differ from the fp32 restatement" % (
            name, int((~((got == want) | (np.isnan(got) & np.isnan(want)))).sum()), got.size)


def close(got, want64, bound, name, case):
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    within(t(got), t(want64), t(np.asarray(bound, np.float64)), name, gc.case_id(case))


# ------------------------------------------------------------------------------------------------- encode
def run_encode(c, t):
    _lib, L = abi()
    cst, rows, off = t["cst"], c["rows"], c["off"]
    k = cst["k"]
    a, I = Arena(DEV), Hold(DEV)
    ins = [I(t["ref_pts"], off), I(t["ref_theta"], off), I(t["boxes"], off), I(t["mean_sizes"], off), I(cst["ss"], off), I(cst["deltas"], off),
           I(cst["hi_xz"], off)]
    outs = dict(bin_x=IntOut(a, rows * k), res_x=Out(a, rows * k, off=off), bin_z=IntOut(a, rows * k), res_z=Out(a, rows * k, off=off), bin_t=IntOut(a, rows),
                res_t=Out(a, rows, off=off), res_y=Out(a, rows, off=off), res_size=Out(a, rows * 3, off=off))
    call(L.hf_bin_box_encode(rows, k, c["rcnn"], *ins, float(cst["r"]), float(cst["hi_theta"]), float(cst["delta_theta"]), float(cst["half_delta_theta"]),
                             *[outs[n].p for n in gc.ENCODE_OUT], _lib.stream_ptr()), "hf_bin_box_encode")
    a.check()
    shape = dict(bin_x=(rows, k), res_x=(rows, k), bin_z=(rows, k), res_z=(rows, k), bin_t=(rows,), res_t=(rows,), res_y=(rows,), res_size=(rows, 3))
    return {n: host(outs[n], shape[n]) for n in gc.ENCODE_OUT}


@pytest.mark.parametrize("c", gc.cases_of("encode"), ids=gc.case_id)
def test_bin_box_encode(c):
    t = gc.encode_inputs(c)
    cst = t["cst"]
    got = twice(run_encode, c, t)
    enc = lambda dt, heading: gc.encode(c["rcnn"], t["ref_pts"], t["ref_theta"] if heading else None, t["boxes"], t["mean_sizes"], cst, dt)
    trig = c["heading"] == "random"
    o32, t32 = enc(np.float32, c["heading"] != "zero")          # zero heading tensor: the bits of the call without one
    for n in ("bin_x", "bin_z", "bin_t"):
        nb = cst["nbt"] if n == "bin_t" else cst["nbx"]
        assert ((got[n] >= 0) & (got[n] < nb)).all(), "%s outside [0, %d): the loss kernels index with it" % (n, nb)
    for n in gc.ENCODE_OUT:
        if not (trig and n in ("res_x", "res_z")):
            exact(got[n], o32[n], "hf_bin_box_encode." + n)      # bins included: equal on every row
    if trig:
        o64, t64 = enc(np.float64, True)
        b = gc.encode_bounds(o64, t64, cst)
        ex = gc.exact_rows(t64)
        for n in ("res_x", "res_z"):
            close(got[n][~ex], o64[n][~ex], b[n][~ex], "hf_bin_box_encode." + n, c)
            exact(got[n][ex], o32[n][ex], "hf_bin_box_encode.%s (rows sent to a clamp)" % n)


# ------------------------------------------------------------------------------------------------- decode, head decode
def check_boxes(c, got, b32, b64, t64, name):
    """columns downstream of sinf / cosf by the bound, every other one bit for bit"""
    assert not np.isnan(got).any(), "%s: %d elements never written" % (name, int(np.isnan(got).sum()))
    if c["heading"] == "random":
        e = gc.decode_bounds(b64, t64)
        for col in gc.DECODE_TRIG:
            close(got[..., col], b64[..., col], e[..., col], "%s.boxes[%d]" % (name, col), c)
        keep = [1, 3, 4, 5, 6]
        exact(np.ascontiguousarray(got[..., keep]), np.ascontiguousarray(b32[..., keep]), name + ".boxes[1, 3:7]")
    else:
        exact(got, b32, name + ".boxes")


def run_decode(c, t):
    _lib, L = abi()
    cst, rows, off = t["cst"], c["rows"], c["off"]
    k = cst["k"]
    a, I = Arena(DEV), Hold(DEV)
    ins = [I(t["ref_pts"], off), I(t["ref_theta"], off)] + [I(t[n], off and t[n].dtype == np.float32) for n in gc.DECODE_ARGS] + \
          [I(cst["ss"], off), I(cst["deltas"], off)]
    boxes = Out(a, rows * k * 7, off=off)
    call(L.hf_bin_box_decode(rows, k, *ins, float(cst["r"]), float(cst["delta_theta"]), boxes.p, _lib.stream_ptr()), "hf_bin_box_decode")
    a.check()
    return dict(boxes=host(boxes, (rows, k, 7)))


@pytest.mark.parametrize("c", gc.cases_of("decode"), ids=gc.case_id)
def test_bin_box_decode(c):
    t = gc.decode_inputs(c)
    got = twice(run_decode, c, t)["boxes"]
    b32, _ = gc.decode_ref(t, heading=c["heading"] != "zero")
    b64, t64 = gc.decode_ref(t, np.float64)
    check_boxes(c, got, b32, b64, t64, "hf_bin_box_decode")


def run_head(c, t):
    _lib, L = abi()
    cst, rows, k, off = t["cst"], c["rows"], c["k"], c["off"]
    a, I = Arena(DEV), Hold(DEV)
    ins = [I(t["head"], off), I(t["ref_pts"], off), I(t["ref_theta"], off), I(t["mean_sizes_k"], off), I(cst["ss"], off), I(cst["deltas"], off)]
    boxes = Out(a, rows * 7 if c["cls"] else rows * k * 7, off=off)
    call(L.hf_bin_head_decode(rows, k, *c["bins"], *ins, float(cst["r"]), float(cst["delta_theta"]), I(t["cls"]), boxes.p, _lib.stream_ptr()), "hf_bin_head_decode")
    a.check()
    return dict(boxes=host(boxes, (rows, 7) if c["cls"] else (rows, k, 7)))


@pytest.mark.parametrize("c", gc.cases_of("head"), ids=gc.case_id)
def test_bin_head_decode(c):
    t = gc.head_inputs(c)
    got = twice(run_head, c, t)["boxes"]
    b32, _, _ = gc.head_ref(c, t, heading=c["heading"] != "zero")
    b64, t64, _ = gc.head_ref(c, t, np.float64)
    if not c["cls"]:
        check_boxes(c, got, b32, b64, t64, "hf_bin_head_decode")
        return
    # rows of a valid class hold exactly 7 floats, the others keep the NaN they were pre-filled with
    b32, valid = gc.gather_cls(b32, t["cls"])
    b64, _ = gc.gather_cls(b64, t["cls"])
    assert np.isnan(got[~valid]).all(), "a row whose cls lies outside [0, k) was written"
    assert not np.isnan(got[valid]).any(), "a row of a valid class was not written in full"
    pick = lambda v: np.take_along_axis(v, np.clip(t["cls"], 0, c["k"] - 1)[:, None], axis=1)[valid, 0]
    t64v = {n: (pick(v) if v.shape[1] > 1 else v[valid, 0]) for n, v in t64.items()}
    check_boxes(c, got[valid], b32[valid], b64[valid], t64v, "hf_bin_head_decode (cls)")


# ------------------------------------------------------------------------------------------------- projection
def run_gather(c, t):
    _lib, L = abi()
    b, p, h, w, ch = c["b"], c["p"], c["h"], c["w"], c["c"]
    a, I = Arena(DEV), Hold(DEV)
    out, pix = Out(a, b * p * ch, off=c["off"] == "out"), IntOut(a, b * p * 2, passed=c["pix"])
    call(L.hf_project_gather(b, p, h, w, ch, I(t["pts"]), I(t["calib"]), I(t["img"], c["off"] == "img"), out.p, pix.p, _lib.stream_ptr()), "hf_project_gather")
    a.check()
    return dict(out=host(out, (b, p, ch)), pix=host(pix, (b, p, 2)))


@pytest.mark.parametrize("c", gc.cases_of("gather"), ids=gc.case_id)
def test_project_gather(c):
    t = gc.gather_inputs(c)
    got = twice(run_gather, c, t)
    out, pix = gc.gather_ref(c, t)
    if c["pix"]:
        exact(got["pix"], pix, "hf_project_gather.pix")
    else:
        assert (got["pix"] == INT_FILL).all(), "pix == NULL: nothing is stored"
    assert not np.isnan(got["out"]).any(), "an element of out was never written"
    exact(got["out"], out, "hf_project_gather.out")


@pytest.mark.parametrize("c", gc.cases_of("gather_grad"), ids=gc.case_id)
def test_project_gather_grad(c):
    """integer-valued rows: every sum is exact in any order, so the atomic form equals the fp64 scatter bit for bit; pixels that receive
    nothing, and the whole image when p == 0, are exactly 0.0"""
    _lib, L = abi()
    t = gc.gather_grad_inputs(c)
    b, p, h, w, ch = c["b"], c["p"], c["h"], c["w"], c["c"]
    a, I = Arena(DEV), Hold(DEV)
    g = Out(a, b * h * w * ch, off=c["off"])
    go, px = (I(t["grad_out"], c["off"]), I(t["pix"])) if p else (None, None)
    call(L.hf_project_gather_grad(b, p, h, w, ch, go, px, g.p, _lib.stream_ptr()), "hf_project_gather_grad")
    a.check()
    got = host(g, (b, h, w, ch))
    want = gc.gather_grad(t["grad_out"], t["pix"], b, h, w, ch)
    assert not np.isnan(got).any(), "grad_img is not zero-filled everywhere"
    assert not got[:, h - 1].any() and not got[1, 0, 0].any()
    exact(got, want, "hf_project_gather_grad.grad_img")


# ------------------------------------------------------------------------------------------------- concat
def masks_of(c, I):
    m = gc.MASKS[c["masks"]]
    return m, (I(np.array(m, np.float32)) if m is not None else None)


def run_concat(c, t):
    _lib, L = abi()
    rows, c1, c2 = c["rows"], c["c1"], c["c2"]
    a, I = Arena(DEV), Hold(DEV)
    m, mp = masks_of(c, I)
    out = Out(a, rows * (c1 + c2), off=c["off"] == "out")
    call(L.hf_fuse_concat(rows, c1, c2, I(t["a"], c["off"] == "a"), I(t["b"], c["off"] == "b"), mp, out.p, _lib.stream_ptr()), "hf_fuse_concat")
    a.check()
    return dict(out=host(out, (rows, c1 + c2)))


@pytest.mark.parametrize("c", gc.cases_of("concat"), ids=gc.case_id)
def test_fuse_concat(c):
    t = gc.concat_inputs(c)
    got = twice(run_concat, c, t)["out"]
    exact(got, gc.concat(t["a"], t["b"], gc.MASKS[c["masks"]]), "hf_fuse_concat.out")


def run_concat_grad(c, t):
    _lib, L = abi()
    rows, c1, c2, null = c["rows"], c["c1"], c["c2"], c["null"]
    a, I = Arena(DEV), Hold(DEV)
    m, mp = masks_of(c, I)
    ga = Out(a, rows * c1, passed=null not in ("grad_a", "both"), off=c["off"] == "grad_a")
    gb = Out(a, rows * c2, passed=null not in ("grad_b", "both"), off=c["off"] == "grad_b")
    call(L.hf_fuse_concat_grad(rows, c1, c2, I(t["grad_out"], c["off"] == "grad_out"), mp, ga.p, gb.p, _lib.stream_ptr()), "hf_fuse_concat_grad")
    a.check()
    return dict(grad_a=host(ga, (rows, c1)), grad_b=host(gb, (rows, c2)))


@pytest.mark.parametrize("c", gc.cases_of("concat_grad"), ids=gc.case_id)
def test_fuse_concat_grad(c):
    t = gc.concat_inputs(c)
    got = twice(run_concat_grad, c, t)
    want = dict(zip(("grad_a", "grad_b"), gc.concat_grad(t["grad_out"], c["c1"], gc.MASKS[c["masks"]])))
    for n in ("grad_a", "grad_b"):
        if c["null"] in (n, "both"):
            assert (got[n] == SENTINEL).all(), "%s is NULL: its buffer keeps the sentinel" % n
        else:
            exact(got[n], want[n], "hf_fuse_concat_grad." + n)
    if c["null"] == "both":                 # nothing is read either: grad_out may be NULL
        _lib, L = abi()
        assert L.hf_fuse_concat_grad(c["rows"], c["c1"], c["c2"], None, None, None, None, _lib.stream_ptr()) == _lib.HF_OK


# ------------------------------------------------------------------------------------------------- argument checks
def test_argument_matrix_on_the_device():
    gc.check_arguments()
    torch.cuda.synchronize()


def test_a_refused_gradient_leaves_grad_img_alone():
    """a NULL grad_out or pix with points to scatter is refused before the zero-fill"""
    _lib, L = abi()
    a, I = Arena(DEV), Hold(DEV)
    g = Out(a, 2 * 3 * 5 * 4, fill=SENTINEL)
    go, px = I(np.ones((2, 7, 4), np.float32)), I(np.zeros((2, 7, 2), np.int32))
    assert L.hf_project_gather_grad(2, 7, 3, 5, 4, None, px, g.p, _lib.stream_ptr()) == _lib.HF_EINVAL
    assert L.hf_project_gather_grad(2, 7, 3, 5, 4, go, None, g.p, _lib.stream_ptr()) == _lib.HF_EINVAL
    a.untouched()


def render_parity(report):
    """profiles/glue_parity.md from the JSON that a session with GLUE_PARITY_OUT wrote"""
    lines = ["# Parity of the box codec of csrc/glue.hip with fp64 through the C ABI", "",
             "Worst `|got - ref64| / bound` of the outputs downstream of `sinf` / `cosf` (the x / z outputs of a call with a reference-heading",
             "tensor) over the cases of `tests/glue_cases.py`, one MI355X session of `GLUE_PARITY_OUT=report.json pytest -m gpu tests/test_glue_abi.py`;",
             "rendered by `python tests/test_glue_abi.py report.json`.  The bound is derived in `tests/glue_cases.py` (half an ulp per fp32 operation,",
             "`sinf` / `cosf` within 4 ulp, first order); it is not tuned from this file.  Every other output of the seven entry points (bins, theta,",
             "y, sizes, pixels, gathered rows, the integer-valued atomic gradient, the concat and its gradient) is compared bit for bit with the fp32",
             "restatement and does not appear.  Every ratio must be <= 1; those >= 0.5 are marked.", "",
             "## Worst ratio per entry point and output", "", "| output | worst ratio | |", "|---|---:|---|"]
    worst = {}
    for key, v in report.items():
        name = key.split("|")[0]
        worst[name] = max(worst.get(name, 0.0), v)
    for name, v in sorted(worst.items()):
        lines.append("| `%s` | %.3g | %s |" % (name, v, "**>= 0.5**" if v >= 0.5 else ""))
    lines += ["", "## Per case", "", "| output | case | worst ratio |", "|---|---|---:|"]
    for key, v in sorted(report.items()):
        name, case = key.split("|")
        lines.append("| `%s` | `%s` | %.3g |" % (name, case, v))
    lines += ["", "The decoders' ratios near 0.9 are the last rounding, not the trigonometry: `out = rx + ref` with `|ref|` up to 70 has a half ulp of",
              "`u |out|` when `|out|` lies just above a power of two.  The host's own fp32 evaluation (NumPy `sin` / `cos`, below 1 ulp) reaches",
              "0.65 to 0.91 on the same cases (`tests/test_glue_cases_cpu.py` prints it), and 0.18 to 0.33 on the encoder's residuals.", "",
              "## Mutations of `csrc/glue.hip` tried against the cases", "",
              "Each was built into a scratch library and run on the MI355X against the narrowest selection of `tests/test_glue_abi.py`; none is committed.", ""]
    lines += MUTATIONS
    return "\n".join(lines)


MUTATIONS = [
    "| mutation | failing test | first assertion |", "|---|---|---|",
    "| `vz = v + 2 * nbz` in the head decoder | `test_bin_head_decode`, bins 5x7x3 | 600 of 4200 floats differ |",
    "| the `hi_xz` clamp dropped from `xs` | `test_bin_box_encode`, dyadic family | `bin_x` outside [0, 12) |",
    "| `dtheta >= half_pi` in the fold | `test_bin_box_encode`, dyadic family, RCNN rank | 27 of 641 theta bins differ |",
    "| the RCNN rank's lower clamp `1e-3f` replaced by `0.0f` | `test_bin_box_encode`, dyadic family, RCNN rank | 160 of 641 `res_t` differ |",
    "| `row` of `project_gather_kernel` taken modulo the grid's span | `test_project_gather`, second-trip cases | elements never written |",
    "| `boxes + e * 7` under `cls` | `test_bin_head_decode`, the three-row case | write outside an output (it lands in the guard band) |",
    "| `vec4` without the pointer-alignment test | cross-compiled only, never run | `test_project_gather` with `off=img` / `off=out` is the case that would take it |",
    "", "`test_project_gather_against_oracle`, `test_bin_box_codec_against_oracle` and `test_bin_head_decode_against_oracle` of `tests/test_ops_gpu.py` pass on the",
    "first four (run); the fifth needs a second trip they never take; the sixth was not run against them (its write would leave their buffer).",
]


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        print(render_parity(json.load(f)))
