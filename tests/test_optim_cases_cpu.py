"""tests/optim_cases.py checked on any machine: the restated rules against the text of optim.hip, the fp64 reference against
torch.optim.Adam (fp64, CPU) and against a restatement of TensorFlow's clip_by_norm + AdamOptimizer + exponential_decay, optim.lr_at against
the reference's learning rate, the fp32 floor of the staircase at every global step of the reference's schedule, the NumPy-fp32
restatement of the kernels inside the bound on every case, six planted errors outside it, the exact family exact, every regime of the
three kernels reached, and the argument checks of hf_adam_multi and hf_copy_multi before any launch."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402
from abi_harness import same_bits  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heterofusionrcnn_amd", "csrc")
CASES = oc.all_cases()
_INPUTS = {}


def data(c):
    if c["name"] not in _INPUTS:
        _INPUTS[c["name"]] = oc.inputs(c)
    return _INPUTS[c["name"]]


def test_case_ids_are_unique_and_the_list_stays_small():
    ids = [oc.case_id(c) for c in CASES] + [c["name"] for c in oc.COPY_CASES]
    assert len(ids) == len(set(ids))
    assert len(CASES) == 113 and len(oc.COPY_CASES) == 41, "a case was added or removed: update these numbers when you add a case"
    assert sum(oc.elements(c) for c in CASES) <= 310000
    assert max(oc.elements(c) for c in CASES) * 4 * 4 <= 4 << 20                      # p, g, m, v of the largest case: a few MB
    assert sum(max(b, 0) for c in oc.COPY_CASES for b, _, _ in c["entries"]) <= 2 << 20


def test_restated_rules_stand_in_the_source():
    with open(os.path.join(CSRC, "optim.hip")) as f:
        text = f.read()
    for rule in oc.SOURCE_RULES:
        assert rule in text, rule
    with open(os.path.join(CSRC, "Makefile")) as f:
        make = f.read()
    assert "-ffp-contract=off" in make and "fast-math" not in make and "-Ofast" not in make


# ------------------------------------------------------------------------------------------------- the reference
def test_reference_is_torch_adam_in_fp64_for_mode_1():
    picked = [c for c in CASES if c["mode"] == 1 and c["clip"] == 0 and c["sched"] == oc.SCHED_CONST]
    assert {c["family"] for c in picked} == {"instantiations", "exact"}
    for c in picked:
        d, ref = data(c), oc.reference(c, data(c))
        for k, i in enumerate(oc.live(c)):
            p = torch.from_numpy(d["p"][i].astype(np.float64)).requires_grad_(True)
            opt = torch.optim.Adam([p], lr=c["lr"], betas=(c["b1"], c["b2"]), eps=c["eps"])
            opt.state[p] = {"step": torch.tensor(float(c["t"] - 1)), "exp_avg": torch.from_numpy(d["m"][i].astype(np.float64)),
                            "exp_avg_sq": torch.from_numpy(d["v"][i].astype(np.float64))}
            p.grad = torch.from_numpy(d["g"][i].astype(np.float64) * c["scale"])
            opt.step()
            st = opt.state[p]
            assert float(st["step"]) == c["t"]
            for name, got in (("p", p.detach()), ("m", st["exp_avg"]), ("v", st["exp_avg_sq"])):
                np.testing.assert_allclose(ref[k][name][0], got.numpy(), rtol=1e-12, atol=1e-300, err_msg="%s of %s" % (name, c["name"]))


def _tf_step(p, g, m, v, t, lr, b1, b2, eps, scale, clip, decay):
    """one step of tests/test_train_op.py's _tf_reference from given moments, fp64: x = grad_scale g; tf.clip_by_norm(x, clip) per
    tensor; tf.train.AdamOptimizer with lr = exponential_decay(lr, t - 1, *decay) (staircase)"""
    lr_t = lr if decay is None else lr * decay[1] ** np.floor((t - 1) / decay[0])
    x = g * scale
    if clip is not None:
        norm = np.sqrt((x * x).sum())
        x = x * clip / max(norm, clip)
    m = b1 * m + (1 - b1) * x
    v = b2 * v + (1 - b2) * x * x
    return p - lr_t * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * m / (np.sqrt(v) + eps), m, v


def test_reference_is_tensorflow_clip_then_adam_with_staircase_for_mode_0():
    picked = [c for c in CASES if c["mode"] == 0 and c["clip"] > 0 and c["sched"] in (oc.SCHED_CONST, oc.SCHED_STAIR)]
    assert {"schedule", "tables", "clipping", "lengths", "alignment"} <= {c["family"] for c in picked}
    for c in picked:
        d, ref = data(c), oc.reference(c, data(c))
        decay = (c["dsteps"], c["dfactor"]) if c["sched"] == oc.SCHED_STAIR else None
        for k, i in enumerate(oc.live(c)):
            want = _tf_step(*(d[n][i].astype(np.float64) for n in "pgmv"), c["t"], c["lr"], c["b1"], c["b2"], c["eps"], c["scale"], c["clip"], decay)
            for name, w in zip("pmv", want):
                np.testing.assert_allclose(ref[k][name][0], w, rtol=1e-11, atol=1e-300, err_msg="%s of %s" % (name, c["name"]))


def test_lr_at_is_the_references_learning_rate_at_every_boundary():
    from heterofusionrcnn_amd.optim import lr_at
    seen = set()
    for c in oc.cases_of("schedule"):
        ref = oc.reference(c, data(c))[0]["lr"]
        got = lr_at(c["lr"], (c["dsteps"], c["dfactor"], c["sched"] == oc.SCHED_STAIR), c["t"] - 1)
        assert abs(got - ref) <= 4 * oc.U * ref, (c["name"], got, ref)             # powf within an ulp (2 u), one product, the rounded q
        seen.add((c["sched"], c["dsteps"], c["t"] - 1))
    assert {(s, 20000.0, g) for s in (1, 2) for g in oc.REF_STEPS} | {(s, 3.0, g) for s in (1, 2) for g in (2, 3, 9)} == seen


def test_fp32_floor_of_the_reference_schedule_is_the_integer_floor_at_every_step():
    g = np.arange(240001)
    q = np.floor(g.astype(np.float32) / np.float32(oc.REF_DECAY[0]))
    assert q.dtype == np.float32 and np.array_equal(q, g // 20000)
    t = (g + 1).astype(np.float32)                                                   # the kernel's counter: t - 1 in fp32
    assert np.array_equal(np.floor((t - np.float32(1)) / np.float32(oc.REF_DECAY[0])), g // 20000)


# ------------------------------------------------------------------------------------------------- the restatement and the bound
@pytest.mark.parametrize("family", ["alignment", "lengths", "tables", "clipping", "instantiations", "schedule", "grad_scale", "exact"])
def test_fp32_restatement_is_within_the_bound(family):
    worst = {}
    for c in oc.cases_of(family):
        got, partials = oc.kernel32(c, data(c))
        for k, r in oc.worst_ratios(c, data(c), got, partials).items():
            worst[k] = max(worst.get(k, 0.0), r)
            assert r <= 1.0, (c["name"], k, r)
    print(family, {k: round(v, 3) for k, v in worst.items()})
    assert worst["p"] > 0.05, "a bound nothing comes near checks little"


@pytest.mark.parametrize("plant", oc.PLANTS)
def test_planted_error_leaves_the_bound(plant):
    bad = []
    for c in oc.cases_of(oc.PLANT_FAMILY[plant]):
        got, partials = oc.kernel32(c, data(c), plant)
        r = oc.worst_ratios(c, data(c), got, partials)
        if max(r.values()) > 1.0:
            bad.append((c["name"], {k: v for k, v in r.items() if v > 1.0}))
    print(plant, len(bad), bad[:2])
    assert bad, "%s passes every case of the family %s" % (plant, oc.PLANT_FAMILY[plant])
    if plant == "drop_tail":
        assert all("partials" in r for _, r in bad)                                  # seen in the partials themselves, not only downstream
    if plant in ("nofloor", "t_for_tm1"):
        assert any("20000x0.8" in name for name, _ in bad)                           # at the reference's own boundaries


def test_exact_family_is_exact():
    for c in oc.cases_of("exact"):
        got, _ = oc.kernel32(c, data(c))
        for o, r in zip(got, oc.reference(c, data(c))):
            for k in "mv":
                assert same_bits(o[k], r[k][0].astype(np.float32)) and np.array_equal(r[k][0].astype(np.float32).astype(np.float64), r[k][0]), (c["name"], k)
    assert not oc.exact_grid_ok(np.array([5000]), np.array([0]), np.array([0]))       # g^2 past 2^24
    assert not oc.exact_grid_ok(np.array([1]), np.array([0]), np.array([0.5]))


# ------------------------------------------------------------------------------------------------- coverage
def test_every_instantiation_path_and_regime_has_a_case():
    seen = set()
    by_family = {}
    for c in CASES:
        r = oc.regimes_of(c)
        seen |= r
        by_family.setdefault(c["family"], set()).update(x for x in r if x[0] == "t")
    f32 = lambda x: float(np.float32(x))
    want = {("inst-path", kc, s, m, path) for kc in (0, 1) for s in (0, 1, 2) for m in (0, 1) for path in ("vec", "scalar")}
    want |= {("update-trips", x) for x in ("none", "partial", "one", "several")} | {("update-tail", True), ("update-tail", False)}
    want |= {("update-off", o) for n, o in oc.OFFSETS.items() if n != "aligned"} | {("update", "vec"), ("update", "scalar"), ("update", "mixed")}
    want |= {("norm", "vec"), ("norm", "scalar"), ("norm-tail", True), ("norm-tail", False)}
    want |= {("chunk", x) for x in ("full", "short", "one", "later")} | {("rows", x) for x in ("first>0", "first=0", "several", "one")}
    want |= {("table", "dropped"), ("entry", "multi"), ("entry", "sched"), ("t", "small"), ("t", "large")}
    want |= {("sched", s, 20000.0, f32(0.8), g) for s in (1, 2) for g in oc.REF_STEPS} | {("sched", s, 3.0, 0.5, g) for s in (1, 2) for g in (2, 3, 9)}
    want |= {("scale", 1.0), ("scale", 0.125), ("scale", f32(1.0 / 3.0))}
    assert want <= seen, sorted(want - seen, key=str)
    for family, ts in by_family.items():
        assert ("t", "large") in ts, family                                          # every family that checks p' also runs at a large t
    assert {n for c in oc.cases_of("lengths") for n in (x["n"] for x in c["tensors"])} == set(oc.LENGTHS)
    norms = {(c["clip"], x["norm"]) for c in oc.cases_of("clipping") for x in c["tensors"]}
    assert norms == {(f32(cl), r) for cl in (1.0, 0.7) for r in (0.0, 0.5, "one", 1.001, 50.0)}
    assert max(len(oc.live(c)) for c in oc.cases_of("tables")) == 7


def test_copy_cases_reach_every_regime():
    seen = set()
    for c in oc.COPY_CASES:
        seen |= oc.copy_regimes_of(c)
        assert len(c["entries"]) <= oc.COPY_MAX
    want = {("which", w) for w in range(64)} | {("n", n) for n in (1, 2, 63, 64)} | {("copy", "vec"), ("copy-chunk", "later")}
    want |= {("copy", "bytes", a, b) for a, b in ((True, False), (False, True), (True, True))}
    want |= {("copy-trips", x) for x in ("none", "partial", "one", "several")} | {("copy-tail", True), ("copy-tail", False)}
    want |= {("zero", x) for x in ("first", "middle", "last", "null")}
    assert want <= seen, sorted(want - seen, key=str)
    single = {(c["entries"][0], ) for c in oc.COPY_CASES if len(c["entries"]) == 1}
    assert {e[0][0] for e in single} == set(oc.COPY_BYTES)
    for b in oc.COPY_BYTES[:8]:
        assert {(b, do, so) for do in (0, 1) for so in (0, 1)} <= {e[0] for e in single}
    # the six steps find the owner of every workgroup: against the definition, on a table with zero-chunk copies in it
    first, chunks = oc.copy_first(dict(entries=[(0, 0, 0), (65537, 0, 0), (0, 0, 0), (1, 0, 0), (0, 0, 0)]))
    assert (first, chunks) == ([0, 0, 2, 2, 3], 3)
    assert [oc.copy_search(first, 5, chunks, b) for b in range(3)] == [1, 1, 3]


# ------------------------------------------------------------------------------------------------- argument checks, no launch
def test_adam_multi_and_copy_multi_refuse_bad_arguments_before_any_launch():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    fake = 16                       # a non-null address that is never dereferenced: every call below fails its checks first
    E, OK = _lib.HF_EINVAL, _lib.HF_OK

    def adam(n=1, table=fake, cmap=fake, step=fake, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, scale=1.0, mode=0):
        return L.hf_adam_multi(n, table, cmap, step, lr, b1, b2, eps, scale, mode, None)

    assert adam(n=-1) == E
    assert adam(table=None) == E and adam(cmap=None) == E and adam(step=None) == E
    assert adam(mode=2) == E and adam(mode=-1) == E
    assert adam(b1=1.0) == E and adam(b1=-0.1) == E and adam(b1=float("nan")) == E
    assert adam(b2=1.0) == E and adam(b2=-0.1) == E and adam(b2=float("nan")) == E
    assert adam(n=0, table=None, cmap=None, step=None) == OK                          # nothing to do, nothing launched
    assert adam(n=0, mode=2) == E                                                     # the checks come before the early return
    assert L.hf_adam_chunk() == oc.CHUNK

    assert L.hf_copy_multi_max() == oc.COPY_MAX

    def copy(n, dst, src, nbytes):
        arr = lambda xs, ty: None if xs is None else (ty * max(len(xs), 1))(*xs)
        return L.hf_copy_multi(n, arr(dst, ctypes.c_void_p), arr(src, ctypes.c_void_p), arr(nbytes, ctypes.c_longlong), None)

    many = oc.COPY_MAX + 1
    assert copy(many, [fake] * many, [fake] * many, [16] * many) == E                 # n > hf_copy_multi_max()
    assert copy(-1, [fake], [fake], [16]) == E
    assert copy(1, None, [fake], [16]) == E and copy(1, [fake], None, [16]) == E and copy(1, [fake], [fake], None) == E
    assert copy(1, [fake], [fake], [-1]) == E                                         # a negative byte count
    assert copy(2, [fake, fake], [fake, fake], [0, -5]) == E
    assert copy(1, [None], [fake], [16]) == E and copy(1, [fake], [None], [16]) == E  # a null pointer paired with bytes
    assert copy(3, [fake, None, fake], [fake, fake, fake], [0, 1, 0]) == E
    assert copy(2, [fake, fake], [fake, fake], [2 ** 46, 2 ** 46]) == E               # more workgroups than a grid holds
    assert copy(0, None, None, None) == OK
    assert copy(2, [None, fake], [None, fake], [0, 0]) == OK                          # zero bytes everywhere: nothing launched
