"""CPU tests of tests/bev_cases.py: the constants and rules it pins stand in csrc/bev_iou.hip, every case reaches the regime and the
sub-regimes its row names by the model, the fixtures hold their conditions, and the references agree with each other where they can
(the greedy sweep over the sparse fp64 adjacency against the fp32 oracle on the full matrix).  The fp32 oracle's error against the
fp64 clip is MEASURED here and the value bound of tests/test_bev_abi.py derived from it.

Run as a script, the module prints the table committed as profiles/bev_cases.md (up to the device-side section, which a GPU run
of tests/test_bev_abi.py fills)."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bev_cases as bc  # noqa: E402
import sampler_cases as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "bev_cases.md")
DEVICE_MARK = "## Device side"
ORACLE_MAX_N = 4800            # the full fp32 oracle costs ~0.3 us per pair: fine up to here

NMS_IDS = bc.nms_case_ids()
_id = lambda p: "%s-%g" % p


def _want(c, key, thresh):
    v = c[key]
    return v[thresh] if isinstance(v, dict) else v


# ------------------------------------------------------------------------------------------------ the source
def test_pinned_constants_and_rules_stand_in_the_source():
    with open(bc.SOURCE) as f:
        text = f.read()
    assert bc.missing_pins(text) == []
    assert bc.kSweepGatherers == 960 and bc.STREAM_LOAD_TRIP == 256 and bc.SLAB_ROWS == 65535 * 96
    # the check itself: a changed constant or rule is noticed
    for old, new in (("constexpr int kStreamRing = 4096;", "constexpr int kStreamRing = 8192;"), ("#define HF_IOU_ROWS 96", "#define HF_IOU_ROWS 80"),
                     ("col_t > row_t + 1 && w != 0ull", "col_t > row_t && w != 0ull"), ("std::min(cb, 64)", "std::min(cb, 32)"),
                     ("if (gy > 65535)", "if (gy > 65536)"), ("cb > 8192", "cb > 4096")):
        assert old in text
        assert bc.missing_pins(text.replace(old, new)), old


# ------------------------------------------------------------------------------------------------ the model
def test_model_on_hand_made_examples():
    n = 64 * 5
    # 0 -> 130 (block 2: filed), 0 -> 131 (the same entry), 1 -> 70 (block 1: next word, not filed), 70 -> 5 * 64 - 1 (block 4: filed)
    ai, aj = np.array([0, 0, 1, 70]), np.array([130, 131, 70, n - 1])
    counts = bc.filing(n, ai, aj)
    assert counts.tolist() == [0, 0, 1, 0, 1]
    assert bc.regime(n, counts) == "stream"
    keep, kept, km = bc.greedy_keep(n, ai, aj)
    assert kept == n - 3 and not km[[130, 131, 70]].any() and km[n - 1]          # 70 is suppressed, so n - 1 stays
    assert keep[:3].tolist() == [0, 1, 2] and keep[kept:].tolist() == [0] * 3 and keep[kept - 1] == n - 1
    assert bc.chains(ai, aj, km) == (1, 1)
    cb = 75
    z = np.zeros(cb, np.int64)
    one = lambda k, v: np.where(np.arange(cb) == k, v, z)
    assert bc.regime(4800, one(70, 600)) == "stream" and bc.regime(4800, one(70, 601)) == "barrier by average"    # 32 * 75 / 4
    assert bc.regime(4800, z + 32) == "stream" and bc.regime(4800, (z + 32) + one(3, 1)) == "barrier by average"
    assert bc.regime(4800, one(70, 2048)) == "barrier by average" and bc.regime(4800, one(70, 2049)) == "barrier by overflow"
    assert bc.regime(65536, np.zeros(1024, np.int64)) == "stream" and bc.regime(65537, np.zeros(1025, np.int64)) == "barrier by size"
    # the dense mask: both triangles, the diagonal tile strictly upper
    m = bc.dense_mask(130, np.array([0, 3]), np.array([3, 129]))
    assert m[0].tolist() == [8, 0, 0] and m[3].tolist() == [0, 0, 2] and m[129].tolist() == [8, 0, 0] and int(m.astype(bool).sum()) == 3


@pytest.mark.parametrize("case", NMS_IDS, ids=_id)
def test_case_reaches_its_regime(case):
    name, thresh = case
    c, m = bc.NMS_CASES[name], bc.nms_model(name, thresh)
    assert m["n"] == c["n"] and m["cb"] == (c["n"] + 63) // 64
    assert m["regime"] == _want(c, "regime", thresh), (m["regime"], m["total"], m["longest"])
    assert m["flags"] >= _want(c, "flags", thresh), (sorted(m["flags"]), m["total"], m["longest"])
    if name == "C":
        assert bc.STREAM_LOAD_TRIP < m["longest"] <= bc.kNmsListCap and int(np.argmax(m["counts"])) == bc.HUB_BLOCK
    if name == "D":
        assert bc.kSweepGatherers < m["counts"][bc.HUB_BLOCK] <= bc.kNmsListCap and m["total"] > bc.kStreamMaxAverage * m["cb"]
    if name == "E":
        assert m["counts"][bc.HUB_BLOCK] > bc.kNmsListCap
    if name == "B":
        assert m["total"] <= bc.kStreamMaxAverage * m["cb"] and m["longest"] <= bc.STREAM_LOAD_TRIP


def test_a_hub_moved_out_of_its_block_misses_the_regime():
    """the regime assertions depend on the planted positions: the hubs' last members one block to the left (next to nothing changes
    for the totals) leave block HUB_BLOCK without its long column"""
    fx = bc.nms_fixture("C")
    ai, aj = bc.adjacency(fx, 0.1)
    moved = lambda v: np.where(v // 64 == bc.HUB_BLOCK, v - 64 * 40, v)
    counts = bc.filing(fx["n"], np.minimum(moved(ai), moved(aj)), np.maximum(moved(ai), moved(aj)))
    assert counts[bc.HUB_BLOCK] == 0 and "column above 256" not in bc.flags(fx["n"], counts, ai, aj, np.ones(fx["n"], bool))


def test_every_regime_and_flag_is_reached():
    seen = {}
    for name, thresh in NMS_IDS:
        m = bc.nms_model(name, thresh)
        seen.setdefault(m["regime"], set()).update(m["flags"])
    assert set(seen) == {"stream", "barrier by average", "barrier by overflow", "barrier by size"}
    assert seen["stream"] >= {"word ring wraps", "entry ring wraps", "column above 256"}
    assert seen["barrier by average"] >= {"second chunk", "column above kSweepGatherers", "share rule alone", "next word across chunks"}
    assert seen["barrier by overflow"] >= {"second chunk", "overflow with chunking"}
    assert seen["barrier by size"] >= {"second chunk"}
    assert {bc.NMS_CASES[n]["n"] for n, _ in NMS_IDS} >= {1, 63, 64, 65, 128, 129, 4096, 4097}
    # the batched call: its frames take different forms
    forms = [m["regime"] for _, m in bc.batch_frames()]
    assert forms[0] == "stream" and forms[1].startswith("barrier") and forms[2] == "stream" and bc.batch_frames()[2][1]["total"] == 0
    assert len({len(b) for b, _ in bc.batch_frames()}) == 1
    # C truncated for the dense mask check still has tiles on, next to and right of the diagonal
    m = bc.nms_model("C", 0.1, 1024)
    assert m["cb"] == 16 and len(m["ai"]) > 0
    # the IoU matrix: partial and full tiles in both directions, more than one block each way, vector and scalar rows, the slab walk
    shapes = set(bc.IOU_SHAPES)
    assert {(1, 1), (96, 64), (97, 63), (193, 130), (300, 3), (300, 5)} <= shapes
    assert bc.SLAB_SHAPE[0] > bc.SLAB_TILES * bc.kIouRows and -(-bc.SLAB_SHAPE[0] // bc.kIouRows) == bc.SLAB_TILES + 2
    assert set(bc.SLAB_PLANTED) == {0, bc.SLAB_ROWS - 1, bc.SLAB_ROWS, bc.SLAB_ROWS + 1, bc.SLAB_SHAPE[0] - 1}


# ------------------------------------------------------------------------------------------------ the fixtures
@pytest.mark.parametrize("name", list(bc.NMS_CASES))
def test_nms_fixture_conditions(name):
    fx, c = bc.nms_fixture(name), bc.NMS_CASES[name]
    assert fx["n"] == c["n"] and fx["boxes"].shape == (c["n"], 5) and fx["boxes"].dtype == np.float32
    assert bc.circles_clear(fx) >= bc.MIN_GAP, "two sites come too close: a cross-site pair might not be an exact zero"
    assert (fx["site"][fx["pi"]] == fx["site"][fx["pj"]]).all() and (fx["pi"] < fx["pj"]).all()
    for t in c["thresh"]:
        assert (np.abs(fx["piou"] - t) >= bc.MARGIN).all(), "a same-site pair within the margin of threshold %g" % t
    assert fx["shrunk"] == 0
    # headings: every same-site pair at least HEADING_SLOT from parallel and from perpendicular
    d = np.abs(fx["boxes"][fx["pi"], 4].astype(np.float64) - fx["boxes"][fx["pj"], 4])
    if len(d):
        assert d.min() >= bc.HEADING_SLOT and d.max() <= np.pi / 2 - bc.HEADING_SLOT, (d.min(), d.max())
    if name in bc.CHAIN_CASES:
        m = bc.nms_model(name, c["thresh"][0])
        assert m["chains"] > 0 and m["chains_filed"] > 0, "greedy suppression is transitive everywhere: kept_row decides nothing"
    if c["n"] <= 129 and c["n"] > 1:
        # the small cases in full: the fp64 IoU of every cross-site pair is an exact zero (a separating axis parts them)
        gap = sc.bev_gap(bc.bev7(fx["boxes"]), bc.bev7(fx["boxes"]))
        cross = fx["site"][:, None] != fx["site"][None, :]
        assert (gap[cross] > bc.MIN_GAP).all()


@pytest.mark.parametrize("name", bc.iou_case_ids() + ["slab"])
def test_iou_fixture_conditions(name):
    c = bc.iou_case(name)
    assert c["a"].shape == (c["na"], 5) and c["b"].shape == (c["nb"], 5)
    assert bc.circles_clear(c["fx"]) >= bc.MIN_GAP
    assert len(c["rows"]) > 0 and (c["iou"] > 0).any(), "no overlapping pair at all"
    gap = sc.bev_gap(bc.bev7(c["a"]), bc.bev7(c["b"]))
    same = np.zeros((c["na"], c["nb"]), bool)
    same[c["rows"], c["cols"]] = True
    assert (gap[~same] > bc.MIN_GAP).all()
    if name == "dense":
        # every pair of the tile survives the device's filters: all 6144 overlap, well above zero
        assert len(c["rows"]) == bc.kIouRows * 64 and c["iou"].min() > 0.05
    if name == "slab":
        assert len(c["rows"]) == len(bc.SLAB_PLANTED) * bc.SLAB_SHAPE[1] and c["iou"].min() > 0.05
        far = bc.bev7(bc.FAR_BOX[None])
        assert (sc.bev_gap(far, bc.bev7(c["b"])) > 1000).all()


# ------------------------------------------------------------------------------------------------ the references against each other
@functools.lru_cache(maxsize=None)
def measured(kind, name):
    """(largest |fp32 oracle - fp64 clip| over the same-site pairs, pairs, the bound derived from it)"""
    import oracle
    fx = bc.nms_fixture(name) if kind == "nms" else bc.iou_case(name)["fx"]
    err, pairs = bc.oracle_site_error(oracle, fx)
    return err, pairs, bc.value_bound(err)


def all_measured():
    return [("nms", n) for n in bc.NMS_CASES] + [("iou", n) for n in bc.iou_case_ids() + ["slab"]]


def test_oracle_error_and_the_bound_derived_from_it(oracle_mod):
    worst = 0.0
    for kind, name in all_measured():
        err, pairs, bound = measured(kind, name)
        print("%s %s: |oracle - fp64| <= %.3g over %d same-site pairs, bound %.3g" % (kind, name, err, pairs, bound))
        worst = max(worst, err)
        assert bound == sc.ELU_FACTOR * max(err, sc.U)
        # the margin the fixtures were drawn with covers the bound plus the margin test_ops_gpu._drop_borderline uses
        assert bound + 3e-5 <= bc.MARGIN, (kind, name, err)
    assert worst > sc.U, "the oracle equals the fp64 clip to the last bit: the measurement measures nothing"


@pytest.mark.parametrize("case", [p for p in NMS_IDS if bc.NMS_CASES[p[0]]["n"] <= ORACLE_MAX_N], ids=_id)
def test_greedy_reference_equals_the_oracle(oracle_mod, case):
    name, thresh = case
    fx, m = bc.nms_fixture(name), bc.nms_model(name, thresh)
    keep, kept = oracle_mod.oriented_nms(fx["boxes"], thresh, return_count=True)
    assert kept == m["kept"] and np.array_equal(keep, m["keep"])
    if m["n"] <= 1024:
        mask = bc.dense_mask(m["n"], m["ai"], m["aj"])
        assert np.array_equal(mask, oracle_mod.nms_mask(fx["boxes"], thresh))
        keep2, kept2 = oracle_mod.nms_sweep(mask)
        assert kept2 == m["kept"] and np.array_equal(keep2, m["keep"])


def test_truncated_mask_equals_the_oracle(oracle_mod):
    m = bc.nms_model("C", 0.1, 1024)
    assert np.array_equal(bc.dense_mask(1024, m["ai"], m["aj"]), oracle_mod.nms_mask(bc.nms_fixture("C")["boxes"][:1024], 0.1))


# ------------------------------------------------------------------------------------------------ the equal-heading family
@functools.lru_cache(maxsize=None)
def equal_measured(name):
    import oracle
    c = bc.equal_case(name)
    di, dj, closed, pairs, _ = bc.equal_disagreement(oracle, name)
    _, oi = oracle.compute_bev_iou(c["boxes"], c["boxes"])
    diff = oi[c["pi"], c["pj"]].astype(np.float64) - c["piou"]
    return dict(pairs=pairs, differ=len(di), share=len(di) / pairs, off=float((np.abs(diff) > 1e-3).mean()), high=float(diff.max()), low=float(diff.min()))


@pytest.mark.parametrize("name", bc.equal_case_ids())
def test_equal_heading_family(oracle_mod, name):
    c = bc.equal_case(name)
    n = int(name.split("-")[0])
    assert c["boxes"].shape == (n, 5) and len(c["pi"]) > n // 2
    # the closed form is the fp64 clip's value (the menu shifts are exact in the box frame), and clear of the threshold
    b7 = bc.bev7(c["boxes"])
    for k in range(0, len(c["pi"]), 7):
        assert abs(bc.ref_pair(b7[c["pi"][k]], b7[c["pj"][k]])[1] - c["piou"][k]) < 1e-5
    assert np.abs(c["piou"] - bc.EQUAL_THRESH).min() > 5e-3 and (c["piou"] > bc.EQUAL_THRESH).any() and (c["piou"] < bc.EQUAL_THRESH).any()
    heads = c["boxes"][:, 4]
    assert (heads == 0).all() if "aligned" in name else (heads != 0).all()
    m = equal_measured(name)
    print("%s: %d overlapping pairs, the oracle decides against the closed form on %d (%.2f %%), value off by more than 1e-3 on %.2f %%, "
          "oracle - closed form in [%.3g, %.3g]" % (name, m["pairs"], m["differ"], 100 * m["share"], 100 * m["off"], m["low"], m["high"]))
    assert m["share"] < bc.EQUAL_CAP


# ------------------------------------------------------------------------------------------------ the table
def table():
    out = ["# BEV IoU and oriented NMS: the case table of tests/bev_cases.py", "",
           "Printed by `python tests/test_bev_cases_cpu.py` (everything above \"%s\"); the device-side section is filled from a run of" % DEVICE_MARK,
           "`tests/test_bev_abi.py` on an MI355X.", "",
           "## NMS cases (hf_oriented_nms, hf_oriented_nms_batched, hf_nms_mask)", "",
           "List counts, regime and flags by the model of bev_cases.py (filing(), regime(), flags()); chains = pairs (b, c) with b suppressed, c kept and",
           "b adjacent to c, all / those filed in a column list (where the sweep's kept_row test decides).", "",
           "| case | n | cb | threshold | list entries | longest column | regime | flags | chains | kept | pairs | oracle - fp64 | bound |",
           "|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, thresh in NMS_IDS:
        m = bc.nms_model(name, thresh)
        err, pairs, bound = measured("nms", name)
        out.append("| %s | %d | %d | %g | %d | %d | %s | %s | %d / %d | %d | %d | %.3g | %.3g |"
                   % (name, m["n"], m["cb"], thresh, m["total"], m["longest"], m["regime"], ", ".join(sorted(m["flags"])) or "-", m["chains"],
                      m["chains_filed"], m["kept"], pairs, err, bound))
    fr = bc.batch_frames()
    out += ["", "Batched case H: %d frames of %d boxes at threshold %g: %s." % (len(fr), len(fr[0][0]), bc.BATCH_THRESH, ", ".join(
        "%s (%s, %d entries, %d kept)" % (nm, m["regime"], m["total"], m["kept"]) for nm, (_, m) in zip(bc.BATCH_FRAMES, fr))), "",
            "## IoU-matrix cases (hf_compute_bev_iou)", "", "| case | num_a | num_b | same-site pairs | oracle - fp64 | bound |", "|---|---|---|---|---|---|"]
    for name in bc.iou_case_ids() + ["slab"]:
        c = bc.iou_case(name)
        err, pairs, bound = measured("iou", name)
        na, nb = bc.SLAB_SHAPE if name == "slab" else (c["na"], c["nb"])
        out.append("| %s | %d | %d | %d | %.3g | %.3g |" % (name, na, nb, len(c["rows"]), err, bound))
    worst = max(measured(k, n)[0] for k, n in all_measured())
    out += ["", "Largest |fp32 oracle - fp64 clip| over every same-site pair of every generic-heading case: %.3g; the bound derived from it" % worst,
            "(%d x the error, floored at 2^-24): %.3g; with the 3e-5 of `_drop_borderline`: %.3g, below the %.0e the fixtures were drawn with."
            % (sc.ELU_FACTOR, bc.value_bound(worst), bc.value_bound(worst) + 3e-5, bc.MARGIN), "",
            "## Equal-heading family (threshold %g)" % bc.EQUAL_THRESH, "",
            "| case | overlapping pairs | oracle decides against the closed form | share | value off by > 1e-3 | oracle - closed form |", "|---|---|---|---|---|---|"]
    for name in bc.equal_case_ids():
        m = equal_measured(name)
        out.append("| %s | %d | %d | %.2f %% | %.2f %% | %.3g .. %.3g |" % (name, m["pairs"], m["differ"], 100 * m["share"], 100 * m["off"], m["low"], m["high"]))
    return "\n".join(out) + "\n"


def test_profile_table_is_current(oracle_mod):
    with open(PROFILE) as f:
        text = f.read()
    assert "\n" + DEVICE_MARK in text
    assert text.split("\n" + DEVICE_MARK)[0].rstrip() == table().rstrip(), "profiles/bev_cases.md is stale: python tests/test_bev_cases_cpu.py prints it"


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.stdout.write(table())
