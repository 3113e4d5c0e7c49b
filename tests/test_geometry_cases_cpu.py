"""tests/geometry_cases.py checked on any machine: the constants and rule literals it restates are read back from the sources, every case
is in the regime it is named for, the project's CPU oracle agrees with the module's independent NumPy statement on every case (a
tie-handling slip in either shows without a GPU), and the inputs are sharp: every FPS case has tied rounds, every ball-query case has
balls with fewer hits than nsample and balls with more, every kNN case has a tie at the k-th place."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "heterofusionrcnn_amd", "csrc")
CASES = gc.all_cases()


def _source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_case_ids_are_unique_and_counted():
    ids = [gc.case_id(c) for c in CASES]
    assert len(ids) == len(set(ids))
    count = {f: len(gc.cases_of(f)) for f in ("fps", "bq", "knn", "topk")}
    assert count == dict(fps=71, bq=46, knn=25, topk=3), "a case was added or removed: update these numbers when you change the table"


@pytest.mark.parametrize("name,constant,value", gc.SOURCE_CONSTANTS, ids=lambda v: str(v))
def test_constants_are_those_of_the_sources(name, constant, value):
    found = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % constant, _source(name))
    assert found == [str(value)], "%s of %s changed: the restated rules of geometry_cases.py and the regimes of its cases depend on it" % (constant, name)


@pytest.mark.parametrize("name,text", gc.SOURCE_RULES, ids=lambda v: v[:40].replace(" ", "_"))
def test_rule_literals_are_those_of_the_sources(name, text):
    assert _source(name).count(text) == 1, "the dispatch rule of %s changed: restate it in geometry_cases.py (%r)" % (name, text)


def test_the_product_build_compiles_the_diagnostic_knobs_out():
    common = _source("hf_common.h")
    assert "#define HF_DIAG_INT(name, dflt) (dflt)" in common and "#ifdef HF_DIAG\n" in common
    with open(os.path.join(CSRC, "Makefile")) as f:
        assert "HF_DIAG" not in f.read()


def test_the_getter_and_the_python_wrapper_agree_with_the_restated_constants():
    from heterofusionrcnn_amd import _lib
    from heterofusionrcnn_amd import grouping, sampling
    L = _lib.lib()
    assert L.hf_fps_onchip_limit() == gc.FPS_MAX_POINTS
    assert L.hf_fps_workspace(3, gc.FPS_MAX_POINTS) == 0 and L.hf_fps_workspace(3, gc.FPS_MAX_POINTS + 1) == 4 * 3 * (gc.FPS_MAX_POINTS + 1)
    assert L.hf_knn_workspace(1, gc.KNN_BIN_MAX_DATA) > 0 and L.hf_knn_workspace(1, gc.KNN_BIN_MAX_DATA + 1) == 0
    for b, n in ((2, 1000), (2, 1024), (130, 1025), (3, 4096), (1, 4097), (1, 16385), (1, gc.PACKED_MAX_N + 1)):
        assert L.hf_ball_query_workspace(b, n) == gc.sorted_workspace(b, n)
    assert tuple(sorted(sampling.FPS_KERNELS, key=sampling.FPS_KERNELS.get)) == gc.FPS_KERNELS
    assert tuple(sorted(grouping.BALL_QUERY_VARIANTS, key=grouping.BALL_QUERY_VARIANTS.get)) == gc.BQ_VARIANTS


def test_diagnostic_only_list_cites_real_lines_and_is_disjoint_from_the_cases():
    diag = gc.diagnostic_instantiations()
    assert len(diag) == len(gc.DIAGNOSTIC_ONLY) == 15
    assert not diag & gc.selected_instantiations()
    for name, args, source, line in gc.DIAGNOSTIC_ONLY:
        assert sum(l.strip().startswith(line) for l in _source(source).splitlines()) == 1, (name, args, line)


# ---------------------------------------------------------------------------------------------- regimes
def test_fps_cases_cover_every_bucket_edge():
    seen = {}
    for c in gc.cases_of("fps"):
        b, n, m = c["b"], c["n"], c["m"]
        d = gc.fps_dispatch(n, m, c["kernel"], c["threads"])
        assert d is not None and 2 <= m and (32 <= m <= 300), gc.case_id(c)
        seen.setdefault(d, []).append((n, m))
        if c["regime"] == "wave":
            assert d[0] == "fps_wave_kernel" and gc.fps_dispatch(n, m) == d and (b == 1 or (b % 4 != 0 and gc.fps_wave_grid(b) > 1))
        elif c["regime"] == "plain":
            assert d == ("fps_onchip_kernel", (d[1][0], c["threads"]))
        elif c["regime"] == "bucket":
            assert d == ("fps_bucket_kernel", (d[1][0], c["threads"]))
        else:
            assert d == ("fps_scratch_kernel", ()) and n == gc.FPS_MAX_POINTS + 1
        assert c["same"] is None or c["same"] < b
    assert set(n for v in seen.values() for n, _ in v) >= set(gc.WAVE_N)
    for (name, args), shapes in seen.items():
        if name in ("fps_onchip_kernel", "fps_bucket_kernel"):
            p, nt = args
            ns = sorted(n for n, _ in shapes)
            assert ns[-1] == p * nt, (name, args)                                # the upper edge of the PPT bucket
            assert ns[0] % 64 != 0 and (p == 1 or ns[0] == (p // 2) * nt + 1), (name, args)   # its lower edge plus one; no multiple of 64
        elif name == "fps_wave_kernel":
            p = args[0]
            ns = sorted(set(n for n, _ in shapes))
            assert ns[-1] == 64 * p and (p == 1 or ns[0] == 32 * p + 1)
    for regime in ("wave", "plain", "bucket"):
        fam = [c for c in gc.cases_of("fps") if c["regime"] == regime]
        assert any(c["m"] > c["n"] for c in fam) and sum(c["same"] is not None for c in fam) == 1, regime
    # the forced workgroup sizes are refused where the library refuses them
    assert gc.fps_dispatch(4097, 64, "plain", 256) is None and gc.fps_dispatch(16384, 64, "plain", 1024) == ("fps_onchip_kernel", (16, 1024))
    assert gc.fps_dispatch(513, 64, "wave") is None and gc.fps_dispatch(8192, 256) == ("fps_bucket_kernel", (16, 512))
    assert gc.fps_dispatch(8192, 255) == ("fps_onchip_kernel", (16, 512)) and gc.fps_dispatch(4096, 300) == ("fps_onchip_kernel", (16, 256))


def test_ball_query_cases_are_in_their_regimes():
    cells, builds = set(), set()
    for c in gc.cases_of("bq"):
        b, n, m, ns, w = c["b"], c["n"], c["m"], c["nsample"], c["want"]
        inst = gc.instantiations(c)
        assert inst, gc.case_id(c)
        names = {name for name, _ in inst}
        assert min(n // 2, 2 * ns + 50) > ns, gc.case_id(c)          # the dense cube of make_inputs overflows a row
        assert m < 300 or c["regime"] in ("tiles", "auto_ws", "auto_ws_few_clouds"), gc.case_id(c)
        if c["off"] or c["ws"]:
            assert c["variant"] in ("cell", "sorted", "auto")        # these go through the C ABI
        if c["off"]:
            assert n % 4 == 0 and w["a4"] is False
        if "qpw" in w:
            assert names == {"qbp_cell_kernel"} and gc.cell_geometry(b, m, ns) == (w["qpw"], w["sm"]), gc.case_id(c)
            assert inst == {("qbp_cell_kernel", (c["group"], w["sm"], 1024, w["a4"]))}
            assert w["a4"] or c["off"] or n % 4 != 0
            cells.add((c["group"], w["sm"], w["a4"], w["qpw"], ns))
        elif "build" in w:
            assert inst == {("bq_build_kernel", w["build"]), ("bq_query_kernel", (c["group"], 1, 8))}, gc.case_id(c)
            assert w["packed"] == (n <= gc.PACKED_MAX_N)
            builds.add((w["build"], gc.sorted_split(b), w["packed"], c["group"]))
            if c["variant"] == "auto":
                assert c["ws"] and b >= 32 and b * gc.cdiv(m, 128) > gc.NUM_CU
        else:
            assert inst == {("qbp_bruteforce_kernel", (c["group"],))}
            assert c["variant"] == "bruteforce" or ns > 128
        if c["regime"] == "auto_ws_few_clouds":
            assert b == 31 and b * gc.cdiv(m, 128) > gc.NUM_CU
        if c["regime"] == "auto_ws_one_round":
            assert b >= 32 and b * gc.cdiv(m, 128) == gc.NUM_CU
    assert {(g, sm, a4) for g, sm, a4, _, _ in cells} == {(g, sm, a4) for g in (False, True) for sm in (1, 2) for a4 in (False, True)}
    assert {q for _, _, _, q, _ in cells} == set(gc.CELL_QPW) and {ns for _, _, _, _, ns in cells} >= {7, 32, 64, 128}
    assert {(q, sm) for _, sm, _, q, _ in cells} >= {(256, 1), (256, 2), (128, 1), (128, 2), (64, 1), (64, 2), (32, 1), (32, 2), (16, 2)}
    assert {bd for bd, _, _, _ in builds} == set(gc.BQ_BUILD)
    assert {(bd, g) for bd, _, _, g in builds} == {(bd, g) for bd in gc.BQ_BUILD for g in (False, True)}
    assert {s for _, s, _, _ in builds} == {1, 2, 4} and {p for _, _, p, _ in builds} == {False, True}
    # the edges of the clouds-per-chip rule
    assert [gc.sorted_split(b) for b in (64, 65, 128, 129)] == [4, 2, 2, 1]


def test_knn_cases_are_in_their_regimes():
    seen = set()
    for c in gc.cases_of("knn"):
        b, n, m, k, w = c["b"], c["n"], c["m"], c["k"], c["want"]
        inst = gc.instantiations(c)
        assert inst, gc.case_id(c)
        seen |= inst
        if c["regime"] == "small":
            assert inst == {("knn_small_kernel", (k,))}
        elif "parts" in w:
            assert inst == {("knn_kernel", (w["parts"],))}, gc.case_id(c)
        else:
            assert c["entry"] in ("sorted", "three_nn") and ("knn_bin_kernel", ()) in inst and n <= gc.KNN_BIN_MAX_DATA
            assert (("knn_grid_reg_kernel", (k,)) in inst) == (k in gc.KNN_REG_K) and (("knn_grid_kernel", ()) in inst) == (k not in gc.KNN_REG_K)
            assert (c["entry"] == "three_nn") == (k == 3)
    assert any(c["k"] == c["n"] for c in gc.cases_of("knn")) and any(c["k"] == 67 and c["entry"] == "all_pairs" for c in gc.cases_of("knn"))
    assert any(c["n"] > gc.KNN_TILE and c["n"] % gc.KNN_TILE for c in gc.cases_of("knn") if c["regime"] == "small")
    assert gc.knn_dispatch(1, 100, 5, 70) is None and gc.knn_dispatch(1, 100, 5, 69) is not None and gc.knn_dispatch(1, 5, 5, 6) is None


# ---------------------------------------------------------------------------------------------- oracle against the independent statement
@pytest.mark.parametrize("c", CASES, ids=gc.case_id)
def test_oracle_equals_the_independent_statement_and_the_inputs_are_sharp(oracle_mod, c):
    t = gc.make_inputs(c)
    mine = gc.statement(c, t)
    sharp = mine.pop("sharp")
    theirs = gc.oracle_outputs(c, t, oracle_mod)
    assert set(theirs) == set(mine)
    for name in theirs:
        assert theirs[name].dtype == mine[name].dtype and np.array_equal(theirs[name], mine[name]), name
    if c["family"] == "fps":
        assert (sharp["tied_rounds"] >= 1).all(), "every cloud has a round with two equally far points"
        x = t["xyz"]
        h, w = c["n"] // 2, gc.wrap_block(c["n"])
        keep = np.ones(h, bool)
        if w is not None and w.stop > h:               # the wrap block lies in the second half: it repeats points 100 .. instead
            keep[w.start - h:w.stop - h] = False
        assert np.array_equal(x[:, h:2 * h][:, keep], x[:, :h][:, keep])
        if w is not None:
            assert np.array_equal(x[:, w], x[:, gc.WRAP_SOURCE:gc.WRAP_SOURCE + w.stop - w.start])
            others = [i for i in range(c["b"]) if i != c["same"]]
            assert (sharp["higher_index_wins"][others] >= 1).all(), "no tie of this cloud goes to the higher index (k mod 512 first)"
        else:
            assert (sharp["higher_index_wins"] == 0).all()
        if c["same"] is not None:
            assert (x[c["same"]] == x[c["same"], 0]).all() and (mine["out"][c["same"]] == 0).all()
    elif c["family"] == "bq":
        assert sharp["fewer"] >= 1 and sharp["more"] >= 1, sharp
        assert c["m"] < 8 or sharp["none"] >= 1
    elif c["family"] == "knn":
        assert sharp["tied_queries"].sum() >= 1, "no query has a tie at the k-th place"
    else:
        assert sharp["tied_rows"] >= 1
