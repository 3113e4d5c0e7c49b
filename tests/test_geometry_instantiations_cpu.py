"""Coverage guard of the point-geometry parity suite, on any machine with hipcc: csrc/sampling.hip, grouping.hip, ballquery.hip and
ballquery_sorted.hip are compiled to assembly with the Makefile's flags, and the set of kernels in the four code objects must equal the
instantiations that the cases of tests/geometry_cases.py select by the restated dispatch rules, plus the diagnostic-only instantiations
listed there one by one (the product build can never launch them), plus the kernels of families pinned elsewhere, also listed one by
one.  A new instantiation cannot land without a case, and a case table that stops reaching one fails here without a GPU.  Only the
kernel-metadata table is read (names, LDS, registers, spills, scratch).  Run as a script, the module prints the table committed as
profiles/geometry_instantiations.md."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import geometry_cases as gc  # noqa: E402
from kernel_asm import compile_to_assembly, kernel_table  # noqa: E402


def compile_all(directory):
    """[(source, kernel, template arguments, metadata)] of the four sources"""
    rows = []
    for source in gc.SOURCES:
        rows += [(source, name, args, f) for name, args, f in kernel_table(compile_to_assembly(directory, source))]
    return rows


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return compile_all(tmp_path_factory.mktemp("geometry_asm"))


def in_scope(table):
    return [(name, args) for source, name, args, _ in table if (source, name, args) not in gc.OUT_OF_SCOPE]


def test_every_out_of_scope_kernel_exists(table):
    compiled = {(source, name, args) for source, name, args, _ in table}
    assert len(set(gc.OUT_OF_SCOPE)) == len(gc.OUT_OF_SCOPE)
    assert not set(gc.OUT_OF_SCOPE) - compiled, sorted(set(gc.OUT_OF_SCOPE) - compiled)
    assert not {name for _, name, _ in gc.OUT_OF_SCOPE} & {name for name, _ in gc.selected_instantiations() | gc.diagnostic_instantiations()}


def test_compiled_kernels_are_the_selected_and_the_diagnostic_only_ones(table):
    scoped = in_scope(table)
    compiled = set(scoped)
    assert len(scoped) == len(compiled), "a kernel of this family is compiled into two of the sources"
    selected, diag = gc.selected_instantiations(), gc.diagnostic_instantiations()
    assert not selected & diag, sorted(selected & diag)
    assert not compiled - selected - diag, "compiled but reached by no case of geometry_cases.py: %s" % sorted(compiled - selected - diag)
    assert not selected - compiled, "the dispatch rule restated in geometry_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert not diag - compiled, "listed as diagnostic-only but not compiled: %s" % sorted(diag - compiled)


def test_every_family_alone_reaches_its_kernels(table):
    """no family leans on another one's cases"""
    compiled = set(in_scope(table)) - gc.diagnostic_instantiations()
    prefix = dict(fps=("fps_",), bq=("qbp_", "bq_"), knn=("knn_",), topk=("select_top_k",))
    for family, pre in prefix.items():
        want = {i for i in compiled if i[0].startswith(pre)}
        assert want and gc.selected_instantiations(gc.cases_of(family)) == want, family
    assert sum(len({i for i in compiled if i[0].startswith(pre)}) for pre in prefix.values()) == len(compiled)


def test_the_instantiation_counts_follow_the_dispatch_tables(table):
    count = {}
    for name, _ in in_scope(table):
        count[name] = count.get(name, 0) + 1
    diag = {}
    for name, _ in gc.diagnostic_instantiations():
        diag[name] = diag.get(name, 0) + 1
    assert diag == dict(qbp_cell_kernel=10, bq_query_kernel=4, fps_onchip_kernel=1)
    assert count == dict(fps_wave_kernel=len(gc.FPS_WAVE_PPT),
                         fps_onchip_kernel=sum(len(v) for v in gc.FPS_PLAIN_PPT.values()) + diag["fps_onchip_kernel"],
                         fps_bucket_kernel=sum(len(v) for v in gc.FPS_BUCKET_PPT.values()), fps_scratch_kernel=1,
                         qbp_bruteforce_kernel=2, qbp_cell_kernel=2 * len(gc.CELL_STORE_MODES) * 2 + diag["qbp_cell_kernel"],
                         bq_build_kernel=len(gc.BQ_BUILD), bq_query_kernel=2 + diag["bq_query_kernel"],
                         knn_small_kernel=len(gc.KNN_SMALL_K), knn_kernel=len(gc.KNN_PARTS), knn_bin_kernel=1,
                         knn_grid_reg_kernel=len(gc.KNN_REG_K), knn_grid_kernel=1, select_top_k_kernel=1)


def render(table):
    reach = {}
    for c in gc.all_cases():
        for inst in gc.instantiations(c):
            reach[inst] = reach.get(inst, 0) + 1
    diag = gc.diagnostic_instantiations()
    lines = ["# Kernels and template instantiations of the point-geometry sources", "",
             "csrc/sampling.hip, csrc/grouping.hip, csrc/ballquery.hip and csrc/ballquery_sorted.hip compiled for gfx950 with the Makefile's flags",
             "(`-O3 -ffp-contract=off`); produced by `python tests/test_geometry_instantiations_cpu.py`.  Template arguments:",
             "`fps_wave_kernel<PPT>`, `fps_onchip_kernel` / `fps_bucket_kernel<PPT, NT>`, `qbp_bruteforce_kernel<GROUP>`,",
             "`qbp_cell_kernel<GROUP, SM, NT, A4>`, `bq_build_kernel<PPT, HB, S>`, `bq_query_kernel<GROUP, SM, G>`, `knn_small_kernel<K>`,",
             "`knn_kernel<PARTS>`, `knn_grid_reg_kernel<K>`.  LDS is the static part (the ball-query and the tiled kNN kernels take theirs at",
             "launch).  `cases` counts the cases of `tests/geometry_cases.py` whose forced call launches the kernel; `diagnostic only` marks the",
             "instantiations that the product build cannot launch (`DIAGNOSTIC_ONLY` of that module names the source line); the kernels of the",
             "row-gather machine and `group_concat_kernel` in these sources belong to other suites (`OUT_OF_SCOPE`) and are left out.", "",
             "| source | kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | cases | diagnostic only |",
             "|---|---|---|---:|---:|---:|---:|---:|---:|---|"]
    shown = 0
    for source, name, args, f in table:
        if (source, name, args) in gc.OUT_OF_SCOPE:
            continue
        shown += 1
        lines.append("| %s | `%s` | %s | %d | %d | %d | %d | %d | %d | %s |" % (source, name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"],
                                                                             f["spill"], f["sgpr_spill"], f["scratch"], reach.get((name, args), 0),
                                                                             "yes" if (name, args) in diag else ""))
    lines += ["", "%d kernels (%d diagnostic only), %d cases." % (shown, len(diag), len(gc.all_cases()))]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(compile_all(d)))
