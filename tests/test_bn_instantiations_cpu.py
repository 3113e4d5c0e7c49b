"""Coverage guard of the BatchNorm parity suite, on any machine with hipcc: csrc/mlp.hip is compiled to assembly with the Makefile's
flags, and the set of kernels in the code object must equal the set of kernels and template instantiations that the cases of
tests/bn_cases.py select by the restated dispatch rule.  A new instantiation cannot land without a case, and a case table that stops
reaching one fails here without a GPU.  The restated launch geometry is checked against the 1024-thread workgroup limit for every
channel count the entry points accept.  Run as a script, the module prints the table committed as profiles/mlp_instantiations.md."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bn_cases as bc  # noqa: E402
from kernel_asm import compile_to_assembly, kernel_table  # noqa: E402

MAX_THREADS = 1024
LDS_PER_WORKGROUP = 64 * 1024
ROW_COUNTS = (1, 2, 7, 255, 256, 257, 4096, 4097, 100003, 1 << 22)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("mlp_asm"), "mlp.hip"))


def test_case_ids_are_unique():
    ids = [bc.case_id(c) for c in bc.all_cases()]
    assert len(ids) == len(set(ids))


def test_every_compiled_kernel_is_selected_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = bc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case of bn_cases.py: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the dispatch rule restated in bn_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled)


def test_exact_family_alone_reaches_every_kernel(table):
    """the bit-for-bit family is the one that sees dropped rows and wrong block edges: it does not lean on the rounding family"""
    compiled = {(name, args) for name, args, _ in table}
    exact = bc.selected_instantiations([c for c in bc.all_cases() if c["family"] == "exact"])
    assert compiled == exact, sorted(compiled - exact)


def test_no_case_can_be_removed_unnoticed():
    """every case is either the only one of its (kind, family) to reach one of its kernels, or listed by name in the tables of bn_cases.py:
    here, the shapes the issue names must all be present, on the route it names"""
    ids = {bc.case_id(c) for c in bc.all_cases()}
    for rows, c in bc.STREAM4 + bc.STREAM1 + tuple(p[1] for p in bc.STRADDLE):
        assert bc.small_geom(rows, c) is None, (rows, c)
        for kind in ("train", "bwd", "eval", "bwd_dx", "stats"):
            assert any(i.startswith(kind + "-exact-rows%d-c%d" % (rows, c)) for i in ids), (kind, rows, c)
    for rows, c in bc.SMALL:
        assert bc.small_geom(rows, c) is not None, (rows, c)
        for kind in ("train", "bwd"):
            assert sum(i.startswith(kind + "-exact-rows%d-c%d-" % (rows, c)) for i in ids) >= 4, (kind, rows, c)
    for small, streaming in bc.STRADDLE:
        assert bc.small_geom(*small) is not None and bc.small_geom(*streaming) is None
    assert len(bc.cases_of("pool")) == len(bc.POOLS) * 8 and len(bc.cases_of("narrow")) == len(bc.NARROWS) * 2
    assert len(bc.cases_of("drop")) == len(bc.DROP_SHAPES) * (2 * len(bc.DROP_RATES) + 5) + 2
    assert len(ids) == 651, "a case was added or removed: update this count with it"


def test_restated_geometry_of_the_named_shapes():
    g = bc.geom
    assert g(4097, 8)["nblk"] == 5 and g(4097, 8)["rows_per_block"] % g(4097, 8)["rpb"] == 0 and 4097 % g(4097, 8)["rows_per_block"] != 0
    assert g(33000, 64)["nblk"] == 258 and bc.finalize_wide(258) and not bc.finalize_wide(256)
    assert g(2100, 1024)["rpb"] == 1 and bc.finalize_wide(g(2100, 1024)["nblk"])
    assert bc.cdiv(16391, g(16391, 1024)["rpb"] * bc.ROWS_PER_THREAD) > bc.BN_MAX_BLOCKS >= g(16391, 1024)["nblk"]
    assert g(300, 7)["threads"] == 252 and g(300, 7)["threads"] % 64 != 0
    assert g(1500, 1023)["threads"] == 1023 and g(257, 4096)["threads"] == 1024
    for (rows, c), _ in bc.NT_SHAPES:
        assert bc.nt_fwd(rows, c) and bc.nt_bwd(rows, c)
    assert 4 * bc.AT_NT_FWD[0] * bc.AT_NT_FWD[1] == bc.NT_BYTES and not bc.nt_fwd(*bc.AT_NT_FWD)
    assert 8 * bc.AT_NT_BWD[0] * bc.AT_NT_BWD[1] == bc.NT_BYTES and not bc.nt_bwd(*bc.AT_NT_BWD)
    # a block's rows times the row stride stay below 2^31 (32-bit element offsets) at every case
    for c in bc.all_cases():
        if "rows" in c and c["kind"] != "narrow":
            gg = g(c["rows"], c["c"])
            assert (gg["rows_per_block"] + (bc.UNROLL + 1) * gg["rpb"]) * max(c.get("ld", 0), c["c"]) < 1 << 31


def test_launch_geometry_stays_within_a_workgroup_for_every_accepted_channel_count():
    """bn_geom asks for cv * rpb threads.  For every 1 <= c <= 4096 and a spread of row counts that is at most 1024, or the entry points
    reject the channel count before launching (launch_limit_ok, checked on the device by test_channel_limits_are_rejected_...); the
    dynamic LDS of the reductions (threads * 2 * vec floats) fits a workgroup's 64 KiB"""
    rejected = []
    for c in range(1, bc.MAX_CHANNELS + 1):
        for rows in ROW_COUNTS:
            g = bc.geom(rows, c)
            fits = g["threads"] <= MAX_THREADS
            assert fits or not bc.launch_limit_ok(c), (rows, c, g["threads"])
            if bc.launch_limit_ok(c):
                assert fits and 4 * g["threads"] * 2 * g["vec"] <= LDS_PER_WORKGROUP and 1 <= g["nblk"] <= bc.BN_MAX_BLOCKS
                assert g["nblk"] * g["rows_per_block"] >= rows > (g["nblk"] - 1) * g["rows_per_block"]
            sg = bc.small_geom(rows, c)
            if sg:
                assert sg["threads"] <= 512 and sg["threads"] % 64 == 0 and sg["rpb"] * bc.ROWS_PER_THREAD >= rows and sg["cvw"] * sg["rpb"] == sg["threads"]
        if not bc.launch_limit_ok(c):
            rejected.append(c)
    assert rejected == [c for c in range(1025, 4097) if c % 4], "exactly the scalar-width channel counts above 1024 are refused"
    for c in bc.all_cases():
        assert all(t <= MAX_THREADS for t in bc.case_threads(c)), bc.case_id(c)
        assert bc.launch_limit_ok(c.get("c", c.get("cin")))


def render(table):
    reach = {}
    for c in bc.all_cases():
        for inst in bc.instantiations(c):
            e = reach.setdefault(inst, [0, 0])
            e[0 if c["family"] == "exact" else 1] += 1
    lines = ["# Kernels and template instantiations of csrc/mlp.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_bn_instantiations_cpu.py`.  Template arguments: `bn_stats_kernel<VEC, ELU, NT>`,",
             "`bn_apply_kernel` / `bn_bwd_reduce_kernel` / `bn_bwd_dx_kernel<VEC, ELU, DROP, NT>`, the pool and narrow kernels `<VEC>`.",
             "The last two columns count the cases of `tests/bn_cases.py` that launch the kernel.", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | scratch bytes | exact cases | rounding cases |",
             "|---|---|---:|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        e = reach.get((name, args), [0, 0])
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d | %d |" % (name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"], f["spill"],
                                                                     f["scratch"], e[0], e[1]))
    lines += ["", "%d kernels, %d cases." % (len(table), len(bc.all_cases()))]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d, "mlp.hip"))))
