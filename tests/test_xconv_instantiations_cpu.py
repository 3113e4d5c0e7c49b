"""Coverage guard of the X-Conv parity suite, on any machine with hipcc: csrc/xconv.hip is compiled to assembly with the Makefile's
flags, and the set of kernels in the code object must equal the set of kernels and template instantiations that the cases of
tests/xconv_cases.py select by the restated dispatch rule.  A new instantiation cannot land without a case, and a case table that stops
reaching one fails here without a GPU.  Only the kernel-metadata table is read (names, LDS, registers, spills, scratch).  Run as a
script, the module prints the table committed as profiles/xconv_instantiations.md."""
import os
import sys
import tempfile

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import xconv_cases as xc  # noqa: E402
from kernel_asm import compile_to_assembly, kernel_table  # noqa: E402


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    return kernel_table(compile_to_assembly(tmp_path_factory.mktemp("xconv_asm"), "xconv.hip"))


def test_every_compiled_kernel_is_selected_by_a_case_and_nothing_else(table):
    compiled = {(name, args) for name, args, _ in table}
    selected = xc.selected_instantiations()
    assert not compiled - selected, "compiled but reached by no case of xconv_cases.py: %s" % sorted(compiled - selected)
    assert not selected - compiled, "the dispatch rule restated in xconv_cases.py names kernels that do not exist: %s" % sorted(selected - compiled)
    assert len(table) == len(compiled)


def test_exact_family_alone_reaches_every_kernel(table):
    """the bit-for-bit family is the one that sees dropped rows, wrong block edges and misrouted channels: it does not lean on the
    rounding family"""
    compiled = {(name, args) for name, args, _ in table}
    exact = xc.selected_instantiations([c for c in xc.all_cases() if c["family"] == "exact"])
    assert compiled == exact, sorted(compiled ^ exact)


def test_the_instantiation_counts_follow_the_dispatch_tables(table):
    count = {}
    for name, _, _ in table:
        count[name] = count.get(name, 0) + 1
    nx, nd = len(xc.XDW_DISPATCH), len(xc.DW_DISPATCH)
    assert count == dict(xconv_apply_kernel=2 * len(xc.APPLY_K), xconv_dx_kernel=len(xc.APPLY_K), depthwise_fwd_kernel=nd, depthwise_dx_kernel=nd,
                         depthwise_narrow_kernel=2 * nd, depthwise_dw_kernel=nd, xconv_dw_fwd_kernel=4 * nx, xconv_dw_bwd_fw_kernel=2 * nx,
                         xconv_dw_bwd_x_kernel=2 * nx, xconv_dw_bwd_fts_kernel=2 * nx)


def render(table):
    reach = {}
    for c in xc.all_cases():
        for inst in xc.instantiations(c):
            e = reach.setdefault(inst, [0, 0])
            e[0 if c["family"] == "exact" else 1] += 1
    lines = ["# Kernels and template instantiations of csrc/xconv.hip", "",
             "Compiled for gfx950 with the Makefile's flags (`-O3 -ffp-contract=off`); produced by",
             "`python tests/test_xconv_instantiations_cpu.py`.  Template arguments: `xconv_apply_kernel<K, TRANSPOSED>`, `xconv_dx_kernel<K>`,",
             "`depthwise_fwd_kernel` / `depthwise_dx_kernel` / `depthwise_dw_kernel<K, M>`, `depthwise_narrow_kernel<K, M, DX>`,",
             "`xconv_dw_fwd_kernel<K, M, GATHER, V2, BN>`, `xconv_dw_bwd_fw_kernel<K, M, GATHER, BN>`, `xconv_dw_bwd_x_kernel<K, M, GATHER>`,",
             "`xconv_dw_bwd_fts_kernel<K, M, VEC>`.  LDS is the static part (`xconv_dx_kernel`, `xconv_dw_bwd_x_kernel` and",
             "`depthwise_dw_kernel` take theirs at launch).  The last two columns count the cases of `tests/xconv_cases.py` that launch the kernel.", "",
             "| kernel | template arguments | LDS bytes | VGPRs | spilled VGPRs | spilled SGPRs | scratch bytes | exact cases | rounding cases |",
             "|---|---|---:|---:|---:|---:|---:|---:|---:|"]
    for name, args, f in table:
        e = reach.get((name, args), [0, 0])
        lines.append("| `%s` | %s | %d | %d | %d | %d | %d | %d | %d |" % (name, ", ".join(str(a).lower() for a in args) or "-", f["lds"], f["vgpr"], f["spill"],
                                                                          f["sgpr_spill"], f["scratch"], e[0], e[1]))
    lines += ["", "%d kernels, %d cases." % (len(table), len(xc.all_cases()))]
    return "\n".join(lines)


if __name__ == "__main__":
    with tempfile.TemporaryDirectory() as d:
        print(render(kernel_table(compile_to_assembly(d, "xconv.hip"))))
