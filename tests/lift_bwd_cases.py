"""The shapes of tests/test_lift_bwd_onepass_abi.py and the instantiations of csrc/lift_bwd.hip they select, as a plain module:
tests/test_lift_bwd_instantiations_cpu.py compares the set with the compiled one on any machine with hipcc."""
import gemm_cases as gc

MAX_C0 = 128                                   # the entry's limit: NT = ceil(c0 / 32) <= 4 compiles without spills
C0S = (4, 36, 64, 96, 128)                     # 4, 36: partial 32-column groups; 128 = MAX_C0, the largest the entry accepts
C1S = (33, 64, 100, 256)                       # 33: scalar loads
SMALL_ROWS = (1, 129, 300)                     # one row; one full tile plus one row; a ragged third tile


def _shapes():
    out = [(r, c0, c1) for r in SMALL_ROWS + (40000,) for c0 in C0S for c1 in C1S]
    out += [(gc.multi_tile_rows(gc.cdiv(c0, 32)), c0, c1) for c0 in C0S for c1 in C1S]
    return out


CASES = [gc._case("lift_bwd", rows=r, c0=c0, c1=c1, family="round") for r, c0, c1 in _shapes()]
TWINS = [gc._case("lift_bwd", rows=300, c0=36, c1=100, family="exact", misalign=m) for m in ("dz1", "w1_t")]


def instantiations(c):
    """(kernel, template arguments) of lift_bwd.hip that a case launches: NT = ceil(c0 / 32), VEC = c1 % 4 == 0 and dz1, w1_t aligned"""
    vec = c["c1"] % 4 == 0 and c["misalign"] not in ("dz1", "w1_t")
    return {("lift_bwd_onepass_kernel", (gc.cdiv(c["c0"], 32), vec)), ("lift_bwd_onepass_finalize_kernel", ())}


def selected_instantiations():
    out = set()
    for c in CASES + TWINS:
        out |= instantiations(c)
    return out
