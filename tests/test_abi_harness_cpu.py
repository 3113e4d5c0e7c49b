"""The shared checkers of tests/abi_harness.py can fail: each one is shown, on device "cpu", a write or a value it must catch and one it
must let pass.  Smallest shapes that can still go wrong: outputs of 1 and of GUARD + 1 elements (a slot shorter and longer than a guard
band), an ld output of 2 rows, 3 columns, ld 5."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_harness as H  # noqa: E402

DEV = "cpu"
SIZES = (1, H.GUARD + 1)


def slot(arena, index=-1):
    """(the whole buffer, first element of the output) of an output of the arena"""
    buf, start = arena.slots[index][:2]
    return buf, start


# ------------------------------------------------------------------------------------------------------- Arena
@pytest.mark.parametrize("off", (False, True))
@pytest.mark.parametrize("n", SIZES)
def test_arena_catches_a_write_one_element_below_and_one_above_an_output(n, off):
    for where in ("below", "above"):
        a = H.Arena(DEV)
        a.out((3,))                                     # a slot that stays clean beside the one written
        view = a.out((n,), off=off)
        assert view.shape == (n,) and view.data_ptr() % 16 == (4 if off else 0)
        buf, start = slot(a)
        a.check()
        buf[start - 1 if where == "below" else start + n] = 0.0
        with pytest.raises(AssertionError, match="write outside an output"):
            a.check()


@pytest.mark.parametrize("n", SIZES)
def test_arena_passes_a_write_inside_the_output_and_untouched_does_not(n):
    a = H.Arena(DEV)
    view = a.out((n,))
    a.untouched()
    view.fill_(7.0)
    a.check()
    with pytest.raises(AssertionError, match="must be rejected"):
        a.untouched()
    b = H.Arena(DEV)
    b.out((n,))[n - 1] = H.NAN                         # any write: the last element alone
    with pytest.raises(AssertionError, match="must be rejected"):
        b.untouched()


def test_arena_catches_a_write_into_a_gap_column():
    a = H.Arena(DEV)
    view = a.out((2, 3), ld=5)
    assert view.shape == (2, 3) and view.stride() == (5, 1)
    view.fill_(1.0)
    a.check()
    buf, start = slot(a)
    for element in (3, 4, 5 + 3, 5 + 4):                # every gap element of the two rows
        buf[start + element] = 1.0
        with pytest.raises(AssertionError, match="gap columns"):
            a.check()
        buf[start + element] = H.SENTINEL
    a.check()
    buf[start + 2 * 5] = 1.0                            # one past the last row: the guard, not a gap
    with pytest.raises(AssertionError, match="write outside an output"):
        a.check()


def test_arena_forms_agree_where_they_overlap():
    """ld == columns is the dense output; a dtype other than float32 is guarded with its own fill; init lands in the view only"""
    a = H.Arena(DEV)
    dense, strided = a.out((2, 3)), a.out((2, 3), ld=3)
    assert dense.is_contiguous() and strided.is_contiguous() and a.slots[0][1:] == a.slots[1][1:]
    cube = a.out((2, 3, 4), init=torch.arange(24.0).view(2, 3, 4))
    assert cube.shape == (2, 3, 4) and float(cube[1, 2, 3]) == 23.0
    bytes_ = a.out((2, 3), dtype=torch.uint8)
    assert bool((bytes_ == H.BYTE_FILL).all())
    a.check()
    buf, start = slot(a)
    buf[start - 1] = 0
    with pytest.raises(AssertionError, match="write outside an output"):
        a.check()


# ------------------------------------------------------------------------------------------------------- Out, IntOut, In, place
def test_out_not_passed_hands_null_and_keeps_the_sentinel():
    a = H.Arena(DEV)
    asked, skipped, empty = H.Out(a, 5), H.Out(a, 5, passed=False), H.Out(a, 0)
    assert asked.p.value == asked.view.data_ptr() and bool(torch.isnan(asked.view).all())
    assert skipped.p is None and not skipped.passed and bool((skipped.view == H.SENTINEL).all())
    assert empty.p is None
    assert bool((H.Out(a, 5, fill=H.SENTINEL).view == H.SENTINEL).all())
    ints, no_ints = H.IntOut(a, 4), H.IntOut(a, 4, passed=False)
    assert ints.p.value == ints.view.data_ptr() and no_ints.p is None and bool((ints.view == H.INT_FILL).all())
    a.check()


@pytest.mark.parametrize("off", (False, True))
def test_in_sits_between_nan_bands_at_the_alignment_asked_for(off):
    values = np.arange(1, 6, dtype=np.float32)
    x = H.In(DEV, values, off)
    assert x.p.value % 16 == (4 if off else 0)
    first = (x.p.value - x.buf.data_ptr()) // 4
    assert first == H.GUARD + (1 if off else 0)
    assert bool(torch.isnan(x.buf[:first]).all()) and bool(torch.isnan(x.buf[first + 5:]).all()) and x.buf.numel() == first + 5 + H.GUARD
    assert np.array_equal(np.ctypeslib.as_array(ctypes.cast(x.p, ctypes.POINTER(ctypes.c_float)), (5,)), values)
    i = H.In(DEV, np.arange(3, dtype=np.int32))
    assert i.buf.dtype == torch.int32 and i.buf[H.GUARD:H.GUARD + 3].tolist() == [0, 1, 2]
    with pytest.raises(AssertionError, match="float32 or int32"):
        H.In(DEV, np.zeros(3, np.float64))
    hold = H.Hold(DEV)
    assert hold(None) is None and not hold.items
    assert hold(values, off).value % 16 == (4 if off else 0) and len(hold.items) == 1


@pytest.mark.parametrize("off", (False, True))
def test_place_keeps_the_values_and_the_alignment(off):
    t = torch.arange(6.0).view(2, 3)
    dense, wide = H.place(DEV, t, off), H.place(DEV, t, off, ld=5)
    for v in (dense, wide):
        assert torch.equal(v, t) and v.data_ptr() % 16 == (4 if off else 0)
    assert wide.stride() == (5, 1)
    row = torch.as_strided(wide, (2, 5), (5, 1))
    assert bool(torch.isnan(row[:, 3:]).all()), "the gap columns of an ld input hold NaN"
    assert H.place(DEV, None) is None


# ------------------------------------------------------------------------------------------------------- Workspace
@pytest.mark.parametrize("nbytes", (0, 1, 256, 1000))
def test_workspace_names_the_guard_that_was_written(nbytes):
    ws = H.Workspace(DEV, nbytes)
    assert ws.p.value % 256 == 0 and ws.p.value == ws.buf.data_ptr() + H.WS_GUARD and ws.buf.numel() == nbytes + 2 * H.WS_GUARD
    ws.buf[H.WS_GUARD:H.WS_GUARD + nbytes] = 0            # every byte of the workspace itself
    ws.check("inside")
    ws.buf[H.WS_GUARD - 1] = 0
    with pytest.raises(AssertionError, match="lower: the guard below the workspace"):
        ws.check("lower")
    ws.buf[H.WS_GUARD - 1] = H.WS_GUARD_BYTE
    ws.buf[H.WS_GUARD + nbytes] = 0
    with pytest.raises(AssertionError, match="upper: the guard above the workspace"):
        ws.check("upper")


# ------------------------------------------------------------------------------------------------------- same, within
@pytest.mark.parametrize("n", SIZES)
def test_same_raises_on_one_differing_element_and_on_a_nan(n):
    want = torch.arange(n, dtype=torch.float64) + 1.0
    H.same(want.float(), want, "equal")
    got = want.float()
    got[n - 1] = torch.nextafter(got[n - 1], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match=r"one ulp: 1 of %d elements differ from the fp64 reference, first at \[%d\]" % (n, n - 1)):
        H.same(got, want, "one ulp")
    got = want.float()
    got[0] = H.NAN
    with pytest.raises(AssertionError, match=r"a NaN: 1 of %d elements differ" % n):
        H.same(got, want, "a NaN")
    with pytest.raises(AssertionError):
        H.same(torch.tensor([H.NAN]), torch.tensor([H.NAN], dtype=torch.float64), "NaN against NaN")


@pytest.fixture
def ratios():
    before = dict(H.RATIOS)
    yield H.RATIOS
    H.RATIOS.clear()
    H.RATIOS.update(before)


def test_within_at_the_bound_just_over_it_on_a_nan_and_on_nothing(ratios, capsys):
    want = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    bound = torch.tensor([0.5, 0.25, 0.125], dtype=torch.float64)
    at = (want + bound).float()                                    # exactly representable: the difference IS the bound
    H.within(at, want, bound, "at the bound")
    assert ratios[("at the bound", None)] == 1.0
    assert capsys.readouterr().out == "at the bound: max |got - ref64| / bound = 1\n"
    over = at.clone()
    over[2] = torch.nextafter(over[2], torch.tensor(float("inf")))
    with pytest.raises(AssertionError, match="just over: 1 of 3 elements outside the bound"):
        H.within(over, want, bound, "just over", "round")
    assert 1.0 < ratios[("just over", "round")] < 1.0 + 1e-5       # recorded before the assertion
    assert capsys.readouterr().out.startswith("just over [round]: max |got - ref64| / bound = ")
    nan = at.clone()
    nan[1] = H.NAN
    with pytest.raises(AssertionError, match="a NaN: 1 of 3 elements outside the bound"):
        H.within(nan, want, bound, "a NaN")
    empty = torch.zeros((0, 4))
    H.within(empty, empty.double(), torch.zeros((0, 4), dtype=torch.float64), "nothing")
    assert ratios[("nothing", None)] == 0.0


def test_within_broadcasts_the_bound_and_keeps_the_worst_ratio(ratios):
    want = torch.zeros((2, 3), dtype=torch.float64)
    got = torch.tensor([[0.0, 0.25, 0.0], [0.5, 0.0, 0.0]])
    H.within(got, want, torch.tensor(1.0, dtype=torch.float64), "hf_x.y", "round")             # a scalar bound
    H.within(got * 0.5, want, torch.ones(3, dtype=torch.float64), "hf_x.y", "round")           # a row, and a smaller ratio: the worst stays
    assert ratios[("hf_x.y", "round")] == 0.5
    with pytest.raises(AssertionError, match="hf_x.y: 1 of 6 elements outside the bound, worst ratio 1.25"):
        H.within(got, want, torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64) * 0.4, "hf_x.y", "round")
    assert ratios[("hf_x.y", "round")] == 1.25


def test_same_array_and_the_unwritten_fill():
    want = np.arange(6, dtype=np.int32).reshape(2, 3)
    H.same_array(torch.from_numpy(want.copy()), want, "ints", "case")
    got = want.copy()
    got[1, 2] = -7
    with pytest.raises(AssertionError, match="ints of case: 1 of 6 elements differ, the first at .*1.*2.*got .*-7.*want .*5"):
        H.same_array(got, want, "ints", "case")
    with pytest.raises(AssertionError, match="ints of case: 1 elements never written"):
        H.same_array(got, want, "ints", "case", unwritten=-7)
    with pytest.raises(AssertionError, match="floats of case: 2 elements never written"):
        H.same_array(np.array([1.0, H.NAN, H.NAN], np.float32), np.ones(3, np.float32), "floats", "case", unwritten=-7)
    with pytest.raises(AssertionError):
        H.same_array(want.astype(np.int64), want, "dtype", "case")


def test_twice_and_the_bit_comparisons():
    steady = lambda x: dict(a=torch.tensor([x]), b=None, c=np.array([x], np.float32))
    assert set(H.twice(steady, 1.0)) == {"a", "b", "c"}
    counter = iter(range(2))
    with pytest.raises(AssertionError, match="a differs between two calls"):
        H.twice(lambda: dict(a=torch.tensor([float(next(counter))])))
    signs = iter((1.0, -1.0))
    with pytest.raises(AssertionError, match="c differs between two calls"):
        H.twice(lambda: dict(c=np.array([next(signs) * 0.0], np.float32)))          # arrays by their bits: the sign of zero counts
    zero, minus, nan = np.zeros(2, np.float32), -np.zeros(2, np.float32), np.full(2, np.nan, np.float32)
    assert H.same_bits(zero, zero.copy()) and H.same_bits(nan, nan.copy())
    assert not H.same_bits(zero, minus) and not H.same_bits(zero, np.zeros(3, np.float32))


# ------------------------------------------------------------------------------------------------------- parity_report
def test_report_filters_by_prefix_and_keeps_the_json_shapes(ratios, tmp_path):
    ratios.clear()
    ratios.update({("hf_a.y", "round"): 0.5, ("hf_a.x", "round"): 0.25, ("hf_b.y", "case"): 0.75, ("z", None): 2.0})
    path = str(tmp_path / "report.json")
    plain = {"hf_a.x|round": 0.25, "hf_a.y|round": 0.5}
    for extra, want in (({}, plain), (dict(elu={"ratio": 1.5}), {"ratios": plain, "elu": {"ratio": 1.5}})):
        H.write_report(path, ("hf_a",), **extra)
        with open(path) as f:
            got = json.load(f)
        assert got == want and list(got.get("ratios", got)) == sorted(plain)
