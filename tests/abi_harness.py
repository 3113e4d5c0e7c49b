"""The checking tools of the C-ABI parity tests (tests/test_*_abi.py), one definition each.  A plain module: pytest does not collect
it and does not rewrite its asserts, so every assert carries its own message.

Everything that allocates takes the torch device as its first argument (or an Arena that knows it); nothing here is fixed to "cuda" at
import time.  tests/test_bn_cases_cpu.py and tests/test_gemm_cases_cpu.py run the bodies of the GPU tests on the host by setting DEV of
their ABI sibling to "cpu": the ABI files pass their own DEV, looked up at the call.  tests/test_abi_harness_cpu.py shows on the host
that each checker can fail.

  outputs   Arena.out: a slice of a buffer filled with SENTINEL, GUARD elements either side; check() after the call
            Out / IntOut: such a slice pre-filled with NaN / INT_FILL (an element never written shows); passed=False hands NULL
            Workspace: exactly nbytes between two bands of WS_GUARD bytes of WS_GUARD_BYTE
  inputs    place: at a 16-byte boundary or one float past one, uninitialised padding (NaN only in the gap columns of an ld input)
            In / Hold: between two NaN bands of GUARD elements
  compare   same: bit for bit against fp64 rounded once; within: |got - ref64| <= bound, the worst ratio kept in RATIOS
            same_array: NumPy, equal element for element
  reports   parity_report: the module fixture that writes the RATIOS of its entry points as JSON"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

SENTINEL = 12345.0          # float32 outputs; every other dtype is filled with BYTE_FILL
BYTE_FILL = 0x5a
GUARD = 64                  # elements either side of an output or an input: 256 bytes of float32, keeps the slice's 16-byte alignment
NAN = float("nan")
INT_FILL = -123456789       # the pre-fill of an IntOut
WS_GUARD, WS_GUARD_BYTE = 256, 0xA5
RATIOS = {}                 # (entry point output, family) -> worst |got - ref64| / bound of the session


def abi(unset=()):
    """(_lib, the loaded library); unset: environment variables that the caller's restated launch rule does not model"""
    from heterofusionrcnn_amd import _lib
    for name in unset:
        assert name not in os.environ, "%s is set: the restated launch rule of the cases assumes the library's default" % name
    return _lib, _lib.lib()


def call(status, name):
    _lib, _ = abi()
    _lib.check(status, name)


def _sync(device):
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize()


def _aligned(p, off, what):
    assert p % 16 == (4 if off else 0), "%s sits %d bytes past a 16-byte boundary, not %d" % (what, p % 16, 4 if off else 0)


# ------------------------------------------------------------------------------------------------------- outputs
class Arena:
    """outputs as slices of sentinel-filled buffers; ld > columns: a column slice of wider rows whose other columns must keep the sentinel"""

    def __init__(self, device):
        self.device = device
        self.slots = []

    def out(self, shape, ld=0, init=None, off=False, dtype=torch.float32):
        shape = tuple(shape)
        rows, cols = int(np.prod(shape[:-1], dtype=np.int64)), shape[-1]
        assert not ld or (len(shape) == 2 and ld >= cols), "ld = %d needs a (rows, columns) shape with columns <= ld, got %s" % (ld, shape)
        ld = ld or cols
        start = GUARD + (1 if off else 0)
        buf = torch.full((start + rows * ld + GUARD,), SENTINEL if dtype == torch.float32 else BYTE_FILL, device=self.device, dtype=dtype)
        wide = buf[start:start + rows * ld].view(rows, ld)
        view = wide[:, :cols] if ld > cols else wide.view(shape)
        if init is not None:
            view.copy_(init)
        self.slots.append((buf, start, rows, ld, cols))
        return view

    def check(self):
        _sync(self.device)
        for buf, start, rows, ld, cols in self.slots:
            s = SENTINEL if buf.dtype == torch.float32 else BYTE_FILL
            assert bool((buf[:start] == s).all()) and bool((buf[start + rows * ld:] == s).all()), "write outside an output"
            if ld > cols:
                assert bool((buf[start:start + rows * ld].view(rows, ld)[:, cols:] == s).all()), "write into the gap columns of a strided output"

    def untouched(self):
        """every output still holds the sentinel: nothing was launched"""
        self.check()
        for buf, start, rows, ld, cols in self.slots:
            s = SENTINEL if buf.dtype == torch.float32 else BYTE_FILL
            assert bool((buf == s).all()), "an output was written by a call that must be rejected"


class Out:
    """an output of `n` floats inside a sentinel-filled buffer of the arena, pre-filled with NaN; passed=False: the buffer of a gradient
    that is not asked for (NULL goes to the library) keeps the sentinel everywhere"""

    def __init__(self, arena, n, passed=True, off=False, fill=NAN):
        self.view = arena.out((n,), off=off)
        self.passed = passed
        if passed:
            self.view.fill_(fill)
        self.p = ctypes.c_void_p(self.view.data_ptr()) if passed and n else None
        if passed and n:
            _aligned(self.p.value, off, "an output")


class IntOut:
    """an int32 output of n elements inside a guarded buffer of the arena, pre-filled with INT_FILL"""

    def __init__(self, arena, n, passed=True):
        self.view = arena.out((n,), dtype=torch.int32)
        self.view.fill_(INT_FILL)
        self.p = ctypes.c_void_p(self.view.data_ptr()) if passed and n else None


class Workspace:
    """exactly nbytes between two guards of WS_GUARD bytes, the first byte at a 256-byte boundary"""

    def __init__(self, device, nbytes):
        self.device, self.nbytes = device, int(nbytes)
        raw = torch.full((self.nbytes + 2 * WS_GUARD + 255,), WS_GUARD_BYTE, dtype=torch.uint8, device=device)
        lo = -raw.data_ptr() % 256                      # 0 on the GPU: the allocator's blocks start at 512-byte boundaries
        self.buf = raw[lo:lo + self.nbytes + 2 * WS_GUARD]
        self.p = ctypes.c_void_p(self.buf.data_ptr() + WS_GUARD)

    def check(self, what):
        _sync(self.device)
        assert bool((self.buf[:WS_GUARD] == WS_GUARD_BYTE).all()), "%s: the guard below the workspace was written" % what
        assert bool((self.buf[WS_GUARD + self.nbytes:] == WS_GUARD_BYTE).all()), "%s: the guard above the workspace was written" % what


# ------------------------------------------------------------------------------------------------------- inputs
def place(device, t, off=False, ld=0):
    """the tensor on the device at a 16-byte boundary (off: one float past one); ld: as a column slice of NaN-filled wider rows.  The
    padding after the tensor is uninitialised memory"""
    if t is None:
        return None
    o = 1 if off else 0
    if ld:
        buf = torch.full((t.shape[0] * ld + 8,), NAN, dtype=t.dtype, device=device)
        view = buf[o:o + t.shape[0] * ld].view(t.shape[0], ld)[:, :t.shape[1]]
    else:
        buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=device)
        view = buf[o:o + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == o * t.element_size(), "a placed tensor sits %d bytes past a 16-byte boundary" % (view.data_ptr() % 16)
    return view


class In:
    """an input on the device between two bands of GUARD elements (NaN for floats), 16-byte aligned or (off) one float past that"""

    def __init__(self, device, a, off=False):
        a = np.ascontiguousarray(a)
        start = GUARD + (1 if off else 0)
        if a.dtype == np.float32:
            self.buf = torch.full((start + a.size + GUARD,), NAN, dtype=torch.float32, device=device)
        else:
            assert a.dtype == np.int32, "an input is float32 or int32, not %s" % a.dtype
            self.buf = torch.zeros(start + a.size + GUARD, dtype=torch.int32, device=device)
        if a.size:
            self.buf[start:start + a.size].copy_(torch.from_numpy(a.reshape(-1)))
        self.p = ctypes.c_void_p(self.buf.data_ptr() + 4 * start)
        _aligned(self.p.value, off, "an input")


class Hold:
    """places inputs on the device and keeps them alive until the caller has synchronised; None stays NULL"""

    def __init__(self, device):
        self.device = device
        self.items = []

    def __call__(self, a, off=False):
        if a is None:
            return None
        self.items.append(In(self.device, a, off))
        return self.items[-1].p


def dev64(device, a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def dev(device, a):
    """a copy on the device, C-contiguous: the shared case inputs are read-only"""
    return torch.from_numpy(np.array(a, order="C")).to(device)


def host(t):
    return t.detach().cpu().numpy()


def filled(device, shape, dtype, sent_i):
    """a plain output pre-filled with NaN (floats) or sent_i (integers): none may survive the call"""
    return torch.full(shape, NAN if dtype.is_floating_point else sent_i, dtype=dtype, device=device)


# ------------------------------------------------------------------------------------------------------- comparisons
def same(got, want64, name):
    """bit for bit against the fp64 reference rounded once; a NaN differs"""
    want = want64.float()
    if not torch.equal(got, want):
        bad = (got != want) | torch.isnan(got)
        idx = bad.nonzero()[0].tolist()
        raise AssertionError("%s: %d of %d elements differ from the fp64 reference, first at %s: %r != %r" % (
            name, int(bad.sum()), got.numel(), idx, float(got[tuple(idx)]), float(want[tuple(idx)])))


def within(got, want64, bound, name, family=None):
    """|got - want64| <= bound element for element (the bound broadcasts; a NaN fails; an empty tensor passes); the worst ratio is
    printed and kept in RATIOS[(name, family)]"""
    diff = (got.double() - want64).abs()
    bound = bound.expand_as(diff) if bound.shape != diff.shape else bound
    ratio = float((diff / bound.clamp(min=1e-300)).max()) if diff.numel() else 0.0
    print("%s: max |got - ref64| / bound = %.3g" % (name if family is None else "%s [%s]" % (name, family), ratio))
    RATIOS[(name, family)] = max(RATIOS.get((name, family), 0.0), ratio)
    ok = diff <= bound          # a NaN fails
    assert bool(ok.all()), "%s: %d of %d elements outside the bound, worst ratio %.3g" % (name, int((~ok).sum()), got.numel(), ratio)


def same_array(got, want, what, case, unwritten=None):
    """NumPy: shape, dtype and every element equal.  unwritten: the integer pre-fill of the outputs (floats: NaN), none may survive"""
    got = host(got) if isinstance(got, torch.Tensor) else got
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    if unwritten is not None:
        never = np.isnan(got) if got.dtype.kind == "f" else got == unwritten
        assert not never.any(), "%s of %s: %d elements never written" % (what, case, int(never.sum()))
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError("%s of %s: %d of %d elements differ, the first at %s: got %r, want %r"
                             % (what, case, len(bad), got.size, tuple(bad[0]), got[tuple(bad[0])], want[tuple(bad[0])]))


def bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def same_bits(x, y):
    """NumPy arrays of one shape with the same bits (NaN for NaN, the sign of zero included)"""
    return x.shape == y.shape and np.array_equal(bits(x), bits(y))


def twice(run, *args):
    """every case is called twice: the same bits (the header promises fixed-order reductions).  Tensors by torch.equal, arrays by bits"""
    first, second = run(*args), run(*args)
    for key in first:
        a, b = first[key], second[key]
        if a is not None:
            assert torch.equal(a, b) if isinstance(a, torch.Tensor) else np.array_equal(bits(a), bits(b)), "%s differs between two calls" % key
    return first


# ------------------------------------------------------------------------------------------------------- reports
def write_report(path, prefixes, **extra):
    """the worst ratios of the outputs whose names start with one of `prefixes` as JSON {"name|family": ratio}; with `extra`,
    {"ratios": {...}, **extra}"""
    ratios = {"%s|%s" % k: RATIOS[k] for k in sorted((k for k in RATIOS if k[0].startswith(prefixes)), key=lambda k: (k[0], k[1] or ""))}
    with open(path, "w") as f:
        json.dump(dict(ratios=ratios, **extra) if extra else ratios, f, indent=1)


def parity_report(env_name, prefixes, **extra):
    """the module-scoped autouse fixture of a parity file: with <env_name>=<file> set, write_report at the end of the module"""
    @pytest.fixture(scope="module", autouse=True)
    def report():
        yield
        if os.environ.get(env_name):
            write_report(os.environ[env_name], prefixes, **extra)
    return report
