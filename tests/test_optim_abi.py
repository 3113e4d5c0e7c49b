"""Kernel-level parity of csrc/optim.hip through the C ABI: hf_adam_sqnorm_partials, hf_adam_multi, hf_adam_multi_sched and hf_copy_multi
at every launch regime (the case table, the restated launch rule, the fp64 reference and its derived bound are in tests/optim_cases.py),
ctypes on _lib.lib() with no Python routing: the hf_adam_entry table and the chunk map are built here by hand.

p, m and v of every tensor are slices of sentinel-filled buffers at a 16-byte boundary or one float past it; g is placed at 0, 4, 8 or 12
bytes past one (8 and 12: a slice of a flat buffer, the layout of graph_step.FlatGrads); the step counter is a one-element tensor set to t.
After the call: no write outside an output, g, the table, the map and the counter keep their bits, partial rows beyond num_chunks keep their
pre-fill; p', m', v' and the partials lie within the bound of the fp64 reference, m' and v' of the exact family equal it bit for bit.  With
clipping off the partials go in as NULL.  Every call is made twice from the same state and must give the same bits.

`python tests/test_optim_abi.py report.json` renders the report of OPTIM_PARITY_OUT=report.json as the tables of profiles/optim_parity.md."""
import ctypes
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_cases as oc  # noqa: E402
from abi_harness import BYTE_FILL, Arena, abi, call, dev, parity_report, place, same, twice, within  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
parity_report = parity_report("OPTIM_PARITY_OUT", ("hf_adam", "hf_copy_multi"))      # the source of profiles/optim_parity.md


class Entry(ctypes.Structure):          # hf_adam_entry (include/hfops.h)
    _fields_ = [("p", ctypes.c_void_p), ("g", ctypes.c_void_p), ("m", ctypes.c_void_p), ("v", ctypes.c_void_p), ("n", ctypes.c_longlong)]


def tt(a):
    """a tensor that owns a copy: the shared case inputs are read-only"""
    return torch.from_numpy(np.array(a, order="C"))


def put_g(g, off):
    """the gradient `off` floats past a 16-byte boundary; 2 and 3: a slice of a flat buffer"""
    t = tt(g)
    if off < 2:
        return place(DEV, t, off=bool(off))
    flat = torch.empty(g.size + 8, dtype=torch.float32, device=DEV)
    view = flat[off:off + g.size]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off
    return view


def bits(t):
    return t.contiguous().view(torch.int32)


def run(c, d, entry=None):
    _lib, L = abi()
    entry = entry or c["entry"]
    a, idx = Arena(DEV), oc.live(c)
    P, G, M, V = [], [], [], []
    for i in idx:
        x = c["tensors"][i]
        for lst, key, off in ((P, "p", x["off"][0]), (M, "m", x["off"][2]), (V, "v", x["off"][3])):
            lst.append(a.out((x["n"],), init=tt(d[key][i]), off=bool(off)))
            assert lst[-1].data_ptr() % 16 == 4 * off
        G.append(put_g(d["g"][i], x["off"][1]))
    table = (Entry * len(idx))(*[Entry(P[k].data_ptr(), G[k].data_ptr(), M[k].data_ptr(), V[k].data_ptr(), P[k].numel()) for k in range(len(idx))])
    raw = np.frombuffer(bytes(table), np.uint8).copy()
    rows = np.array(oc.map_rows(c), np.int32).reshape(-1, 2)
    dev_table, dev_map = dev(DEV, raw), dev(DEV, rows)
    step = torch.tensor([float(c["t"])], dtype=torch.float32, device=DEV)
    n, part, stream = len(rows), None, _lib.stream_ptr()
    if c["clip"] > 0:
        part = a.out((n + 3,), dtype=torch.float64)
        part.fill_(oc.PARTIAL_FILL)
        call(L.hf_adam_sqnorm_partials(n, _lib.ptr(dev_table), _lib.ptr(dev_map), c["scale"], _lib.ptr(part), stream), "hf_adam_sqnorm_partials")
    if entry == "multi":
        assert c["clip"] == 0 and c["sched"] == oc.SCHED_CONST
        call(L.hf_adam_multi(n, _lib.ptr(dev_table), _lib.ptr(dev_map), _lib.ptr(step), c["lr"], c["b1"], c["b2"], c["eps"], c["scale"], c["mode"], stream),
             "hf_adam_multi")
    else:
        call(L.hf_adam_multi_sched(n, _lib.ptr(dev_table), _lib.ptr(dev_map), _lib.ptr(step), _lib.ptr(part), c["clip"], c["lr"], c["sched"], c["dsteps"],
                                   c["dfactor"], c["b1"], c["b2"], c["eps"], c["scale"], c["mode"], stream), "hf_adam_multi_sched")
    a.check()
    for k, i in enumerate(idx):
        assert torch.equal(bits(G[k]), bits(tt(d["g"][i]).to(DEV))), "the gradient of tensor %d changed" % i
    assert torch.equal(dev_table.cpu(), torch.from_numpy(raw)) and torch.equal(dev_map.cpu(), torch.from_numpy(rows)), "the table or the map changed"
    assert float(step[0]) == float(c["t"]), "the step counter changed"
    out = dict(partials=None if part is None else part.clone())
    for k in range(len(idx)):
        out.update({"p%d" % k: P[k].clone(), "m%d" % k: M[k].clone(), "v%d" % k: V[k].clone()})
    return out


def check(c, d, got):
    t64 = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    for k, r in enumerate(oc.reference(c, d)):
        for name in "pmv":
            val, bound = r[name]
            g = got["%s%d" % (name, k)].cpu()
            if c["exact"] and name in "mv":
                same(g, t64(val), "hf_adam.%s of tensor %d of %s" % (name, k, c["name"]))
            else:
                within(g, t64(val), t64(bound), "hf_adam." + name, c["family"])
    if c["clip"] > 0:
        S, B = oc.reference_partials(c, d)
        part = got["partials"].cpu()
        within(part[:len(S)], t64(S), t64(B), "hf_adam.partials", c["family"])
        assert bool((part[len(S):] == oc.PARTIAL_FILL).all()), "a partial row beyond num_chunks was written"
    else:
        assert got["partials"] is None


@pytest.mark.parametrize("c", oc.all_cases(), ids=oc.case_id)
def test_adam_update(c):
    d = oc.inputs(c)
    check(c, d, twice(run, c, d))


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", ["alignment-g12-t=1000", "alignment-mixed-t=2", "alignment-p4-t=2", "exact-scalar-t=5"])
def test_sched_entry_with_everything_off_is_adam_multi_bit_for_bit_on_the_scalar_path(name, mode):
    base = [c for c in oc.all_cases() if c["name"] == name]
    assert len(base) == 1 and ("update", "scalar") in oc.regimes_of(base[0])
    c = dict(base[0], clip=0.0, sched=oc.SCHED_CONST, mode=mode)
    d = oc.inputs(c)
    one, two = run(c, d, "multi"), run(c, d, "sched")
    for key in one:
        if key != "partials":
            assert torch.equal(bits(one[key]), bits(two[key])), "%s differs between hf_adam_multi and hf_adam_multi_sched" % key
    check(c, d, one)


# ------------------------------------------------------------------------------------------------- hf_copy_multi
def run_copy(c):
    _lib, L = abi()
    a, n = Arena(DEV), len(c["entries"])
    dst, src, nbytes, views, keep = [], [], [], [], []
    for i, (b, do, so) in enumerate(c["entries"]):
        if b < 0:                                        # a zero-byte copy with NULL on both sides
            dst.append(None), src.append(None), nbytes.append(0), views.append(None)
            continue
        view = a.out((max(b, 16),), dtype=torch.uint8, off=bool(do))
        sbuf = torch.full((b + 48,), 0xC3, dtype=torch.uint8, device=DEV)
        s = sbuf[16 + so:16 + so + b]
        s.copy_(torch.from_numpy(oc.copy_source(c, i)))
        sp = sbuf.data_ptr() + 16 + so                   # not s.data_ptr(): an empty slice has none
        assert view.data_ptr() % 16 == do and sp % 16 == so
        dst.append(view.data_ptr()), src.append(sp), nbytes.append(b), views.append(view), keep.append(sbuf)
    call(L.hf_copy_multi(n, (ctypes.c_void_p * n)(*dst), (ctypes.c_void_p * n)(*src), (ctypes.c_longlong * n)(*nbytes), _lib.stream_ptr()), "hf_copy_multi")
    a.check()                                            # every guard byte
    return {"dst%d" % i: None if v is None else v.clone() for i, v in enumerate(views)}


@pytest.mark.parametrize("c", oc.COPY_CASES, ids=lambda c: c["name"])
def test_copy_multi(c):
    got = twice(run_copy, c)
    for i, (b, _, _) in enumerate(c["entries"]):
        if b < 0:
            continue
        g = got["dst%d" % i].cpu().numpy()
        want = oc.copy_source(c, i)
        assert np.array_equal(g[:b], want), "copy %d of %s: %d of %d bytes differ" % (i, c["name"], int((g[:b] != want).sum()), b)
        assert (g[b:] == BYTE_FILL).all(), "copy %d of %s wrote past its %d bytes" % (i, c["name"], b)


def test_copy_multi_refuses_65_copies_and_launches_nothing():
    _lib, L = abi()
    a, n = Arena(DEV), oc.COPY_MAX + 1
    assert L.hf_copy_multi_max() == oc.COPY_MAX
    views = [a.out((16,), dtype=torch.uint8) for _ in range(n)]
    srcs = [torch.zeros(16, dtype=torch.uint8, device=DEV) for _ in range(n)]
    status = L.hf_copy_multi(n, (ctypes.c_void_p * n)(*[v.data_ptr() for v in views]), (ctypes.c_void_p * n)(*[s.data_ptr() for s in srcs]),
                             (ctypes.c_longlong * n)(*[16] * n), _lib.stream_ptr())
    assert status == _lib.HF_EINVAL
    a.untouched()


# ------------------------------------------------------------------------------------------------- the report as markdown
def render(path):
    with open(path) as f:
        ratios = json.load(f)
    lines = ["| output | family | worst ratio | |", "|---|---|---:|---|"]
    for key in sorted(ratios):
        name, family = key.split("|")
        lines.append("| `%s` | %s | %.3g | %s |" % (name, family, ratios[key], "**> 1**" if ratios[key] > 1 else "**>= 0.5**" if ratios[key] >= 0.5 else ""))
    return "\n".join(lines)


if __name__ == "__main__":
    print(render(sys.argv[1]))
