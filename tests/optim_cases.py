"""Case table, restated launch rule, fp64 reference with a running error bound, and a NumPy-fp32 restatement of the three kernels of
csrc/optim.hip: adam_sqnorm_partials_kernel (hf_adam_sqnorm_partials), adam_multi_kernel<kClip, kSched> (hf_adam_multi,
hf_adam_multi_sched) and copy_multi_kernel (hf_copy_multi).  tests/test_optim_abi.py runs the cases on the GPU through the C ABI,
tests/test_optim_cases_cpu.py checks this module on any machine (the reference against torch.optim.Adam and against TensorFlow's formula,
the restatement inside the bound, six planted errors outside it, every regime below reached).  A plain helper module: nothing here
imports the library, nothing is measured and nothing is tuned to the device.

Launch rule, restated from optim.hip (the constants are pinned against its text by test_optim_cases_cpu.py):
  table     one hf_adam_entry (p, g, m, v, n) per LIVE tensor (a tensor without a gradient has no entry), one map row (tensor, chunk) per
            CHUNK = 16384 elements, a tensor's rows consecutive; one workgroup of 256 threads per row
  norm      adam_sqnorm_partials_kernel: partials[row] = sum over the chunk of (double) fl(g * grad_scale)^2.  float4 loads iff g + chunk
            start is 16-byte aligned: n4 = n >> 2 vectors in trips of 256, then the n & 3 tail elements; else element by element
  update    adam_multi_kernel: float4 iff p, g, m AND v are 16-byte aligned at the chunk start, same trips and tail; else element by
            element.  kClip (clip_norm > 0): the norm is the sum of partials[row - chunk .. + ceil(n / CHUNK)) in row order.
            kSched 0 / 1 / 2: lr, lr * factor^q, lr * factor^floor(q), q = (t - 1) / decay_steps.  mode 0 / 1: where epsilon stands
  copy      copy_multi_kernel: one workgroup per COPY_CHUNK = 65536 bytes of some copy; first[i] = prefix sum of the chunk counts,
            first[n .. 64] = all; six steps of binary search find the largest i with first[i] <= block (a zero-byte copy owns no block);
            16-byte vectors iff dst and src of the copy are both 16-byte aligned: n16 = bytes >> 4 in trips of 256, then the byte tail

Regimes and the case family that takes each (regimes_of() / copy_regimes_of() compute them from a case; the CPU file asserts all are hit):
  update al, float4 trip count 0 / partial / exactly one full (1024) / several, tail / no tail     lengths (1, 3, 4, 1023, 1024, 1027, ...)
  update scalar path, one pointer off: p / g / m / v by 4 bytes, g by 8 and by 12 bytes            alignment
  update al differs between the tensors of one table                                              alignment (mixed)
  norm float4 / scalar (g aligned / g off), tail / no tail                                         alignment, lengths (clip on)
  chunk length full / short last chunk / one element, chunk > 0                                   lengths (16383 .. 40000)
  row range: first != 0, rows > 1, neighbours at 100 x and 0.5 x clip, a dropped entry            tables
  clip: norm / clip 0, 0.5, exactly 1, 1.001, 50; clip 1.0 and 0.7                                clipping
  each (kClip, kSched, mode) on the float4 and on the scalar path                                 instantiations
  staircase and smooth at global steps 0, 1, 19999, 20000, 20001, 39999, 40000, 239999; (3, .5)   schedule
  grad_scale 1, 0.125, 1 / 3                                                                      grad_scale
  indexing, bit for bit (m', v')                                                                   exact
  copy: which = 0 .. 63 (n = 64: every outcome of the six steps), n = 1, 2, 63; vector / byte path; n16 trips 0 / partial / full /
        several (16 x 256 = one 64 KB chunk); byte tail; zero bytes first / middle / last; one long copy among short ones
Every family that checks p' runs at a small t and at a t with b^t / (1 - b^t) <= 1 for both betas (t >= 700 for 0.999): there the powf
allowance is a few u; at small t the parameter bound is honestly looser (1 - b^t is small and inherits powf's absolute error).

The fp64 reference and its bound.  Inputs: fp32 p, g, m, v, the integer t, the hyper-parameters as fp32 values widened to fp64.  Every
quantity is a pair (value in fp64, e): e bounds |kernel's fp32 value - value| to first order, u = 2^-24, and is carried through the
kernel's own operations.  One rounding u |result| is charged for EACH fp32 operation the kernel performs (the Makefile has
-ffp-contract=off and no fast-math flag: no FMA, `/` and sqrtf correctly rounded), counted here per operation:
  x = g * grad_scale                                   1 (mul)
  norm pass + row sum: fl(g * grad_scale)^2 summed     2 u S from the rounded x (first order), (n + rows) 2^-53 S from the fp64 sums
  clip_den = fmaxf(sqrtf((float) s), clip)             1 (cast) + 1 (sqrtf); fmaxf is 1-Lipschitz: e passes, and is 0 when the norm is
                                                       below clip by more than e
  y = (x * clip) / clip_den                            1 (mul) + 1 (div)
  m' = b1 * m + (1 - b1) * y                           1 (mul) + 1 (sub) + 1 (mul) + 1 (add)
  v' = b2 * v + (1 - b2) * y * y                       1 (mul) + 1 (sub) + 2 (mul, mul) + 1 (add)
  q = (t - 1) / decay_steps                            0 (t - 1 is exact below 2^24) + 1 (div); floorf: 0 (the case list asserts that the
                                                       fp32 floor is the integer floor, else the case would be ill-posed)
  lr * powf(factor, q)                                 powf + 1 (mul)
  bc = 1 - powf(b, t)                                  powf + 1 (sub), for b1 and b2
  sq2 = sqrtf(bc2); inv_sq2 = 1 / sq2                  1 (sqrtf); 1 (div)
  a = lr * sq2 / bc1 (mode 0), lr / bc1 (mode 1)       1 (mul) + 1 (div); 1 (div)
  d = sqrtf(v') + eps; sqrtf(v') * inv_sq2 + eps       1 (sqrtf) + 1 (add); 1 (sqrtf) + 1 (mul) + 1 (add)
  p' = p - a * m' / d                                  1 (mul) + 1 (div) + 1 (sub)
sqrtf of (value, e) is charged value^.5 - max(value - e, 0)^.5 (the larger side, finite at value = 0) instead of e / (2 value^.5).
powf is charged POW_ULP = 16 ulp of its result (an ulp of r is 2^(floor(log2 r) - 23)): OpenCL's bound for pow.  Neither the project nor
the ROCm device library documents a tighter one for powf, so none is assumed; the allowance is propagated through 1 - b^t and, with the
error of q, through |q ln factor|.  The ASSERTED bound is twice e: first order, doubled.  It is derived, not fitted: the ratios the
MI355X reaches are in profiles/optim_parity.md and do not feed back into this file.
Partials: the reference squares fl(g * grad_scale) (an fp32 product, unambiguous) exactly and sums with math.fsum; the bound is
(elements of the chunk) * 2^-53 * S: the squares are exact in fp64, only the additions round.

The exact family: b1 = 0.5, b2 = 0.75, grad_scale = 0.25, no clipping, integer g, m, v that encode (tensor, position): m' = m / 2 + g / 8
and v' = 3 v / 4 + g^2 / 64 are exact fp32 numbers (exact_grid_ok asserts every intermediate below 2^24 in units of its grid) and are
compared bit for bit: a tail element updated from its neighbour or a chunk that reads another tensor's row shows at any tolerance."""
import math
import zlib

import numpy as np

# ---------------------------------------------------------------------------------------------- constants of the source
CHUNK = 16384            # optim.hip kAdamChunk
THREADS = 256            # optim.hip kAdamThreads, kCopyThreads
COPY_MAX = 64            # optim.hip kCopyMax
COPY_CHUNK = 64 * 1024   # optim.hip kCopyChunk
SCHED_CONST, SCHED_EXP, SCHED_STAIR = 0, 1, 2          # optim.hip AdamSched == the `decay` argument
# text that must stand in optim.hip: the rules restated above
SOURCE_RULES = (
    "constexpr int kAdamChunk = 16384;", "constexpr int kAdamThreads = 256;", "constexpr int kCopyMax = 64;",
    "constexpr int kCopyChunk = 64 * 1024;", "constexpr int kCopyThreads = 256;",
    "enum AdamSched { kSchedConst = 0, kSchedExp = 1, kSchedStaircase = 2 };",
    "if ((reinterpret_cast<uintptr_t>(e.g + o0) & 15) == 0) {",
    "const bool al = ((reinterpret_cast<uintptr_t>(e.p + o0) | reinterpret_cast<uintptr_t>(e.g + o0) | reinterpret_cast<uintptr_t>(e.m + o0) |",
    "const int first = static_cast<int>(blockIdx.x) - where.y;",
    "const int rows = static_cast<int>((e.n + kAdamChunk - 1) / kAdamChunk);",
    "float q = (t - 1.0f) / decay_steps;", "if (kSched == kSchedStaircase) q = floorf(q);", "lr = lr * powf(decay_factor, q);",
    "clip_den = fmaxf(sqrtf(static_cast<float>(s)), clip_norm);", "if (kClip) gg = (gg * clip_norm) / clip_den;",
    "mm = b1 * mm + (1.0f - b1) * gg;", "vv = b2 * vv + (1.0f - b2) * gg * gg;",
    "const float d = mode == 0 ? sqrtf(vv) + eps : sqrtf(vv) * inv_sq2 + eps;", "pp -= a * mm / d;",
    "const float a = mode == 0 ? lr * sq2 / bc1 : lr / bc1;",
    "for (int step = 0; step < 6; ++step) {",
    "if (((reinterpret_cast<uintptr_t>(list.dst[which]) | reinterpret_cast<uintptr_t>(list.src[which])) & 15) == 0) {",
)

U = 2.0 ** -24
POW_ULP = 16
FACTOR = 2.0             # the asserted bound is FACTOR times the first-order bound
PARTIAL_FILL = -7.0      # the pre-fill of the partial rows: rows beyond num_chunks keep it

PLANTS = ("nofloor", "t_for_tm1", "extra_row", "drop_tail", "other_prefactor", "eps_under_root")
PLANT_FAMILY = {"nofloor": "schedule", "t_for_tm1": "schedule", "extra_row": "tables", "drop_tail": "lengths", "other_prefactor": "instantiations",
                "eps_under_root": "instantiations"}

A0, OFF_P, OFF_G, OFF_M, OFF_V, OFF_G8, OFF_G12 = (0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (0, 0, 1, 0), (0, 0, 0, 1), (0, 2, 0, 0), (0, 3, 0, 0)
OFFSETS = dict(aligned=A0, p4=OFF_P, g4=OFF_G, m4=OFF_M, v4=OFF_V, g8=OFF_G8, g12=OFF_G12)       # floats past a 16-byte boundary: p, g, m, v
LENGTHS = (1, 3, 4, 1023, 1024, 1027, 16383, 16384, 16385, 32768, 40000)
REF_DECAY = (20000.0, 0.8)                                                                      # rpn_multiclass.config / rcnn_multiclass.config
REF_STEPS = (0, 1, 19999, 20000, 20001, 39999, 40000, 239999)
SMALL_T, LARGE_T = 2, 1000


# ---------------------------------------------------------------------------------------------- the cases
def T(n, off=A0, gs=1.0, norm=None):
    """a tensor of a table: n elements; off: floats past a 16-byte boundary of p, g, m, v; gs: the scale of its random gradient;
    norm: instead, the L2 norm of its averaged gradient in units of clip (a number, or "one": a single element equal to clip / grad_scale)"""
    return dict(n=n, off=tuple(off), gs=gs, norm=norm)


def _case(family, name, tensors, t, mode=0, clip=0.0, sched=SCHED_CONST, decay=(1.0, 1.0), scale=1.0, drop=None, exact=False, entry="sched",
          lr=1e-2, b1=0.9, b2=0.999, eps=1e-8):
    f = lambda x: float(np.float32(x))
    return dict(family=family, name="%s-%s-t=%d" % (family, name, t), tensors=tensors, t=int(t), mode=mode, clip=f(clip), sched=sched,
                dsteps=f(decay[0]), dfactor=f(decay[1]), scale=f(scale), drop=drop, exact=exact, entry=entry, lr=f(lr), b1=f(b1), b2=f(b2), eps=f(eps))


def _build():
    out = []
    both = (SMALL_T, LARGE_T)
    # alignment: the reference's train op (clip, mode 0); the norm pass sees g aligned and g off
    for t in both:
        for name, off in OFFSETS.items():
            out.append(_case("alignment", name, [T(1027, off), T(7, off, gs=0.1)], t, clip=1.0))
        out.append(_case("alignment", "mixed", [T(1027, A0), T(1027, OFF_G8), T(260, A0), T(5, OFF_G12)], t, clip=1.0))
    # lengths: every trip count and tail of the float4 path, chunk edges; norms alternate below / above clip
    for t, ns in ((SMALL_T, LENGTHS[:6]), (LARGE_T, LENGTHS)):
        out.append(_case("lengths", "all", [T(n, gs=(0.5 if i % 2 else 3.0) / math.sqrt(n)) for i, n in enumerate(ns)], t, clip=1.0))
    # tables: seven tensors, a two-chunk tensor (1.2 x clip: a row too few -> 0.85, unclipped) between 100 x clip and 0.5 x clip
    seven = [T(5, norm=3.0), T(1027, norm=100.0), T(16390, norm=1.2), T(515, norm=0.5), T(260, norm=3.0), T(4, norm=0.0), T(1023, norm=1.001)]
    out.append(_case("tables", "seven", seven, LARGE_T, clip=1.0, scale=0.25))
    out.append(_case("tables", "dropped", seven, LARGE_T, clip=1.0, scale=0.25, drop=1))
    out.append(_case("tables", "seven-g12", [dict(x, off=OFF_G12) for x in seven], SMALL_T, clip=1.0, scale=0.25))
    # clipping
    for t in both:
        for clip in (1.0, 0.7):
            out.append(_case("clipping", "clip=%g" % clip, [T(260, norm=0.0), T(1027, norm=0.5), T(1027, norm="one"), T(1027, norm=1.001), T(1027, norm=50.0)],
                             t, clip=clip, scale=0.125))
    # instantiations: (kClip, kSched, mode) x path; gradient scales 1e-3 .. 300; decay (300, 0.5): q = 3.33 at t = 1000
    for t in (3, LARGE_T):
        for kclip in (0, 1):
            for sched in (SCHED_CONST, SCHED_EXP, SCHED_STAIR):
                for mode in (0, 1):
                    for path, off in (("vec", A0), ("scalar", OFF_G12)):
                        out.append(_case("instantiations", "clip=%d-sched=%d-mode=%d-%s" % (kclip, sched, mode, path),
                                         [T(515, off, gs=1e-3), T(5, off, gs=300.0), T(260, off)], t, mode=mode, clip=float(kclip), sched=sched,
                                         decay=(300.0, 0.5), lr=1e-3))
    # schedule: the reference's (20000, 0.8) at its boundaries, the step counter set directly; paths alternate
    for sched, sname in ((SCHED_STAIR, "staircase"), (SCHED_EXP, "smooth")):
        for decay, steps in ((REF_DECAY, REF_STEPS), ((3.0, 0.5), (2, 3, 9))):
            for i, gstep in enumerate(steps):
                off = OFF_G8 if i % 2 else A0
                out.append(_case("schedule", "%s-%gx%g-%s" % (sname, decay[0], decay[1], "scalar" if i % 2 else "vec"), [T(515, off), T(5, off)], gstep + 1,
                                 clip=1.0, sched=sched, decay=decay, lr=1e-3))
    # grad_scale
    for t in both:
        for scale, sname in ((1.0, "1"), (0.125, "0.125"), (1.0 / 3.0, "third")):
            for mode in (0, 1):
                out.append(_case("grad_scale", "scale=%s-mode=%d" % (sname, mode), [T(515, gs=0.05), T(7, OFF_G, gs=30.0)], t, mode=mode, clip=0.7, scale=scale))
    # exact: indexing bit for bit, through hf_adam_multi (the entry the plain train step calls)
    ex = dict(scale=0.25, b1=0.5, b2=0.75, exact=True, entry="multi")
    for t in (1, 5):
        for mode in (0, 1):
            out.append(_case("exact", "vec-mode=%d" % mode, [T(n) for n in (1, 3, 1027) + ((16385,) if (t, mode) == (5, 0) else ()) + (5, 1024)], t, mode=mode, **ex))
    out.append(_case("exact", "scalar", [T(n, OFF_G12) for n in (1, 3, 1027, 5)] + [T(1029, OFF_M)], 5, **ex))
    out.append(_case("exact", "mixed", [T(1027, A0), T(1027, OFF_P), T(6, OFF_V), T(1024, A0)], 5, **ex))
    return out


_CASES = None


def all_cases():
    global _CASES
    if _CASES is None:
        _CASES = _build()
    return _CASES


def cases_of(family):
    return [c for c in all_cases() if c["family"] == family]


def case_id(c):
    return c["name"]


def live(c):
    """the indices of the tensors that have a table entry"""
    return [i for i in range(len(c["tensors"])) if i != c["drop"]]


def map_rows(c):
    """the chunk map: (entry, chunk) per row"""
    return [(k, ch) for k, i in enumerate(live(c)) for ch in range((c["tensors"][i]["n"] + CHUNK - 1) // CHUNK)]


def elements(c):
    return sum(c["tensors"][i]["n"] for i in live(c))


def sched_q(c):
    """q in fp32 as the kernel computes it, and in exact arithmetic"""
    q32 = (np.float32(c["t"]) - np.float32(1)) / np.float32(c["dsteps"])
    q = (c["t"] - 1) / c["dsteps"]
    if c["sched"] == SCHED_STAIR:
        q32, q = np.floor(q32), math.floor(q)
    return float(q32), float(q)


def regimes_of(c):
    """the branches of the two Adam kernels that the case takes, from the case alone"""
    seen = {("inst", int(c["clip"] > 0), c["sched"], c["mode"]), ("entry", c["entry"])}
    als = set()
    for (k, ch), i in ((r, live(c)[r[0]]) for r in map_rows(c)):
        x = c["tensors"][i]
        n = min(CHUNK, x["n"] - ch * CHUNK)
        al = all(o == 0 for o in x["off"])
        als.add(al)
        if al:
            n4 = n >> 2
            trips = "none" if n4 == 0 else "partial" if n4 < THREADS else "one" if n4 == THREADS else "several"
            seen |= {("update", "vec"), ("update-trips", trips), ("update-tail", bool(n & 3))}
        else:
            seen |= {("update", "scalar"), ("update-off", x["off"])}
        seen.add(("inst-path", int(c["clip"] > 0), c["sched"], c["mode"], "vec" if al else "scalar"))
        seen.add(("chunk", "full" if n == CHUNK else "one" if n == 1 else "short"))
        if ch > 0:
            seen.add(("chunk", "later"))
        if c["clip"] > 0:
            seen |= {("norm", "vec" if x["off"][1] == 0 else "scalar"), ("rows", "first>0" if k > 0 else "first=0"),
                     ("rows", "several" if x["n"] > CHUNK else "one")}
            if x["off"][1] == 0:
                seen.add(("norm-tail", bool(n & 3)))
    if len(als) == 2:
        seen.add(("update", "mixed"))
    if c["drop"] is not None:
        seen.add(("table", "dropped"))
    if c["sched"] != SCHED_CONST:
        seen.add(("sched", c["sched"], c["dsteps"], c["dfactor"], c["t"] - 1))
    seen.add(("scale", c["scale"]))
    seen.add(("t", "large" if c["b1"] ** c["t"] <= 0.5 and c["b2"] ** c["t"] <= 0.5 else "small"))
    return seen


# ---------------------------------------------------------------------------------------------- inputs
def exact_grid_ok(g, m, v):
    """every intermediate of the exact family is an integer below 2^24 in units of its grid: x = g / 4 (1/4), (1 - b1) x = g / 8 and
    m' = (4 m + g) / 8 (1/8), (1 - b2) x = g / 16, (1 - b2) x x = g^2 / 64, b2 v = 3 v / 4 and v' = (48 v + g^2) / 64 (1/64)"""
    g, m, v = (np.abs(a.astype(np.float64)) for a in (g, m, v))
    return bool((g == np.round(g)).all() and (m == np.round(m)).all() and (v == np.round(v)).all() and
                (4 * m + g).max() < 2 ** 24 and (g * g).max() < 2 ** 24 and (3 * v).max() < 2 ** 24 and (48 * v + g * g).max() < 2 ** 24)


def inputs(c):
    """{"p", "g", "m", "v"}: a list of fp32 arrays per tensor of the case (dropped ones included), the same for every call"""
    d = dict(p=[], g=[], m=[], v=[])
    for i, x in enumerate(c["tensors"]):
        rng = np.random.default_rng(zlib.crc32(c["name"].encode()) + i)
        n = x["n"]
        pos = np.arange(n)
        if c["exact"]:
            g = (1 + (pos * 7 + i * 131) % 2003) * np.where(pos % 3 == 1, -1, 1)
            m = ((pos * 5 + i * 17) % 509) * np.where(pos % 2 == 1, -1, 1)
            v = (pos * 3 + i * 11) % 8191
            p = rng.standard_normal(n) * 0.05
            assert exact_grid_ok(g, m, v), c["name"]
        else:
            r = rng.standard_normal(n)
            if x["norm"] is None:
                g = r * x["gs"]
            elif x["norm"] == "one":
                g = np.zeros(n)
                g[n // 3] = np.float32(c["clip"]) / np.float32(c["scale"])
                assert float(np.float32(g[n // 3]) * np.float32(c["scale"])) == c["clip"], "clip / grad_scale is not exact in " + c["name"]
            else:
                g = r * (x["norm"] * c["clip"] / (c["scale"] * np.sqrt((r * r).sum()))) if x["norm"] > 0 else np.zeros(n)
            xs = max(float(np.abs(g).max()) * c["scale"], 1e-3) * (0.3 if c["clip"] > 0 and x["norm"] not in (None, "one") and x["norm"] > 1 else 1.0)
            m = rng.standard_normal(n) * 0.3 * xs
            v = rng.uniform(0.25, 1.0, n) * xs * xs
            p = rng.standard_normal(n) * 0.05
        for k, a in zip("pgmv", (p, g, m, v)):
            a = np.ascontiguousarray(a, dtype=np.float32)
            a.setflags(write=False)
            d[k].append(a)
    return d


# ---------------------------------------------------------------------------------------------- the fp64 reference with its bound
def _ex(x):
    return np.asarray(x, np.float64), 0.0


def _mul(a, b):
    v = a[0] * b[0]
    return v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + U * np.abs(v)


def _add(a, b):
    v = a[0] + b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _sub(a, b):
    v = a[0] - b[0]
    return v, a[1] + b[1] + U * np.abs(v)


def _div(a, b):
    v = a[0] / b[0]
    return v, (a[1] + np.abs(v) * b[1]) / np.abs(b[0]) + U * np.abs(v)


def _sqrt(a):
    v = np.sqrt(a[0])
    return v, v - np.sqrt(np.maximum(a[0] - a[1], 0.0)) + U * v


def _cast(a):
    return a[0], a[1] + U * np.abs(a[0])


def _pow(base, q):
    """powf(base, q): base an exact fp32 value > 0, q = (value, e)"""
    v = float(base) ** float(q[0])
    ulp = 2.0 ** (max(math.floor(math.log2(v)), -126) - 23) if v >= 2.0 ** -1000 else 2.0 ** -149      # b^t may underflow: fp32's smallest step
    return np.float64(v), POW_ULP * ulp + v * abs(math.log(base)) * float(q[1])


def reference_partials(c, d):
    """(S, bound) per map row: the sum of the exact squares of fl(g * grad_scale) over the row's chunk"""
    S, B = [], []
    for k, ch in map_rows(c):
        g = d["g"][live(c)[k]][ch * CHUNK:(ch + 1) * CHUNK]
        x = (g * np.float32(c["scale"])).astype(np.float64)
        s = math.fsum(x * x)
        S.append(s)
        B.append(len(g) * 2.0 ** -53 * s)
    return np.array(S, np.float64), np.array(B, np.float64)


def reference(c, d):
    """per live tensor {"p": (p', bound), "m": (m', bound), "v": (v', bound), "lr": the scheduled learning rate, "den": clip_den}: the
    update in fp64 and FACTOR times the first-order bound of the kernel's fp32 evaluation"""
    one, t = _ex(1.0), _ex(float(c["t"]))
    lr, b1, b2, eps, scale, clip = (_ex(c[k]) for k in ("lr", "b1", "b2", "eps", "scale", "clip"))
    if c["sched"] != SCHED_CONST:
        q = _div(_sub(t, one)[:1] + (0.0,), _ex(c["dsteps"]))
        if c["sched"] == SCHED_STAIR:
            q32, qx = sched_q(c)
            assert q32 == qx, "%s: the fp32 floor %r is not the integer floor %r" % (c["name"], q32, qx)
            q = _ex(qx)
        lr = _mul(lr, _pow(c["dfactor"], q))
    bc1, bc2 = _sub(one, _pow(c["b1"], t)), _sub(one, _pow(c["b2"], t))
    sq2 = _sqrt(bc2)
    a = _div(_mul(lr, sq2), bc1) if c["mode"] == 0 else _div(lr, bc1)
    inv_sq2 = _div(one, sq2)
    c1, c2 = _sub(one, b1), _sub(one, b2)
    out = []
    for i in live(c):
        p, g, m, v = (_ex(d[k][i]) for k in "pgmv")
        n = len(p[0])
        y = _mul(g, scale)
        den = None
        if c["clip"] > 0:
            s = math.fsum(y[0] * y[0])
            rows = (n + CHUNK - 1) // CHUNK
            norm = _sqrt(_cast((np.float64(s), s * (2 * U + (n + rows) * 2.0 ** -53))))
            den = (np.maximum(norm[0], clip[0]), norm[1] if norm[0] + norm[1] >= clip[0] else 0.0)
            y = _div(_mul(y, clip), den)
        m2 = _add(_mul(b1, m), _mul(c1, y))
        v2 = _add(_mul(b2, v), _mul(_mul(c2, y), y))
        root = _sqrt(v2)
        dd = _add(root, eps) if c["mode"] == 0 else _add(_mul(root, inv_sq2), eps)
        p2 = _sub(p, _div(_mul(a, m2), dd))
        wide = lambda r: (r[0], FACTOR * np.broadcast_to(r[1], r[0].shape))
        out.append(dict(p=wide(p2), m=wide(m2), v=wide(v2), lr=float(lr[0]), den=None if den is None else float(den[0])))
    return out


# ---------------------------------------------------------------------------------------------- the kernel restated in NumPy fp32
def kernel32(c, d, plant=None):
    """the two Adam kernels operation for operation in NumPy fp32 (the stand-in library of the CPU file): (per live tensor {"p", "m", "v"},
    partials of len(map) + 3 rows or None).  plant: one of PLANTS, a wrong kernel"""
    f = np.float32
    one, t = f(1), f(c["t"])
    lr, b1, b2, eps, scale, clip = (f(c[k]) for k in ("lr", "b1", "b2", "eps", "scale", "clip"))
    if c["sched"] != SCHED_CONST:
        q = (t if plant == "t_for_tm1" else t - one) / f(c["dsteps"])
        if c["sched"] == SCHED_STAIR and plant != "nofloor":
            q = np.floor(q)
        lr = lr * np.power(f(c["dfactor"]), q)
    bc1, bc2 = one - np.power(b1, t), one - np.power(b2, t)
    sq2 = np.sqrt(bc2)
    mode0 = (c["mode"] == 0) != (plant == "other_prefactor")
    a = lr * sq2 / bc1 if mode0 else lr / bc1
    inv_sq2 = one / sq2
    rows = map_rows(c)
    partials = None
    if c["clip"] > 0:
        partials = np.full(len(rows) + 3, PARTIAL_FILL, np.float64)
        for r, (k, ch) in enumerate(rows):
            i = live(c)[k]
            g = d["g"][i][ch * CHUNK:(ch + 1) * CHUNK]
            if plant == "drop_tail" and c["tensors"][i]["off"][1] == 0:
                g = g[:len(g) // 4 * 4]
            x = (g * scale).astype(np.float64)
            partials[r] = np.sum(x * x)
    out, first = [], 0
    for i in live(c):
        p, g, m, v = (d[k][i] for k in "pgmv")
        nrows = (len(p) + CHUNK - 1) // CHUNK
        x = g * scale
        if c["clip"] > 0:
            s = 0.0
            for r in range(nrows + (plant == "extra_row")):
                s += partials[first + r]
            with np.errstate(invalid="ignore"):                # a planted row range may reach the pre-fill
                x = (x * clip) / max(np.sqrt(f(s)), clip)
        m2 = b1 * m + (one - b1) * x
        v2 = b2 * v + (one - b2) * x * x
        root = np.sqrt(v2 + eps) if plant == "eps_under_root" else np.sqrt(v2)
        dd = (root if c["mode"] == 0 else root * inv_sq2) + (f(0) if plant == "eps_under_root" else eps)
        p2 = p - a * m2 / dd
        assert p2.dtype == m2.dtype == v2.dtype == np.float32
        out.append(dict(p=p2, m=m2, v=v2))
        first += nrows
    return out, partials


def worst_ratios(c, d, got, partials):
    """{"p", "m", "v", "partials"}: max |got - reference| / bound over the case (a NaN or a difference at a zero bound gives inf)"""
    def ratio(x, r, b):
        diff = np.abs(np.asarray(x, np.float64) - r)
        q = np.where(diff == 0, 0.0, diff / np.maximum(b, 1e-300))
        return float(np.where(np.isnan(q), np.inf, q).max()) if q.size else 0.0
    ref = reference(c, d)
    out = {k: max(ratio(o[k], r[k][0], r[k][1]) for o, r in zip(got, ref)) for k in "pmv"}
    if c["clip"] > 0:
        S, B = reference_partials(c, d)
        out["partials"] = ratio(partials[:len(S)], S, B)
    return out


# ---------------------------------------------------------------------------------------------- hf_copy_multi
COPY_BYTES = (0, 1, 15, 16, 17, 65535, 65536, 65537, 3 * 65536 + 5)


def _copy_case(name, entries):
    """entries: (bytes, dst 1 byte off, src 1 byte off) per copy; a negative byte count stands for a zero-byte copy with NULL pointers"""
    return dict(name="copy-" + name, entries=[tuple(e) for e in entries])


def _copy_build():
    out = []
    for b in COPY_BYTES:
        for do, so in ((0, 0), (1, 0), (0, 1), (1, 1)):
            if b <= 65537 or do == so:
                out.append(_copy_case("n=1-bytes=%d-dst%d-src%d" % (b, do, so), [(b, do, so)]))
    out.append(_copy_case("n=2", [(17, 0, 0), (65537, 1, 0)]))
    small = (1, 15, 16, 17, 0, 255, 4096, 4097)
    for n in (63, 64):
        out.append(_copy_case("n=%d-every-slot" % n, [(small[i % 8] or 3 if n == 64 else small[i % 8], i % 3 == 1, i % 5 == 2) for i in range(n)]))
    out.append(_copy_case("n=64-chunks", [((65535, 65536, 65537, 16)[i % 4] if i % 9 == 0 else (i * 37) % 300, 0, 0) for i in range(64)]))
    out.append(_copy_case("zero-first-middle-last", [(0, 0, 0), (17, 0, 0), (0, 0, 0), (-1, 0, 0), (65537, 0, 0), (0, 1, 1)]))
    out.append(_copy_case("all-zero", [(0, 0, 0), (-1, 0, 0)]))
    out.append(_copy_case("long-among-short", [(1, 0, 0), (16, 0, 0), (3 * 65536 + 5, 0, 0), (15, 1, 0), (17, 0, 0)]))
    return out


COPY_CASES = _copy_build()


def copy_source(c, i):
    """the bytes of copy i"""
    b = max(c["entries"][i][0], 0)
    return np.random.default_rng(zlib.crc32(c["name"].encode()) + i).integers(0, 256, b, dtype=np.uint8)


def copy_first(c):
    """the prefix table of the launch: first[i], and the number of workgroups"""
    first, chunks = [], 0
    for b, _, _ in c["entries"]:
        first.append(chunks)
        chunks += (max(b, 0) + COPY_CHUNK - 1) // COPY_CHUNK
    return first, chunks


def copy_search(first, n, chunks, block):
    """the kernel's six steps on first[0 .. 64] (first[n ..] = chunks): the copy that workgroup `block` serves"""
    table = list(first) + [chunks] * (COPY_MAX + 1 - n)
    lo, hi = 0, COPY_MAX - 1
    for _ in range(6):
        mid = (lo + hi + 1) >> 1
        if table[mid] <= block:
            lo = mid
        else:
            hi = mid - 1
    return lo


def copy_regimes_of(c):
    first, chunks = copy_first(c)
    n = len(c["entries"])
    seen = {("n", n)}
    for block in range(chunks):
        which = copy_search(first, n, chunks, block)
        b, do, so = c["entries"][which]
        assert first[which] <= block < first[which] + (b + COPY_CHUNK - 1) // COPY_CHUNK, (c["name"], block, which)
        nb = min(COPY_CHUNK, b - (block - first[which]) * COPY_CHUNK)
        seen.add(("which", which))
        if not do and not so:
            n16 = nb >> 4
            seen |= {("copy", "vec"), ("copy-trips", "none" if n16 == 0 else "partial" if n16 < THREADS else "one" if n16 == THREADS else "several"),
                     ("copy-tail", bool(nb & 15))}
        else:
            seen.add(("copy", "bytes", bool(do), bool(so)))
        if block > first[which]:
            seen.add(("copy-chunk", "later"))
    for i, (b, _, _) in enumerate(c["entries"]):
        if b <= 0:
            seen.add(("zero", "first" if i == 0 else "last" if i == n - 1 else "middle"))
            if b < 0:
                seen.add(("zero", "null"))
    return seen
