"""Case table and fp64 references of the kernel-level parity suite of csrc/gemm.hip (tests/test_gemm_abi.py runs the cases on
the GPU through the C ABI, tests/test_gemm_instantiations_cpu.py checks on any machine that the cases reach every compiled
template instantiation).  A plain helper module: nothing here imports the library.

Dispatch rule, restated from include/hfops.h and the launcher comments of gemm.hip (NOT imported):
  linear_fwd_kernel<NT, VEC, GATHER>   NT = ceil(cout / 32); VEC = cin % 4 == 0 and x, weight and (if given) x_act 16-byte aligned
                                       (the gather forms: cin = pad4(c_feat) + 4, so VEC is the weight's alignment alone)
  linear_bwd_kernel<NT, VEC, FROM_DY>  NT = ceil(cin / 32); VEC = cout % 4 == 0 and dy_or_dz, weight_t, z, dz_out (those given)
                                       aligned; FROM_DY = z != NULL
  wgrad_kernel<WM, WN, VEC, GATHER>    WM = 2 if cout > 64 else 1, WN = 2 if cin > 64 else 1; VEC = cout % 4 == 0 and grad_z aligned
                                       and (dense form) cin % 4 == 0 and x aligned
  lift_linear_fwd_kernel<NT>           NT = ceil(c1 / 32)
  lift_linear_bwd_kernel<NT, PASS>     NT = ceil(c0 / 32) <= 5, both passes at every call
  lift_wgrad_kernel<WM, WN>            WM = c1 > 64, WN = c0 > 64
and the persistent grids: min(256 CUs x {5,4,3,3,2,2,2,2}[NT-1] x 2 rounds, 2048, tiles) workgroups of 128 rows (2 rounds is a constant of the
product library; a diagnostic build reads HF_GEMM_ROUNDS, which the GPU tests therefore require to be unset).

Rounding bounds.  u = 2^-24.  Every bound below has the form  c * u * M (+ propagated input error), M being the same formula
evaluated in fp64 with every operand replaced by its magnitude, and c the number of fp32 roundings on the longest path to the
element; each reference function derives its c in its docstring.  The two transcendental paths whose rounding cannot be read
from the code (expm1f of elu_fwd, exp(x) - 1 on the hardware exponential of elu_hw) are given 4 x the error that a plain fp32
torch evaluation of the same formula makes against fp64 on the same inputs (ELU_FACTOR; measured at run time on the host by
elu_abs_error; at the N(0,1)-scale inputs of the cases that measurement is 3.0e-8 .. 6.0e-8 for both formulas, i.e. about u)."""
import torch

U = 2.0 ** -24
NUM_CU = 256
BN_MAX_BLOCKS = 2048
FWD_ROWS = 128
ELU_FACTOR = 4.0
RELU_MARGIN = 1e-3
_PER_CU = (5, 4, 3, 3, 2, 2, 2, 2)


def cdiv(a, b):
    return (a + b - 1) // b


def resident_grid(nt):
    return min(NUM_CU * _PER_CU[nt - 1] * 2, BN_MAX_BLOCKS)


def multi_tile_rows(nt):
    """every workgroup of the persistent grid walks two tiles, workgroup 0 a third, ragged one"""
    return 2 * resident_grid(nt) * FWD_ROWS + 77


def tiles_per_workgroup(rows, nt):
    tiles = cdiv(rows, FWD_ROWS)
    return cdiv(tiles, min(resident_grid(nt), tiles))


def wgrad_plan(rows, cout, cin):
    """(wm, wn, rows per chunk, chunks): about three workgroups per CU, chunks of at least 256 rows, multiples of 32"""
    wm, wn = (2 if cout > 64 else 1), (2 if cin > 64 else 1)
    want = max(1, NUM_CU * 3 // (cdiv(cout, 64 * wm) * cdiv(cin, 64 * wn)))
    rpc = cdiv(max(cdiv(rows, want), 256), 32) * 32
    return wm, wn, rpc, cdiv(rows, rpc)


# ---------------------------------------------------------------------------------------------- the case table
COUT_EDGES = (1, 31, 32, 33, 64, 65, 96, 100, 128, 129, 160, 161, 192, 193, 224, 225, 255, 256)   # both edges of every NT
FWD_CINS = (1, 3, 4, 31, 32, 33, 36, 64, 100, 1023, 1024)
TILE_ROWS = (1, 127, 128, 129, 645)
BWD_COUTS = (1, 3, 4, 31, 32, 33, 64, 100, 256, 384)
BWD_FORMS = ("dz_dx", "dz_dx_sums", "dy_dx_dzout", "dy_dzout", "dz_sums")
WGRAD_PAIRS = ((1, 1), (63, 64), (64, 64), (64, 65), (65, 64), (65, 63), (128, 64), (64, 128), (128, 129), (129, 128), (128, 200),
               (200, 200), (200, 1), (1, 200))
WGRAD_ROWS = (1, 31, 32, 33, 255, 256, 257, 200003)
GATHER_CFEATS = (0, 1, 3, 4, 5, 64, 1020)
GATHER_COUTS = (31, 64, 96, 100, 160, 161, 224, 256)        # one per NT
LIFT_C0_ALL = (4, 32, 36, 64, 96, 128, 160)                 # 96: the only width at NT = 3 of the backward
LIFT_C0_FWD = (164, 192, 256)
LIFT_C1_EDGES = (1, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 224, 225, 256)


def _case(kind, **kw):
    kw["kind"] = kind
    kw.setdefault("family", "exact")
    kw.setdefault("misalign", None)
    return kw


def case_id(c):
    skip = ("kind", "misalign", "family")
    parts = [c["kind"], c["family"]] + ["%s%s" % (k, int(v) if isinstance(v, bool) else v) for k, v in c.items() if k not in skip]
    if c["misalign"]:
        parts.append("off_" + c["misalign"])
    return "-".join(parts)


def _both(cases, every=2):
    """the exact family of every case and the rounding family of every `every`-th one"""
    out = []
    for i, c in enumerate(cases):
        out.append(dict(c, family="exact"))
        if i % every == 0:
            out.append(dict(c, family="round"))
    return out


def fwd_cases():
    shapes = []
    for cout in COUT_EDGES:
        shapes += [(645, 36, cout), (129, 33, cout)]
    for cin in FWD_CINS:
        shapes += [(129, cin, 31), (257, cin, 161)]
    for rows in TILE_ROWS:
        shapes += [(rows, 36, 32), (rows, 36, 160), (rows, 35, 256)]
    out = []
    for i, (rows, cin, cout) in enumerate(shapes):
        for elu in (False, True):
            m, k = i // 2, i + (3 if elu else 0)        # m: the pair the rounding family is thinned by; the switches cycle within and across pairs
            act = (i + m // 2 + elu) % 2 == 1 or i % 6 == 0
            c = _case("fwd", elu=elu, rows=rows, cin=cin, cout=cout, act=act, xact=act and (m // 2 + i) % 3 != 0, bias=(not elu) and k % 3 != 0,
                      running=(i + m // 2) % 4)
            out.append(c)
            # the rounding family thinned by PAIRS of shapes, alternating between the two entry points: each of them keeps every NT, both
            # parities of the switches above and both access widths (negative ELU arguments exist in this family only)
            if (i // 2 + elu) % 2 == 0:
                out.append(dict(c, family="round"))
    for nt in range(1, 9):          # the tile loop and its prefetch across tiles
        for elu in (False, True):
            out.append(_case("fwd", elu=elu, rows=multi_tile_rows(nt), cin=36, cout=32 * nt - (nt % 2), act=nt % 2 == 0,
                             xact=nt % 4 == 0, bias=not elu, running=0))
    return out


def bwd_cases():
    """the rounding family is the only one with dgamma, dbeta != 0 (the - dbeta / R - xhat dgamma / R part of the dz formula), so it takes
    EVERY dy form of the cin sweep (each cin has a dy -> dx + dz_out case), and one dz form per cin"""
    dz_forms, dy_forms = ("dz_dx", "dz_dx_sums", "dz_sums"), ("dy_dx_dzout", "dy_dzout")
    out = []

    def add(rounding, **kw):
        c = _case("bwd", **kw)
        out.append(c)
        if rounding:
            out.append(dict(c, family="round"))

    for j, cin in enumerate(COUT_EDGES):
        for ci, cout in enumerate((33, 64)):
            form = dz_forms[(j + ci) % 3]
            elu = form != "dz_dx" and ((j // 2 + ci) % 2 == 0 or cin == 192)       # 192: without it NT = 6 has no ELU-below case
            add(ci == j % 2 or elu, rows=645, cout=cout, cin=cin, form=form, elu=elu)
            add(True, rows=645, cout=cout, cin=cin, form=dy_forms[(j + ci) % 2], elu=False)
    for i, cout in enumerate(BWD_COUTS):
        for cin in (33, 160):
            form = dz_forms[i % 3] if cout > 256 else BWD_FORMS[(i + cin) % 5]
            add((i + cin) % 2 == 0, rows=257, cout=cout, cin=cin, form=form, elu=form in ("dz_dx_sums", "dz_sums") and i % 2 == 0)
    for rows in TILE_ROWS:
        for j, cin in enumerate((32, 160, 256)):
            add((rows + j) % 2 == 0, rows=rows, cout=36, cin=cin, form=BWD_FORMS[(rows + j) % 5], elu=False)
    for nt in range(1, 9):
        form = "dz_dx_sums" if nt % 2 else "dy_dx_dzout"
        out.append(_case("bwd", rows=multi_tile_rows(nt), cout=36, cin=32 * nt - (nt % 2), form=form, elu=nt % 4 == 1))
    return out


def wgrad_cases():
    cases = []
    for i, (cout, cin) in enumerate(WGRAD_PAIRS):
        for rows in (33, 257):
            cases.append(_case("wgrad", rows=rows, cout=cout, cin=cin, act=(i + rows) % 2 == 0))
    for rows in WGRAD_ROWS:
        cases.append(_case("wgrad", rows=rows, cout=64, cin=64, act=rows % 2 == 1))
        cases.append(_case("wgrad", rows=rows, cout=129, cin=65, act=rows % 2 == 0))
    for cout, cin in ((63, 64), (65, 129), (128, 64), (64, 200)):
        cases.append(_case("wgrad", rows=200003, cout=cout, cin=cin, act=cout % 2 == 0))
    cases += [_case("wgrad", rows=257, cout=1000, cin=40, act=False), _case("wgrad", rows=200003, cout=1000, cin=40, act=True)]
    seen, uniq = set(), []
    for c in cases:
        key = (c["rows"], c["cout"], c["cin"])
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return _both(uniq)


def gather_cases():
    out = []
    for i, cout in enumerate(GATHER_COUTS):
        for j, off in enumerate((None, "weight")):
            out.append(_case("gather_fwd", clouds=3, rows_per_cloud=50, n_src=17, c_feat=GATHER_CFEATS[(2 * i + j) % 7], cout=cout,
                             bias=(i + j) % 2 == 0, misalign=off))
    for cf in GATHER_CFEATS:    # every c_feat at least once on each route
        out.append(_case("gather_fwd", clouds=2, rows_per_cloud=150, n_src=9, c_feat=cf, cout=65, bias=cf % 2 == 0))
    for cout in (63, 64, 65, 128):
        for cf in (5, 64):
            out.append(_case("gather_wgrad", clouds=3, rows_per_cloud=100, n_src=17, c_feat=cf, cout=cout))
    for cf in (0, 1, 3, 4, 1020):
        out.append(_case("gather_wgrad", clouds=2, rows_per_cloud=150, n_src=9, c_feat=cf, cout=36))
    return out


def lift_shapes():
    shapes = [(129, 36, c1) for c1 in LIFT_C1_EDGES]
    for c0 in LIFT_C0_ALL + LIFT_C0_FWD:
        shapes += [(129, c0, 33), (1, c0, 256)]
    shapes += [(40000, 32, 64), (40000, 160, 100), (multi_tile_rows(8), 36, 256)]
    return shapes


def lift_cases():
    out = []
    for rows, c0, c1 in lift_shapes():
        out.append(_case("lift_eval", rows=rows, c0=c0, c1=c1))
        out.append(_case("lift_eval_bn", rows=rows, c0=c0, c1=c1))
        if rows <= 40000:
            out.append(_case("lift_train", rows=rows, c0=c0, c1=c1, family="round"))
    out.append(_case("lift_train", rows=multi_tile_rows(8), c0=36, c1=256, family="round"))
    return out


def lift_bwd_cases():
    shapes = [(129, c0, c1) for c0 in LIFT_C0_ALL for c1 in (33, 64, 256)]
    shapes += [(1, 36, 65), (40000, 32, 64), (40000, 160, 100), (multi_tile_rows(5), 160, 36)]
    return [_case("lift_bwd", rows=r, c0=c0, c1=c1, family="round") for r, c0, c1 in shapes]


# one case per kernel family; every pointer the launcher's alignment test inspects is offset in turn
ALIGN_CASES = (
    [_case("fwd", elu=False, rows=300, cin=36, cout=100, act=True, xact=True, bias=True, running=0, misalign=m)
     for m in ("x", "weight", "x_act")] +
    [_case("bwd", rows=300, cout=36, cin=100, form="dy_dx_dzout", elu=False, misalign=m) for m in ("dy", "weight_t", "z", "dz_out")] +
    [_case("bwd", rows=300, cout=36, cin=100, form="dz_dx_sums", elu=False, misalign=m) for m in ("dy", "weight_t")] +
    [_case("wgrad", rows=300, cout=128, cin=36, act=True, misalign=m) for m in ("grad_z", "x")] +
    [_case("gather_fwd", clouds=3, rows_per_cloud=50, n_src=17, c_feat=64, cout=100, bias=True, misalign=m) for m in ("points", "weight")] +
    [_case("gather_wgrad", clouds=3, rows_per_cloud=100, n_src=17, c_feat=64, cout=128, misalign=m) for m in ("grad_z", "points")] +
    [_case("lift_bwd", rows=300, c0=36, c1=100, family="exact", misalign=m) for m in ("dz1", "w1_t")])


def _unique(cases):
    seen, out = set(), []
    for c in cases:
        if case_id(c) not in seen:
            seen.add(case_id(c))
            out.append(c)
    return out


def all_cases():
    return _unique(fwd_cases() + bwd_cases() + wgrad_cases() + gather_cases() + lift_cases() + lift_bwd_cases() + list(ALIGN_CASES))


def sweep_cases(*kinds):
    """the sweep cases of the given kinds (the alignment twins are a table of their own)"""
    twins = {case_id(c) for c in ALIGN_CASES}
    return [c for c in all_cases() if c["kind"] in kinds and case_id(c) not in twins]


# ---------------------------------------------------------------------------------------------- which kernels a case launches
def instantiations(c):
    """the (kernel, template arguments) a case launches by the dispatch rule in the module docstring"""
    k, mis = c["kind"], c["misalign"]
    if k == "fwd":
        vec = c["cin"] % 4 == 0 and mis not in ("x", "weight", "x_act")
        return {("linear_fwd_kernel", (cdiv(c["cout"], 32), vec, False))}
    if k == "gather_fwd":
        return {("linear_fwd_kernel", (cdiv(c["cout"], 32), mis != "weight", True))}
    if k == "bwd":
        from_dy = c["form"].startswith("dy")
        vec = c["cout"] % 4 == 0 and mis not in ("dy", "weight_t", "z", "dz_out")
        return {("linear_bwd_kernel", (cdiv(c["cin"], 32), vec, from_dy))}
    if k == "wgrad":
        vec = c["cout"] % 4 == 0 and c["cin"] % 4 == 0 and mis not in ("grad_z", "x")
        return {("wgrad_kernel", (2 if c["cout"] > 64 else 1, 2 if c["cin"] > 64 else 1, vec, False)), ("wgrad_reduce_kernel", ())}
    if k == "gather_wgrad":
        cin = (c["c_feat"] + 3) // 4 * 4 + 4
        vec = c["cout"] % 4 == 0 and mis != "grad_z"
        return {("wgrad_kernel", (2 if c["cout"] > 64 else 1, 2 if cin > 64 else 1, vec, True)), ("wgrad_reduce_kernel", ())}
    if k in ("lift_eval", "lift_eval_bn"):
        return {("lift_linear_fwd_kernel", (cdiv(c["c1"], 32),))}
    if k == "lift_train":
        return {("lift_linear_fwd_kernel", (cdiv(c["c1"], 32),)), ("lift_stats_kernel", ())}
    if k == "lift_bwd":
        nt = cdiv(c["c0"], 32)
        return {("lift_linear_bwd_kernel", (nt, 0)), ("lift_linear_bwd_kernel", (nt, 1)), ("partial_rows_sum_kernel", ()),
                ("lift_wgrad_kernel", (2 if c["c1"] > 64 else 1, 2 if c["c0"] > 64 else 1)), ("wgrad_reduce_kernel", ())}
    raise KeyError(k)


def selected_instantiations(cases=None):
    out = set()
    for c in (all_cases() if cases is None else cases):
        out |= instantiations(c)
    return out


# ---------------------------------------------------------------------------------------------- inputs
def generator(c):
    """seeded by the case's shape and switches: both families and the misaligned twins of a case draw the same numbers"""
    return torch.Generator().manual_seed(_seed(c))


def _seed(c):
    s = 17
    for k in sorted(c):
        if k in ("misalign", "family"):
            continue
        v = c[k]
        for ch in (str(k) + "=" + str(v)):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


def ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def sparse_pm1(g, shape, density=0.25):
    """sparse +-1 operand: keeps |z| and the per-workgroup statistics sums small"""
    return ints(g, shape, -1, 1) * (torch.rand(shape, generator=g) < density).float()


def bn_consts(g, c, exact, nonneg=False):
    """(gamma, beta, mean, invstd) of a BatchNorm applied on load: integer-valued affine in the exact family (nonneg: mean <= beta so
    that the affine of a non-negative input stays non-negative), non-trivial constants with means off zero otherwise"""
    if exact:
        mean = ints(g, (c,), 0, 1) if nonneg else ints(g, (c,), -1, 1)
        beta = ints(g, (c,), 1, 2) if nonneg else ints(g, (c,), -1, 1)
        return torch.ones(c), beta, mean, torch.ones(c)
    return (torch.rand(c, generator=g) + 0.5, torch.rand(c, generator=g) - 0.5, torch.randn(c, generator=g) * 0.5 + 0.3,
            1.0 / (torch.rand(c, generator=g) + 0.5))


NUDGE_SHARE_MIN_NUMEL = 20000


def nudge_off_relu_threshold(z, gamma, beta, mean, invstd):
    """moves the elements of the fp32 tensor z whose fp64 pre-activation a (z - mu) + beta lies within 1.1 * RELU_MARGIN of zero
    to 3 * RELU_MARGIN further from it, in place; afterwards relu_margin() >= RELU_MARGIN (asserted by the tests).  Returns the
    share of moved elements: about 1e-3 for a normal pre-activation, and the tests assert it stays below 2e-3 for every tensor of at least
    NUDGE_SHARE_MIN_NUMEL elements (there 2e-3 is more than four standard deviations of the count above its expectation; in a tensor of a
    few hundred elements one moved element already exceeds the share and says nothing about the distribution)."""
    a = (gamma.double() * invstd.double())
    pre = a * (z.double() - mean.double()) + beta.double()
    near = pre.abs() < 1.1 * RELU_MARGIN
    step = (3 * RELU_MARGIN / a.abs()).expand_as(pre)
    z[near] = (z.double() + torch.where(pre >= 0, step, -step))[near].float()
    return float(near.double().mean())


def nudge_share_ok(share, numel):
    return share < 2e-3 or numel < NUDGE_SHARE_MIN_NUMEL


def relu_margin(z, gamma, beta, mean, invstd):
    a = (gamma.double() * invstd.double())
    return float((a * (z.double() - mean.double()) + beta.double()).abs().min())


def elu_abs_error(x32, lift):
    """max |fp32 torch evaluation - fp64| of the ELU formula the kernel uses, on the same inputs, on the host: expm1 (elu_fwd) or
    exp(x) - 1 (elu_hw); the kernels get ELU_FACTOR times this"""
    x32 = x32.detach().float().cpu()
    neg = x32[x32 <= 0]
    if neg.numel() == 0:
        return 0.0
    got = (torch.exp(neg) - 1.0) if lift else torch.expm1(neg)
    return float((got.double() - torch.expm1(neg.double())).abs().max())


# ---------------------------------------------------------------------------------------------- fp64 references
def _d(t):
    return None if t is None else t.double()


def elu64(x):
    return torch.where(x > 0, x, torch.expm1(x))


def ref_on_load(x, bn, elu):
    """activation on load, value and bound.  a = gamma * invstd (1 rounding), d = e - mu (1), a * d (1), + beta (1): 4 roundings on
    the magnitude |a| (|e| + |mu|) + |beta|; e = x, or elu(x) with its own error err_e added as |a| err_e.  The ReLU clamp is exact.
    Returns (h, |h| magnitude envelope, absolute error bound of h)"""
    x = _d(x)
    if bn is None:
        return x, x.abs(), torch.zeros_like(x)
    gamma, beta, mean, invstd = [_d(t) for t in bn]
    a = gamma * invstd
    e = elu64(x) if elu else x
    h = a * (e - mean) + beta
    if not elu:
        h = h.clamp(min=0)
    mag = a.abs() * (e.abs() + mean.abs()) + beta.abs()
    err = 4 * U * mag
    if elu:
        err = err + a.abs() * ELU_FACTOR * elu_abs_error(x, lift=False)
    return h, mag, err


def stats_bounds(s, err_s, chain, eps):
    """BatchNorm batch statistics of the (rows, c) fp64 tensor s, whose fp32 counterpart carries the absolute error err_s, as the
    epilogues form them: a lane adds `chain` values in sequence in fp32 (its rows of every tile, the other row-half, the four waves),
    the per-workgroup sums are added in fp64, mean = S / R, var = Q / R - mean^2 and the casts to fp32:
      |d mean|   <= mean_r(err_s + chain u |s|) + u |mean|
      |d var|    <= mean_r(2 |s| err_s + (chain + 1) u s^2) + 2 |mean| |d mean|       (the square is one more rounding)
      |d invstd| <= invstd^3 (|d var| + u eps) / 2 + u invstd                        (eps arrives as a float)
    Returns mean, var, invstd and their three bounds"""
    mean = s.mean(0)
    var = (s * s).mean(0) - mean * mean
    var = var.clamp(min=0)
    invstd = 1.0 / torch.sqrt(var + eps)
    d_mean = (err_s + chain * U * s.abs()).mean(0) + U * mean.abs()
    d_var = (2 * s.abs() * err_s + (chain + 1) * U * s * s).mean(0) + 2 * mean.abs() * d_mean
    d_invstd = 0.5 * invstd ** 3 * (d_var + U * eps) + U * invstd
    return mean, var, invstd, d_mean, d_var, d_invstd


def running_bounds(r0, batch, d_batch, m):
    """running = (1 - m) r0 + m batch in fp32: 1 - m, two products, one sum: 3 roundings on |(1 - m) r0| + |m batch|, plus the
    error of the batch value and its cast"""
    r0, want = _d(r0), (1 - m) * _d(r0) + m * batch
    return want, 3 * U * ((1 - m) * r0.abs() + m * batch.abs()) + m * (d_batch + U * batch.abs())


def ref_linear_fwd(x, bn, w, bias, elu, rows_chain, eps):
    """z = h W^T + bias with h = ref_on_load(x): the MFMA is a k-ordered fmaf chain, one rounding per input channel, the bias one
    more: |dz| <= (cin + 1) u (|h|mag |W|^T + |bias|) + err_h |W|^T.  Statistics of z (of elu(z) for the ELU entry point, whose expm1f
    adds ELU_FACTOR x its measured error) by stats_bounds with chain = 16 rows per lane and tile x tiles per workgroup + 4."""
    h, hmag, herr = ref_on_load(x, bn, elu)
    w64 = _d(w)
    z = h @ w64.t()
    mag = hmag @ w64.abs().t()
    if bias is not None:
        z = z + _d(bias)
        mag = mag + _d(bias).abs()
    z_err = (x.shape[1] + 1) * U * mag + herr @ w64.abs().t()
    s, s_err = z, z_err
    if elu:
        s = elu64(z)
        s_err = z_err + ELU_FACTOR * elu_abs_error(z.float(), lift=False) + U * s.abs()
    mean, var, invstd, d_mean, d_var, d_invstd = stats_bounds(s, s_err, rows_chain, eps)
    return dict(z=z, z_err=z_err, h=h, h_err=herr, mean=mean, var=var, invstd=invstd, d_mean=d_mean, d_var=d_var, d_invstd=d_invstd)


def ref_linear_bwd(dy, z, bn, dgamma, dbeta, wt, zprev, pbn, elu, rows_chain):
    """dx = dz W (wt = W^T as (cin, cout)).  z given: dz = a (dh - dbeta / R - xhat dgamma / R), dh = dy where a (z - mu) + beta > 0,
    xhat = (z - mu) invstd, formed as the header writes it.  Roundings of dz on the longest path: 1 / R, dgamma / R, z - mu, xhat,
    xhat * (dgamma / R), the two differences, a, the last product: 9, on |a| (|dh| + |dbeta| / R + (|z| + |mu|) invstd |dgamma| / R).
    dx: one rounding per output channel of the layer: |d dx| <= cout u (|dz|mag |W|) + err_dz |W|.
    zprev given: the BatchNorm-backward sums of the layer below, p_dbeta = sum dh', p_dgamma = sum dh' xhat' with dh' = dx under that
    layer's ReLU mask and xhat' = (zprev - mu') invstd' (ELU below: dh' = dx, xhat' from elu(zprev)): xhat' costs 2 roundings on
    X = (|e'| + |mu'|) invstd', the product one more, a lane adds `rows_chain` terms in sequence in fp32, the rest is fp64:
      |d p_dbeta|  <= sum_r(err_dx + chain u |dh'|) + u |p_dbeta|
      |d p_dgamma| <= sum_r(err_dx X + (chain + 3) u |dh'| X [+ |dx| invstd' err_elu]) + u |p_dgamma|"""
    rows = dy.shape[0]
    w64 = _d(wt)
    out = {}
    if z is not None:
        gamma, beta, mean, invstd = [_d(t) for t in bn]
        a = gamma * invstd
        dh = torch.where(a * (_d(z) - mean) + beta > 0, _d(dy), torch.zeros((), dtype=torch.float64, device=dy.device))
        xhat = (_d(z) - mean) * invstd
        dz = a * (dh - _d(dbeta) / rows - xhat * _d(dgamma) / rows)
        dzmag = a.abs() * (dh.abs() + _d(dbeta).abs() / rows + (_d(z).abs() + mean.abs()) * invstd * _d(dgamma).abs() / rows)
        dz_err = 9 * U * dzmag
        out.update(dz=dz, dz_err=dz_err)
    else:
        dz, dzmag, dz_err = _d(dy), _d(dy).abs(), torch.zeros_like(_d(dy))
    dx = dz @ w64.t()
    dx_err = dy.shape[1] * U * (dzmag @ w64.abs().t()) + dz_err @ w64.abs().t()
    out.update(dx=dx, dx_err=dx_err)
    if zprev is not None:
        pg, pb, pm, pis = [_d(t) for t in pbn]
        zp = _d(zprev)
        if elu:
            e = elu64(zp)
            dh2 = dx
            extra = dx.abs() * pis * ELU_FACTOR * elu_abs_error(zprev, lift=False)
        else:
            e = zp
            dh2 = torch.where(pg * pis * (zp - pm) + pb > 0, dx, torch.zeros((), dtype=torch.float64, device=dy.device))
            extra = 0.0
        xh, xmag = (e - pm) * pis, (e.abs() + pm.abs()) * pis
        p_dbeta, p_dgamma = dh2.sum(0), (dh2 * xh).sum(0)
        out.update(p_dbeta=p_dbeta, p_dgamma=p_dgamma,
                   d_p_dbeta=(dx_err + rows_chain * U * dh2.abs()).sum(0) + U * p_dbeta.abs(),
                   d_p_dgamma=(dx_err * xmag + (rows_chain + 3) * U * dh2.abs() * xmag + extra).sum(0) + U * p_dgamma.abs(),
                   sum_abs=torch.maximum(dh2.abs().sum(0), (dh2 * xh).abs().sum(0)))
    return out


def ref_wgrad(g, x, bn, rows_per_chunk, chunks):
    """dW = g^T h, h = ref_on_load(x) (ReLU form).  A chunk's rows are one fmaf chain (min(rows, rows_per_chunk) roundings); the
    chunk partials are added as 16 interleaved groups of ceil(chunks / 16) and the 16 group sums in sequence:
      |d dW| <= (rows in a chunk + ceil(chunks / 16) + 15) u (|g|^T |h|mag) + |g|^T err_h"""
    h, hmag, herr = ref_on_load(x, bn, False)
    g64 = _d(g)
    c = min(g.shape[0], rows_per_chunk) + cdiv(chunks, 16) + 15
    return dict(dw=g64.t() @ h, dw_err=c * U * (g64.abs().t() @ hmag) + g64.abs().t() @ herr)


def gather_operand(points, idx, gxyz, rows_per_cloud):
    """the materialised operand of the gather forms: [features | zero pad to a multiple of 4 | x y z 0]"""
    rows = idx.shape[0]
    cf = 0 if points is None else points.shape[2]
    cfp = (cf + 3) // 4 * 4
    a = torch.zeros(rows, cfp + 4, dtype=gxyz.dtype, device=gxyz.device)
    if cf:
        cloud = torch.arange(rows, device=idx.device) // rows_per_cloud
        a[:, :cf] = points[cloud, idx.long()]
    a[:, cfp:cfp + 3] = gxyz
    return a


def ref_lift_first(x3, w0):
    """e0 = elu(z0), z0 = (x0 wx + x1 wy) + x2 wz: three rounded products and two sums, 3 roundings on the longest path, on |x3| |w0|^T;
    exp(z0) - 1 on the hardware exponential: ELU_FACTOR x the measured error of the fp32 formula; ELU is 1-Lipschitz.
    Returns z0, e0, err_e0, err_z0"""
    z0 = _d(x3) @ _d(w0).t()
    z_err = 3 * U * (_d(x3).abs() @ _d(w0).abs().t())
    return z0, elu64(z0), z_err + ELU_FACTOR * elu_abs_error(z0.float(), lift=True), z_err


def lift_stats_chain(rows):
    """lift_stats_kernel: min(ceil(rows / 256), 2048) blocks, a wave adds every fourth row of its block in sequence, then the waves"""
    nblk = min(cdiv(rows, 256), BN_MAX_BLOCKS)
    return cdiv(cdiv(rows, nblk), 4) + 3


def ref_lift_second(e0, e0_err, bn0, w1, bn1, rows_chain, eps):
    """z1 = y0 W1^T, y0 = a0 (e0 - mu0) + beta0 with the GIVEN constants (4 roundings as ref_on_load, plus |a0| err_e0); one rounding
    per channel of the first layer.  bn1 given: y1 = a1 (elu(z1) - mu1) + beta1, 4 more roundings and the epilogue's ELU.
    The statistics are those of elu(z1) (stats_bounds)."""
    g0, b0, m0, i0 = [_d(t) for t in bn0]
    a0 = g0 * i0
    y0 = a0 * (e0 - m0) + b0
    ymag = a0.abs() * (e0.abs() + m0.abs()) + b0.abs()
    yerr = 4 * U * ymag + a0.abs() * e0_err
    w64 = _d(w1)
    z1 = y0 @ w64.t()
    z_err = e0.shape[1] * U * (ymag @ w64.abs().t()) + yerr @ w64.abs().t()
    e1 = elu64(z1)
    e_err = z_err + ELU_FACTOR * elu_abs_error(z1.float(), lift=True)
    out = dict(z1=z1, z1_err=z_err, y0=y0, y0_mag=ymag, y0_err=yerr)
    if bn1 is not None:
        g1, b1, m1, i1 = [_d(t) for t in bn1]
        a1 = g1 * i1
        out["y1"] = a1 * (e1 - m1) + b1
        out["y1_err"] = 4 * U * (a1.abs() * (e1.abs() + m1.abs()) + b1.abs()) + a1.abs() * e_err
    mean, var, invstd, d_mean, d_var, d_invstd = stats_bounds(e1, e_err, rows_chain, eps)
    out.update(mean=mean, var=var, invstd=invstd, d_mean=d_mean, d_var=d_var, d_invstd=d_invstd)
    return out


def ref_lift_bwd_autograd(x3, w0, gamma0, beta0, w1, dz1, eps):
    """fp64 autograd of z1 = BN0_batch(elu(x3 W0^T)) W1^T with the upstream dz1, the batch statistics inside the graph.
    Returns grad_w1, dgamma0, dbeta0, grad_w0 (c0, 3), mean0, invstd0"""
    w0r, g0r, b0r, w1r = [_d(t).clone().requires_grad_(True) for t in (w0, gamma0, beta0, w1)]
    e0 = torch.nn.functional.elu(_d(x3) @ w0r.t())
    mean = e0.mean(0)
    var = (e0 * e0).mean(0) - mean * mean
    invstd = 1.0 / torch.sqrt(var + eps)
    z1 = ((e0 - mean) * invstd * g0r + b0r) @ w1r.t()
    gw0, gg0, gb0, gw1 = torch.autograd.grad(z1, (w0r, g0r, b0r, w1r), _d(dz1))
    return gw1, gg0, gb0, gw0, mean.detach(), invstd.detach()


def lift_bwd_bounds(x3, w0, bn0, w1, dz1, rows_chain, wgrad_chain):
    """Error bounds of hf_lift_elu_bn_bwd against ref_lift_bwd_autograd when the kernel is given the reference's mean0 / invstd0
    rounded to fp32 (2 more roundings on y0 and xhat0).  With dy0 = dz1 W1 (c1 roundings on D = |dz1| |W1|), xhat0 = (e0 - mu0) invstd0
    (2 roundings + the given constants' 2, on X = (|e0| + |mu0|) invstd0, plus invstd0 err_e0 =: err_x), s = elu'(z0) = exp(min(z0, 0))
    (measured like the ELU; its argument's error scales it by at most err_z0):
      grad_w1  as ref_wgrad with the operand y0: (chain + 6) u |dz1|^T |y0|mag + |dz1|^T |a0| err_e0
      dbeta0   <= sum_r(c1 u D + chain u |dy0|) + u |dbeta0|
      dgamma0  <= sum_r(c1 u D X + (chain + 5) u |dy0| X + |dy0| err_x) + u |dgamma0|
      dz0 = a0 (dy0 - dbeta0 / R - xhat0 dgamma0 / R) s: 10 roundings on Z = |a0| (|dy0| + |dbeta0| / R + X |dgamma0| / R) s, plus
            |a0| s (c1 u D + d_dbeta0 / R + X d_dgamma0 / R + err_x |dgamma0| / R) + (Z / s) err_s
      grad_w0  <= sum_r((err_dz0 + (chain + 1) u |dz0|mag) |x3|) + u |grad_w0|      (fp64 across workgroups)"""
    rows = x3.shape[0]
    g0, b0, m0, i0 = [_d(t) for t in bn0]
    a0 = g0 * i0
    z0, e0, e_err, z_err = ref_lift_first(x3, w0)
    e_err = e_err + 2 * U * (e0.abs() + m0.abs())
    ymag = a0.abs() * (e0.abs() + m0.abs()) + b0.abs()
    g64, w64, x64 = _d(dz1), _d(w1), _d(x3)
    c1 = dz1.shape[1]
    d_w1 = (wgrad_chain + 6) * U * (g64.abs().t() @ ymag) + g64.abs().t() @ (a0.abs() * e_err)
    dy0 = g64 @ w64
    dmag = g64.abs() @ w64.abs()
    dy_err = c1 * U * dmag
    xmag = (e0.abs() + m0.abs()) * i0
    xhat = (e0 - m0) * i0
    x_err = i0 * e_err
    dbeta, dgamma = dy0.sum(0), (dy0 * xhat).sum(0)
    d_dbeta = (dy_err + rows_chain * U * dy0.abs()).sum(0) + U * dbeta.abs()
    d_dgamma = (dy_err * xmag + (rows_chain + 5) * U * dy0.abs() * xmag + dy0.abs() * x_err).sum(0) + U * dgamma.abs()
    s = torch.exp(z0.clamp(max=0))
    neg = z0.float().cpu()
    neg = neg[neg <= 0]
    s_meas = float((torch.exp(neg).double() - torch.exp(neg.double())).abs().max()) if neg.numel() else 0.0
    s_err = ELU_FACTOR * s_meas + s * z_err
    zmag = a0.abs() * (dy0.abs() + dbeta.abs() / rows + xmag * dgamma.abs() / rows)
    dz0_err = 10 * U * zmag * s + a0.abs() * s * (dy_err + d_dbeta / rows + xmag * d_dgamma / rows + x_err * dgamma.abs() / rows) + zmag * s_err
    gw0 = ((a0 * (dy0 - dbeta / rows - xhat * dgamma / rows) * s).t() @ x64)
    d_w0 = (dz0_err + (rows_chain + 1) * U * zmag * s).t() @ x64.abs() + U * gw0.abs()
    return dict(d_w1=d_w1, d_dbeta=d_dbeta, d_dgamma=d_dgamma, d_w0=d_w0)
