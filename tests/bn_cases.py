"""Case table, restated dispatch rule, fp64 references and bounds of the kernel-level parity suite of csrc/mlp.hip
(tests/test_bn_abi.py runs the cases on the GPU through the C ABI, tests/test_bn_instantiations_cpu.py checks on any machine
that the cases reach every compiled kernel of mlp.hip).  A plain helper module: nothing here imports the library.

Dispatch rule, restated from mlp.hip (NOT imported; the line numbers are those of the file at this commit):
  bn_geom (mlp.hip:33-51)            vec = 4 if c % 4 == 0 else 1; cv = c / vec; rpb = 1 if cv >= 256 else 256 / cv; threads = cv * rpb;
                                     nblk = min(ceil(rows / (8 rpb)), kBnMaxBlocks); rows_per_block = ceil(ceil(rows / nblk) / rpb) * rpb;
                                     nblk = ceil(rows / rows_per_block)
  kBnMaxBlocks (hf_common.h:31)      2048 partial columns per channel: the cap on nblk above
  bn_small_geom (mlp.hip:501-520)    the single-launch route: c % 4 == 0, rows <= 4096, not (rows > 2048 and c > 128); a workgroup of
                                     <= 256 (rows <= 1024) or 512 threads owns cvw <= 8 channel vectors and ALL rows, 8 rows per thread.
                                     Taken by hf_bn_relu_fwd_train[_ld] and hf_bn_relu_bwd[_ld] only
  bn_finalize_wide (mlp.hip:196-203) nblk > 256: one 256-thread workgroup per channel instead of one wave (same kernel, other grid)
  bn_nt_fwd / bn_nt_bwd (:980-982)   streaming (non-temporal) loads when 4 rows c > 200 MiB (forward) or 8 rows c > 200 MiB (backward);
                                     16-byte form without dropout only (launch_bn_stats, BnApplyL, BnReduceL, BnDxL, :909-977)
  bn_dispatch (mlp.hip:895-905)      <VEC, ELU, DROP> = (vec, relu & 2, a dropout entry point)
  pool (mlp.hip:1184-1250)           forward / backward reduce: bn_geom(groups, c) over groups; dz pass: bn_geom(groups k, c) over rows;
                                     training statistics: bn_stats_kernel<vec, false, nt> on groups k rows
  narrow linear (mlp.hip:1157-1168)  bn_geom(rows, cin): narrow_linear_dx_kernel<vec>
  channel limit (mlp.hip:983-988)    c <= 4096, and c <= 1024 when c % 4 != 0: there a workgroup has cv = c threads per row, and the launch
                                     of more than 1024 threads is refused by the runtime; launch_limit_ok() restates it and the CPU guard
                                     checks every 1 <= c <= 4096 against it.  No case launches an over-limit geometry

Two families, as in tests/gemm_cases.py.
EXACT: small-integer inputs (x >= 0 where the ELU runs, so that it is the identity; elu(0) = exp2(0) - 1 = 0 and its slope 1 are exact),
integer means / gamma / beta and power-of-two invstd where the statistics are inputs.  Every sum is an integer (or a dyadic fraction)
below 2^24, so the result equals fp64 bit for bit whatever the order.  Per entry point:
  hf_bn_stats, training forward   sum x, sum x^2 exact in fp32, reduced, divided and square-rooted in fp64 by the kernel: save_mean and
                                  save_invstd equal the same fp64 formula rounded once.  momentum = 1/4 and quarter-integer running
                                  estimates: (1 - m) r + m float(batch) is exact in fp64 and rounded once by the kernel's last addition
                                  as long as m float(var) is exact, which it is (a power-of-two scale).  y is compared within 4 u M of
                                  fp64 evaluated with the kernel's own save_mean / save_invstd (they are not dyadic, so y cannot be exact)
  hf_bn_relu_fwd_eval             y exact (a = gamma invstd, x - mean, the product and the sum are small dyadic numbers)
  hf_bn_relu_bwd[_ld]             dbeta, dgamma exact; dx exact where rows is a power of two (1 / rows exact), else within the rounding
                                  bound of fp64 evaluated with the kernel's own dbeta / dgamma; dx_colsum against the fp64 sum of the
                                  kernel's dx (exact where rows is a power of two)
  hf_bn_relu_bwd_dx               dx exact: dgamma = dbeta = 0 unless rows is a power of two (then multiples of rows)
  hf_bn_dropout_*                 gamma = 0, beta = 2: y is 2 scale where kept and 0 where dropped, i.e. the mask, compared element for
                                  element with the numpy restatement below; backward: dx = 0 exactly (gamma = 0), dbeta = sum of the kept
                                  dy scale, exact for the power-of-two scales (rate 0, 0.5), within bound otherwise
  hf_bn_relu_maxpool_*            eval form: pooled and argmax exact (ties: pre-activations of exactly 0 and repeated rows, first
                                  maximum wins); training form: statistics as above, pooled within bound, argmax exact; backward as
                                  hf_bn_relu_bwd
  hf_narrow_linear_dx             exact
The exact family carries the deliberate ties: pre-activations of exactly 0 (the mask is `> 0` in every pass).

ROUND: seeded normals with non-trivial constants, every element within c u M of fp64, u = 2^-24, M the magnitude sum of the terms,
c the number of fp32 roundings on the longest path; the sums: a thread adds its T = rows_per_block / rpb rows in sequence, thread 0 of a
channel adds the other rpb - 1 partials (reduce_rows), everything after that is fp64: chain = T + rpb - 1 (sum_chain); short-tensor
route: 8 rows per thread + 6 shuffle steps.  Rounding-error terms use gamma_n = n u / (1 - n u).
  variance    var = E[x^2] - mean^2 in ONE pass: |d var| <= (chain + 1) u E[x^2] + 2 |mean| chain u E|x| <= (3 chain + 1) u E[x^2]
              (|mean| <= E|x| <= sqrt(E[x^2])).  That is the one-pass envelope c u E[x^2]: relative to the variance it grows with
              1 + (mean / std)^2.  The mean/std = 30 channel of every rounding-family statistics case must stay inside it.
  y           a (e - mu) + beta: a = gamma invstd (1), the difference (1), the product (1), the sum (1): 4 u M, M = |a| (|e| + |mu|) + |beta|,
              against fp64 evaluated with the kernel's own statistics; continuous at 0, so the ReLU needs no margin
  backward    ref_bn_bwd derives its counts; the masks need a margin: inputs whose fp64 pre-activation lies within RELU_MARGIN of zero are
              moved away before the call (nudge_off_relu_threshold of gemm_cases) and the margin is asserted on the reference
  ELU         the one constant that cannot be read from the code: exp(x) - 1 on the hardware exponential (elu_stream: exp2(x log2 e),
              elu_hw: __expf).  |d elu| <= ELU_C u (exp(x) + 1) for x <= 0: exp(x) + 1 is the magnitude sum of the two terms of
              exp(x) - 1 (relative to |elu(x)| itself the error is unbounded near 0: the subtraction cancels; at x = -1e-9 the kernel
              returns 0 and |got - ref| / (u |ref|) is 2^24).  MEASURED on an MI355X (profiles/bn_parity.md): worst |got - ref64| / (u (exp(x) + 1))
              over the ELU-on-load elements of the cases, read through hf_bn_relu_fwd_eval with gamma = invstd = 1, mean = beta = 0
              (y = elu(x) with no other rounding) = ELU_MEASURED = 0.837; ELU_C = 2 is the next power of two at or above twice that.
              Nothing else has a measured tolerance.

Dropout (mlp.hip:117-146, :255-264), restated here in integer arithmetic: the seed of a call is splitmix64 of
drop_state[0] + salt 0xbf58476d1ce4e5b9 + call number 0x9e3779b97f4a7c15; the keep bits of vector number v = row cv + cvec come from
h1 = mix32((lo32(v) ^ lo32(seed)) + mix32(hi32(v) ^ hi32(seed))) and, for vec = 4, h2 = mix32(h1 ^ 0x68bc21eb): 16 bits per element, kept
iff bits >= thresh = min(int(rate 65536 + 0.5), 65535).  The vector index is 64 bits wide because rows cv passes 2^32 for tensors the
entry points accept (rows is a long long: 2^32 scalar-width elements are 16 GiB): with a 32-bit index the rows beyond would repeat the
mask of the rows before (the hi32 term is what separates them), and a product formed in 32 bits would do so silently.  A device case of
that size cannot run in a few seconds; drop_keep() takes the row offset as an argument, and the CPU guard checks that rows 2^32 / cv
apart draw different masks in the restatement, which the device cases pin to the kernel at every size they run."""
import numpy as np
import torch

from gemm_cases import (RELU_MARGIN, U, cdiv, ints, nudge_off_relu_threshold, nudge_share_ok, relu_margin,  # noqa: F401
                        running_bounds)

BN_MAX_BLOCKS = 2048
ROWS_PER_THREAD = 8
UNROLL = 4
FINALIZE_WIDE_FROM = 256
NT_BYTES = 200 << 20
SMALL_MAX_ROWS = 4096
MAX_CHANNELS, MAX_SCALAR_CHANNELS = 4096, 1024
NARROW_MAX_OUT = 4
ELU_MEASURED = 0.837         # worst |got - ref64| / (u (exp(x) + 1)) on an MI355X, profiles/bn_parity.md
ELU_C = 2.0                 # next power of two >= 2 * ELU_MEASURED
EPS = 1e-3


def gam(n):
    return n * U / (1.0 - n * U)


# ---------------------------------------------------------------------------------------------- restated launch geometry
def geom(rows, c):
    vec = 4 if c % 4 == 0 else 1
    cv = c // vec
    rpb = 1 if cv >= 256 else 256 // cv
    nblk = max(1, min(cdiv(rows, rpb * ROWS_PER_THREAD), BN_MAX_BLOCKS))
    rpbk = cdiv(cdiv(rows, nblk), rpb) * rpb
    return dict(vec=vec, cv=cv, rpb=rpb, threads=cv * rpb, nblk=cdiv(rows, rpbk), rows_per_block=rpbk)


def small_geom(rows, c):
    """the single-launch route's geometry, or None where the streaming route runs"""
    if c % 4 != 0 or rows > SMALL_MAX_ROWS or (rows > 2048 and c > 128):
        return None
    cv, cvw = c // 4, 8
    tmax = 256 if rows <= 1024 else 512
    while cvw > 1 and (cvw > cv or cvw * rows > tmax * ROWS_PER_THREAD):
        cvw >>= 1
    want = min(rows, tmax // cvw)
    threads = min((want * cvw + 63) // 64 * 64, tmax)
    rpb = threads // cvw
    if rpb * ROWS_PER_THREAD < rows:
        return None
    return dict(cvw=cvw, threads=threads, rpb=rpb, nwg=cdiv(cv, cvw))


def launch_limit_ok(c):
    """what the entry points accept: the restated bn_channels_ok"""
    return 0 < c <= MAX_CHANNELS and (c % 4 == 0 or c <= MAX_SCALAR_CHANNELS)


def finalize_wide(nblk):
    return nblk > FINALIZE_WIDE_FROM


def nt_fwd(rows, c):
    return 4 * rows * c > NT_BYTES


def nt_bwd(rows, c):
    return 8 * rows * c > NT_BYTES


def sum_chain(rows, c, small=False):
    """fp32 additions on the longest path into one per-block partial"""
    if small:
        return ROWS_PER_THREAD + 6
    g = geom(rows, c)
    return g["rows_per_block"] // g["rpb"] + g["rpb"] - 1


# ---------------------------------------------------------------------------------------------- the case table
STREAM4 = ((4097, 8), (33000, 64), (2100, 1024), (16391, 1024), (8192, 8))     # the last: 1 / rows exact on the streaming route
STREAM1 = ((300, 7), (4099, 1), (1500, 1023), (9, 3), (1, 3), (2, 5))
SMALL = ((1, 4), (2, 8), (33, 256), (7, 4096), (1024, 64), (1025, 64), (4096, 4), (4095, 12), (4096, 128), (2048, 132), (4096, 64))
STRADDLE = (((2048, 132), (2049, 132)), ((4096, 64), (4097, 64)))
NT_SHAPES = (((12803, 4096), 1), ((819211, 64), 2))
AT_NT_FWD, AT_NT_BWD = (12800, 4096), (6400, 4096)          # exactly 200 MiB: not streaming-load by the rule (>)
POOLS = ((1, 1, 4), (333, 17, 5), (50, 255, 24), (600, 32, 64))
NARROWS = ((1, 1, 1), (3000, 7, 3), (4099, 76, 2), (257, 4096, 4))
DROP_RATES = (0.0, 0.25, 0.5, 0.99999, 0.999995)            # the last one reaches the clamp of the threshold to 65535
DROP_SHAPES = ((4097, 8), (300, 7))


def _case(kind, **kw):
    kw["kind"] = kind
    kw.setdefault("family", "exact")
    return kw


def case_id(c):
    return "-".join([c["kind"], c["family"]] + ["%s%s" % (k, v) for k, v in c.items() if k not in ("kind", "family")])


def _shape_cases():
    out = []
    shapes = STREAM4 + STREAM1 + SMALL + tuple(p[1] for p in STRADDLE)
    for i, (rows, c) in enumerate(shapes):
        for relu in (0, 1, 2, 3):
            rounding = relu in (1, 2) or i % 4 == relu
            for fam in ("exact", "round") if rounding else ("exact",):
                out.append(_case("train", rows=rows, c=c, relu=relu, ld=0, family=fam))
                out.append(_case("bwd", rows=rows, c=c, relu=relu, ld=0, colsum=int((i + relu) % 2 == 0), family=fam))
        if small_geom(rows, c) is None or (rows, c) in ((1024, 64), (7, 4096)):     # entry points without a short-tensor route
            for relu in (0, 1, 2, 3):
                fams = ("exact", "round") if relu in (1, 2) else ("exact",)
                for fam in fams:
                    out.append(_case("eval", rows=rows, c=c, relu=relu, family=fam))
                    out.append(_case("bwd_dx", rows=rows, c=c, relu=relu, family=fam))
            for fam in ("exact", "round"):
                out.append(_case("stats", rows=rows, c=c, family=fam))
    return out


def _stride_cases():
    out = []
    for rows, c in ((4097, 8), (1024, 64), (33, 256)):                  # streaming and short-tensor route, vec = 4
        for ld in (c + 4, 3 * c):
            for relu, fam in ((1, "exact"), (2, "exact"), (1, "round")):
                out.append(_case("train", rows=rows, c=c, relu=relu, ld=ld, family=fam))
                out.append(_case("bwd", rows=rows, c=c, relu=relu, ld=ld, colsum=1, family=fam))
    for relu, fam in ((1, "exact"), (2, "exact"), (1, "round")):         # vec = 1: streaming route only
        out.append(_case("train", rows=300, c=7, relu=relu, ld=8, family=fam))
        out.append(_case("bwd", rows=300, c=7, relu=relu, ld=8, colsum=0, family=fam))
    return out


def _nt_cases():
    out = []
    for (rows, c), relu in NT_SHAPES:
        out += [_case("train", rows=rows, c=c, relu=relu, ld=0), _case("eval", rows=rows, c=c, relu=relu),
                _case("bwd", rows=rows, c=c, relu=relu, ld=0, colsum=1), _case("bwd_dx", rows=rows, c=c, relu=relu),
                _case("train", rows=rows, c=c, relu=relu, ld=0, family="round"), _case("bwd", rows=rows, c=c, relu=relu, ld=0, colsum=0, family="round")]
    out.append(_case("stats", rows=NT_SHAPES[0][0][0], c=NT_SHAPES[0][0][1]))
    out += [_case("train", rows=AT_NT_FWD[0], c=AT_NT_FWD[1], relu=1, ld=0), _case("bwd", rows=AT_NT_BWD[0], c=AT_NT_BWD[1], relu=1, ld=0, colsum=0)]
    return out


def _pool_cases():
    return [_case("pool", groups=g, k=k, c=c, training=tr, colsum=cs, family=fam)
            for g, k, c in POOLS for tr in (0, 1) for cs in (0, 1) for fam in ("exact", "round")]


def _narrow_cases():
    return [_case("narrow", rows=r, cin=ci, cout=co, family=fam) for r, ci, co in NARROWS for fam in ("exact", "round")]


def _drop_cases():
    out = []
    for rows, c in DROP_SHAPES:
        for rate in DROP_RATES:
            for salt in (0, 3):
                out.append(_case("drop", rows=rows, c=c, relu=1, rate=rate, salt=salt))
        for relu in (0, 2, 3):
            out.append(_case("drop", rows=rows, c=c, relu=relu, rate=0.25, salt=0))
        for relu in (1, 2):
            out.append(_case("drop", rows=rows, c=c, relu=relu, rate=0.25, salt=3, family="round"))
    out.append(_case("drop", rows=33000, c=64, relu=3, rate=0.5, salt=3))           # wide finalize writes the seed
    out.append(_case("drop", rows=33000, c=64, relu=1, rate=0.25, salt=0, family="round"))
    return out


def all_cases():
    return _shape_cases() + _stride_cases() + _nt_cases() + _pool_cases() + _narrow_cases() + _drop_cases()


def cases_of(*kinds):
    return [c for c in all_cases() if c["kind"] in kinds]


# ---------------------------------------------------------------------------------------------- which kernels a case launches
def instantiations(c):
    """the (kernel, template arguments) a case launches by the dispatch rule in the module docstring"""
    k = c["kind"]
    if k == "narrow":
        return {("narrow_linear_dx_kernel", (geom(c["rows"], c["cin"])["vec"],))}
    if k == "pool":
        rows, vec = c["groups"] * c["k"], geom(c["groups"], c["c"])["vec"]
        out = {("bn_pool_fwd_kernel", (vec,)), ("bn_pool_bwd_reduce_kernel", (vec,)), ("bn_bwd_finalize_kernel", ()), ("bn_pool_bwd_dx_kernel", (vec,))}
        if c["training"]:
            out |= {("bn_stats_kernel", (vec, False, vec == 4 and nt_fwd(rows, c["c"]))), ("bn_stats_finalize_kernel", ())}
        if c["colsum"]:
            out.add(("bn_colsum_finalize_kernel", ()))
        return out
    rows, ch = c["rows"], c["c"]
    vec = geom(rows, ch)["vec"]
    elu = bool(c.get("relu", 0) & 2)
    ntf, ntb = vec == 4 and nt_fwd(rows, ch), vec == 4 and nt_bwd(rows, ch)
    if k == "stats":
        return {("bn_stats_kernel", (vec, False, ntf)), ("bn_stats_finalize_kernel", ())}
    if k == "train":
        if small_geom(rows, ch):
            return {("bn_small_fwd_kernel", ())}
        return {("bn_stats_kernel", (vec, elu, ntf)), ("bn_stats_finalize_kernel", ()), ("bn_apply_kernel", (vec, elu, False, ntf))}
    if k == "eval":
        return {("bn_apply_kernel", (vec, elu, False, ntf))}
    if k == "bwd":
        if small_geom(rows, ch):
            return {("bn_small_bwd_kernel", ())}
        out = {("bn_bwd_reduce_kernel", (vec, elu, False, ntb)), ("bn_bwd_finalize_kernel", ()), ("bn_bwd_dx_kernel", (vec, elu, False, ntb))}
        if c["colsum"]:
            out.add(("bn_colsum_finalize_kernel", ()))
        return out
    if k == "bwd_dx":
        return {("bn_bwd_dx_kernel", (vec, elu, False, ntb))}
    if k == "drop":                 # the dropout forms never take the streaming loads
        return {("bn_stats_kernel", (vec, elu, ntf)), ("bn_stats_finalize_kernel", ()), ("bn_apply_kernel", (vec, elu, True, False)),
                ("bn_bwd_reduce_kernel", (vec, elu, True, False)), ("bn_bwd_finalize_kernel", ()), ("bn_bwd_dx_kernel", (vec, elu, True, False))}
    raise KeyError(k)


def selected_instantiations(cases=None):
    out = set()
    for c in (all_cases() if cases is None else cases):
        out |= instantiations(c)
    return out


def case_threads(c):
    """threads per workgroup of every streaming launch of the case (the CPU guard: <= 1024)"""
    if c["kind"] == "narrow":
        return [geom(c["rows"], c["cin"])["threads"]]
    if c["kind"] == "pool":
        return [geom(c["groups"], c["c"])["threads"], geom(c["groups"] * c["k"], c["c"])["threads"]]
    return [geom(c["rows"], c["c"])["threads"]]


# ---------------------------------------------------------------------------------------------- inputs
def _seed(c):
    s = 23
    for k in sorted(c):
        if k == "family":
            continue
        for ch in (str(k) + "=" + str(c[k])):
            s = (s * 131 + ord(ch)) % 2147483629
    return s


class Draw:
    """seeded draws on the tensor's own device (the streaming-load shapes are 50 M elements: generated where they are used)"""

    def __init__(self, c, dev):
        self.dev = dev
        self.g = torch.Generator(device=dev).manual_seed(_seed(c))

    def ints(self, shape, lo, hi):
        return torch.randint(lo, hi + 1, shape, generator=self.g, device=self.dev).float()

    def normal(self, shape, mean=0.0, std=1.0):
        return torch.randn(shape, generator=self.g, device=self.dev) * std + mean

    def uniform(self, shape, lo, hi):
        return torch.rand(shape, generator=self.g, device=self.dev) * (hi - lo) + lo

    def pow2(self, shape):
        return 2.0 ** self.ints(shape, -1, 1)


ELU_EDGES = (-100.0, -20.0, -1e-6, 0.0, 30.0)


def make_x(d, rows, c, exact, elu):
    """EXACT: integers in [-2, 2] ([0, 2] under the ELU).  ROUND: N(0.3, 1), channel 0 constant over the rows, channel 1 with
    mean / std = 30, and under the ELU the inputs ELU_EDGES in the first rows of the last channel"""
    if exact:
        return d.ints((rows, c), 0 if elu else -2, 2)
    x = d.normal((rows, c), 0.3, 1.0)
    x[:, 0] = 1.5
    if c > 1:
        x[:, 1] = d.normal((rows,), 30.0, 1.0)
    if elu and c > 2:
        n = min(rows, len(ELU_EDGES))
        x[:n, c - 1] = torch.tensor(ELU_EDGES[:n], device=x.device)
    return x


def given_stats(d, c, exact):
    """(gamma, beta, mean, invstd) where the statistics are inputs"""
    if exact:
        return d.ints((c,), -2, 2), d.ints((c,), -2, 2), d.ints((c,), -1, 1), d.pow2((c,))
    return d.uniform((c,), 0.5, 1.5) * torch.where(d.uniform((c,), 0, 1) < 0.25, -1.0, 1.0), d.uniform((c,), -0.5, 0.5), d.normal((c,), 0.3, 0.5), \
        1.0 / d.uniform((c,), 0.5, 1.5)


def affine(d, c, exact):
    """(gamma, beta) of the training forms"""
    if exact:
        return d.ints((c,), -2, 2), d.ints((c,), -2, 2)
    return d.uniform((c,), 0.5, 1.5), d.uniform((c,), -0.5, 0.5)


def pre_activation(x, gamma, beta, mean, invstd, relu):
    e, _ = elu64(x, relu & 2)
    return _d(gamma) * _d(invstd) * (e - _d(mean)) + _d(beta)


def nudge(x, gamma, beta, mean, invstd, relu):
    """moves the inputs whose fp64 pre-activation lies within 1.1 RELU_MARGIN of zero upwards, in place, until none is left (under the ELU
    a step in x is a smaller step in elu(x)); the tests assert the margin on the reference afterwards.  Returns the share moved"""
    near = pre_activation(x, gamma, beta, mean, invstd, relu).abs() < 1.1 * RELU_MARGIN
    share = float(near.double().mean())
    for step in (0.01, 0.05, 0.25, 1.0):
        if not bool(near.any()):
            break
        x[near] = x[near] + step
        near = pre_activation(x, gamma, beta, mean, invstd, relu).abs() < 1.1 * RELU_MARGIN
    return share


def margin(x, gamma, beta, mean, invstd, relu):
    return float(pre_activation(x, gamma, beta, mean, invstd, relu).abs().min())


# ---------------------------------------------------------------------------------------------- fp64 references
def _d(t):
    return None if t is None else t.double()


def elu64(x, on):
    """(elu(x), |error| of the kernel's exp(x) - 1) in fp64; identity with zero error when the ELU is off.  Positive inputs pass
    through unchanged (exact)"""
    x = _d(x)
    if not on:
        return x, torch.zeros_like(x)
    neg = x <= 0
    e = torch.where(neg, torch.expm1(x.clamp(max=0)), x)
    err = torch.where(neg, ELU_C * U * (torch.exp(x.clamp(max=0)) + 1.0), torch.zeros_like(x))
    return e, err


def ref_stats(x, elu, chain, eps, exact):
    """batch statistics of e = elu?(x) and their bounds (module docstring): returns mean, var, invstd, d_mean, d_var, d_invstd.
    exact: the sums carry no error, what is left is the cast of each result (the tests then compare bit for bit instead)"""
    e, err = elu64(x, elu)
    rows = e.shape[0]
    mean = e.sum(0) / rows
    ex2 = (e * e).sum(0) / rows
    var = (ex2 - mean * mean).clamp(min=0)
    eps64 = float(np.float32(eps))
    invstd = 1.0 / torch.sqrt(var + eps64)
    if exact:
        return mean, var, invstd, U * mean.abs(), U * var, 2 * U * invstd
    d_mean = gam(chain) * e.abs().mean(0) + err.mean(0) + U * mean.abs()
    d_var = one_pass_envelope(x, elu, chain) + U * var
    lo = (var - d_var).clamp(min=0)
    d_invstd = 0.5 * (lo + eps64) ** -1.5 * d_var + 2 * U * invstd
    return mean, var, invstd, d_mean, d_var, d_invstd


def one_pass_envelope(x, elu, chain):
    """the documented c u E[x^2], c = 3 chain + 1: (chain + 1) u E[x^2] from the sum of squares, 2 |mean| chain u E|x| <= 2 chain u E[x^2] from
    the square of the mean; 1e-3 of it covers the second-order terms (chain u < 1e-4).  Where the ELU runs, its own error enters both sums:
    E[2 |e| err + err^2] + 2 |mean| E[err]"""
    e, err = elu64(x, elu)
    return (3 * chain + 1) * U * 1.001 * (e * e).mean(0) + (2 * e.abs() * err + err * err).mean(0) + 2 * e.mean(0).abs() * err.mean(0)


def ref_apply(x, gamma, beta, mean, invstd, relu, mult=None, mult_roundings=0):
    """y = [mult] relu?(a (elu?(x) - mean) + beta) with the given statistics: 4 roundings on M = |a| (|e| + |mean|) + |beta|, plus
    |a| err_elu; mult (dropout: 0 or scale) one more and the roundings of the scale itself.  Returns y, bound"""
    e, err = elu64(x, relu & 2)
    a = _d(gamma) * _d(invstd)
    h = a * (e - _d(mean)) + _d(beta)
    if relu & 1:
        h = h.clamp(min=0)
    bound = gam(4) * (a.abs() * (e.abs() + _d(mean).abs()) + _d(beta).abs()) + a.abs() * err
    if mult is not None:
        h, bound = h * mult, (bound + gam(1 + mult_roundings) * h.abs()) * mult.abs()
    return h, bound


def ref_bn_bwd(x, dy, gamma, beta, mean, invstd, relu, chain, mult=None, mult_roundings=0):
    """dbeta = sum dh, dgamma = sum dh xhat with dh = [mult] dy under the ReLU mask (a (e - mean) + beta > 0), xhat = (e - mean) invstd
    (2 roundings on X = (|e| + |mean|) invstd, plus invstd err_elu); a term dh xhat is 3 roundings (+ those of mult), the sum `chain` more,
    the cast of the total one:
      |d dbeta|  <= gamma(chain + m) sum |dh| + u |dbeta|
      |d dgamma| <= gamma(chain + 3 + m) sum |dh| X + sum |dh| invstd err_elu + u |dgamma|
    Returns a dict with dh, xhat, X, the ELU slope s and its error, the sums and their bounds"""
    e, err = elu64(x, relu & 2)
    g, b, mu, inv = _d(gamma), _d(beta), _d(mean), _d(invstd)
    a = g * inv
    dh = _d(dy) if mult is None else _d(dy) * mult
    m = 0 if mult is None else 1 + mult_roundings
    if relu & 1:
        dh = torch.where(a * (e - mu) + b > 0, dh, torch.zeros_like(dh))
    xhat, xmag = (e - mu) * inv, (e.abs() + mu.abs()) * inv
    dbeta, dgamma = dh.sum(0), (dh * xhat).sum(0)
    x64 = _d(x)
    slope = torch.where(x64 > 0, torch.ones_like(x64), torch.exp(x64.clamp(max=0))) if relu & 2 else torch.ones_like(x64)
    return dict(e=e, err=err, a=a, inv=inv, dh=dh, xhat=xhat, xmag=xmag, slope=slope, slope_err=(err + U) * (x64 <= 0) if relu & 2 else torch.zeros_like(x64),
                dbeta=dbeta, dgamma=dgamma, m=m,
                d_dbeta=gam(chain + m) * dh.abs().sum(0) + U * dbeta.abs(),
                d_dgamma=gam(chain + 3 + m) * (dh.abs() * xmag).sum(0) + (dh.abs() * inv * err).sum(0) + U * dgamma.abs())


def ref_bn_dx(r, dgamma, dbeta, rows):
    """dx = a (dh - dbeta / R - xhat dgamma / R) [slope] with the GIVEN dgamma / dbeta (the kernel's own, or the caller's): 1 / R, the
    two products with it, xhat (2), xhat c2, the two differences, a, the product, [mult], [slope]: 11 + m roundings on
    Z = |a| (|dh| + |dbeta| / R + X |dgamma| / R) |s|, plus |a| invstd err_elu |dgamma| / R |s| and Z err_slope / |s|.  Returns dx, bound"""
    dg, db = _d(dgamma), _d(dbeta)
    core = r["a"] * (r["dh"] - db / rows - r["xhat"] * dg / rows)
    z = r["a"].abs() * (r["dh"].abs() + db.abs() / rows + r["xmag"] * dg.abs() / rows)
    elu_term = r["a"].abs() * r["inv"] * r["err"] * dg.abs() / rows
    return core * r["slope"], (gam(11 + r["m"]) * z + elu_term) * r["slope"] + z * r["slope_err"]


def ref_colsum(dx_got, chain):
    """column sums of the kernel's own dx values (the same registers it stored): `chain` roundings and the cast"""
    s = _d(dx_got).sum(0)
    return s, gam(chain) * _d(dx_got).abs().sum(0) + U * s.abs()


def ref_narrow(g, w):
    """dx = g W: cout rounded products, cout - 1 sums, the longest path through cout roundings"""
    cout = g.shape[1]
    return _d(g) @ _d(w), gam(cout) * (_d(g).abs() @ _d(w).abs())


# ---------------------------------------------------------------------------------------------- dropout, restated
M64 = (1 << 64) - 1


def drop_seed(state0, salt, call):
    """splitmix64 of base seed, salt and the number of this forward call (1 for the first)"""
    z = (state0 + salt * 0xbf58476d1ce4e5b9 + call * 0x9e3779b97f4a7c15) & M64
    z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M64
    z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M64
    return z ^ (z >> 31)


def _mix32(h):
    h = h.astype(np.uint32)
    h ^= h >> np.uint32(16)
    h *= np.uint32(0x7feb352d)
    h ^= h >> np.uint32(15)
    h *= np.uint32(0x846ca68b)
    h ^= h >> np.uint32(16)
    return h


def drop_threshold(rate):
    """(thresh, scale) as drop_args forms them in fp32"""
    r = np.float32(rate)
    thresh = min(int(r * np.float32(65536.0) + np.float32(0.5)), 65535)
    return thresh, np.float32(1.0) / (np.float32(1.0) - r)


def drop_keep(rows, c, seed, thresh, row0=0):
    """boolean (rows, c): the elements of rows row0 .. row0 + rows - 1 that the kernels keep"""
    vec = 4 if c % 4 == 0 else 1
    cv = c // vec
    with np.errstate(over="ignore"):
        v = (np.arange(rows, dtype=np.uint64)[:, None] + np.uint64(row0)) * np.uint64(cv) + np.arange(cv, dtype=np.uint64)[None, :]
        s0, s1 = np.uint32(seed & 0xffffffff), np.uint32(seed >> 32)
        lo, hi = (v & np.uint64(0xffffffff)).astype(np.uint32), (v >> np.uint64(32)).astype(np.uint32)
        h1 = _mix32((lo ^ s0) + _mix32(hi ^ s1))
        if vec == 1:
            bits = (h1 & np.uint32(0xffff))[:, :, None]
        else:
            h2 = _mix32(h1 ^ np.uint32(0x68bc21eb))
            bits = np.stack([h1 & np.uint32(0xffff), h1 >> np.uint32(16), h2 & np.uint32(0xffff), h2 >> np.uint32(16)], axis=2)
    return (bits >= np.uint32(thresh)).reshape(rows, c)
