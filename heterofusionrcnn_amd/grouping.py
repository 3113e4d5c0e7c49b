"""grouping ops -- same surface as the reference's grouping/tf_grouping.py:11-95."""
import torch

from . import _lib
from ._lib import check, dev_tensor, ptr, require, stream_ptr
from .determinism import record, refuse_unordered


BALL_QUERY_VARIANTS = {"auto": 0, "cell": 1, "bruteforce": 2, "sorted": 3}   # HF_BQ_* of include/hfops.h


def _ball_query(variant, b, n, m, radius, nsample, xyz1, xyz2, center, idx, cnt, grouped):
    """hf_query_ball_group_xyz_ws with a workspace from the caching allocator (on the current stream)"""
    L = _lib.lib()
    v = BALL_QUERY_VARIANTS[variant]
    ws, nbytes = None, 0
    # the cell-sorted pair needs a workspace; 'auto' takes it from 32 clouds and more than one round of query tiles only
    # (launch_ball_query, grouping.hip), so smaller calls do not allocate b * (16 n + 64 KB) bytes for nothing
    if v == 3 or (v == 0 and b >= 32 and b * ((m + 127) // 128) > 256):
        nbytes = L.hf_ball_query_workspace(b, n)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=xyz1.device)
    check(L.hf_query_ball_group_xyz_ws(v, b, n, m, radius, nsample, ptr(xyz1), ptr(xyz2), 1 if center else 0, ptr(idx), ptr(cnt),
                                       ptr(grouped), ptr(ws), nbytes, stream_ptr()), "query_ball_point")


def query_ball_point(radius, nsample, xyz1, xyz2, variant="auto"):
    """xyz1 (B,N,3) data, xyz2 (B,M,3) queries -> idx (B,M,nsample) int32, pts_cnt (B,M) int32.
    Reference: tf_grouping.py:11-23; non-differentiable (:26).  Rows without any hit are zeros
    (undefined in the reference, tf_grouping.cpp:88).  variant forces one of the kernels (BALL_QUERY_VARIANTS): same output."""
    radius, nsample = float(radius), int(nsample)
    require(radius > 0, "QueryBallPoint expects positive radius")
    require(nsample > 0, "QueryBallPoint expects positive nsample")
    require(xyz1.dim() == 3 and xyz1.shape[2] == 3, "QueryBallPoint expects (batch_size, ndataset, 3) xyz1 shape.")
    require(xyz2.dim() == 3 and xyz2.shape[2] == 3, "QueryBallPoint expects (batch_size, npoint, 3) xyz2 shape.")
    require(xyz1.shape[0] == xyz2.shape[0], "QueryBallPoint expects xyz1 and xyz2 with the same batch_size")
    xyz1 = dev_tensor(xyz1.detach(), torch.float32, "xyz1")
    xyz2 = dev_tensor(xyz2.detach(), torch.float32, "xyz2")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    idx = torch.empty((b, m, nsample), dtype=torch.int32, device=xyz1.device)
    cnt = torch.empty((b, m), dtype=torch.int32, device=xyz1.device)
    _ball_query(variant, b, n, m, radius, nsample, xyz1, xyz2, False, idx, cnt, None)
    return idx, cnt


def gather_rows_into(points, idx, out, col):
    """out[..., col:col+C] = points[idx] for points (B,N,C), idx (B,M,K) and out (B,M,K,width) contiguous: the gather written
    straight into a column slice of wider rows (hf_group_point_into)"""
    b, n, c = points.shape
    _, m, ns = idx.shape
    check(_lib.lib().hf_group_point_into(b, n, c, m, ns, out.shape[-1], col, ptr(points), ptr(idx), ptr(out), stream_ptr()),
          "group_point_into")


def gather_rows_grad(grad_out, col, idx, n, c, inverse=None, ctx=None):
    """the gradient of that gather w.r.t. points, (B,N,C), read in place from columns col.. of grad_out (B,M,K,width) contiguous:
    by the inverse index (offsets, entries) = index_inverse(idx, N) where it came with the geometry -- every row written once,
    no atomics -- else scattered with atomics into a zero-filled target (ctx: the calling Function's, whose forward recorded the
    deterministic mode: under it the scatter is refused)"""
    b, m, ns = idx.shape
    width = grad_out.shape[-1]
    g = torch.empty((b, n, c), dtype=torch.float32, device=grad_out.device)
    if inverse is not None:
        offsets, entries = inverse
        check(_lib.lib().hf_group_point_grad_gather(b, n, c, m, ns, width, col, ptr(grad_out), ptr(offsets), ptr(entries), ptr(g),
                                                    stream_ptr()), "group_point_grad_gather")
    else:
        if ctx is not None:
            refuse_unordered("gather_rows_grad", "no inverse index: n = %d, index_inverse takes up to %d targets" % (n, INVERSE_MAX_TARGETS), ctx)
        check(_lib.lib().hf_group_point_grad_from(b, n, c, m, ns, width, col, ptr(grad_out), ptr(idx), ptr(g), stream_ptr()),
              "group_point_grad_from")
    return g


class _GroupPoint(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx):
        b, n, c = points.shape
        _, m, ns = idx.shape
        out = torch.empty((b, m, ns, c), dtype=torch.float32, device=points.device)
        # dense rows: hf_group_point also has the form for power-of-two widths, which the column-slice entry does not take
        check(_lib.lib().hf_group_point(b, n, c, m, ns, ptr(points), ptr(idx), ptr(out), stream_ptr()), "group_point")
        record(ctx)
        ctx.save_for_backward(idx)
        ctx.shape = (b, n, c)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        b, n, c = ctx.shape
        return gather_rows_grad(grad_out.contiguous(), 0, idx, n, c, ctx=ctx), None


def group_point(points, idx):
    """points (B,N,C), idx (B,M,K) int32 -> (B,M,K,C).  Reference: tf_grouping.py:44-59
    (gradient w.r.t. points only)."""
    require(points.dim() == 3, "GroupPoint expects (batch_size, num_points, channel) points shape")
    require(idx.dim() == 3 and idx.shape[0] == points.shape[0],
            "GroupPoint expects (batch_size, npoints, nsample) idx shape")
    points = dev_tensor(points, torch.float32, "points")
    idx = dev_tensor(idx, torch.int32, "idx")
    return _GroupPoint.apply(points, idx)


INVERSE_MAX_TARGETS = 19968


def index_inverse(idx, n):
    """idx (B,M,K) int32 with values in [0, n) -> (offsets (B,n+1), entries (B,M*K)) int32: for every data point the flat
    (query*K + slot) positions that name it, ascending.  Coordinates-only, so it is prepared with the geometry
    (pipeline.GeometryPrefetcher); the gradient of group_point / concat_group then gathers instead of scattering atomics."""
    idx = dev_tensor(idx, torch.int32, "idx")
    require(idx.dim() == 3, "index_inverse expects (b,m,k) idx shape")
    require(0 < n <= INVERSE_MAX_TARGETS, "index_inverse expects 0 < n <= %d" % INVERSE_MAX_TARGETS)
    b, m, k = idx.shape
    offsets = torch.empty((b, n + 1), dtype=torch.int32, device=idx.device)
    entries = torch.empty((b, m * k), dtype=torch.int32, device=idx.device)
    check(_lib.lib().hf_index_inverse(b, m * k, n, ptr(idx), ptr(offsets), ptr(entries), stream_ptr()), "index_inverse")
    return offsets, entries


class _ConcatGroup(torch.autograd.Function):
    """[head | points[idx]]: the gathered part is written straight into the concat buffer and its gradient is read out
    of the concat's gradient in place (hf_group_point_into / hf_group_point_grad_from); only `head` is copied"""

    @staticmethod
    def forward(ctx, head, points, idx, offsets, entries):
        b, n, c = points.shape
        _, m, ns = idx.shape
        ch = head.shape[-1]
        out = torch.empty((b, m, ns, ch + c), dtype=torch.float32, device=points.device)
        out[..., :ch].copy_(head)
        gather_rows_into(points, idx, out, ch)
        record(ctx)
        ctx.save_for_backward(idx, *([offsets, entries] if offsets is not None else []))
        ctx.shape = (b, n, c, ch)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        idx = ctx.saved_tensors[0]
        b, n, c, ch = ctx.shape
        grad_out = grad_out.contiguous()
        g = None
        if ctx.needs_input_grad[1]:   # with the inverse index of the geometry: gather, every row written once
            g = gather_rows_grad(grad_out, ch, idx, n, c, ctx.saved_tensors[1:] or None, ctx=ctx)
        return (grad_out[..., :ch] if ctx.needs_input_grad[0] else None), g, None, None, None


def concat_group(head, points, idx, inverse=None):
    """torch.cat([head, group_point(points, idx)], -1) for head (B,M,K,Ch), points (B,N,C), idx (B,M,K);
    inverse = index_inverse(idx, N) (optional): the gradient w.r.t. points gathers instead of using atomics"""
    require(head.dim() == 4 and points.dim() == 3 and idx.dim() == 3 and head.shape[:3] == idx.shape,
            "concat_group expects head (B,M,K,Ch), points (B,N,C), idx (B,M,K)")
    points = dev_tensor(points, torch.float32, "points")
    idx = dev_tensor(idx, torch.int32, "idx")
    offsets, entries = inverse if inverse is not None else (None, None)
    return _ConcatGroup.apply(head, points, idx, offsets, entries)


class _GroupConcat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, points, idx, grouped_xyz, width, xyz_last):
        b, n, c = points.shape
        _, m, ns = idx.shape
        out = torch.empty((b, m, ns, width), dtype=torch.float32, device=points.device)
        check(_lib.lib().hf_group_concat(b, n, c, m, ns, width, int(xyz_last), ptr(grouped_xyz), ptr(points), ptr(idx),
                                         ptr(out), stream_ptr()), "group_concat")
        ctx.save_for_backward(idx)
        ctx.shape = (b, n, c, width, int(xyz_last))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (idx,) = ctx.saved_tensors
        b, n, c, width, xyz_last = ctx.shape
        _, m, ns = idx.shape
        grad_out = grad_out.contiguous()
        g = torch.empty((b, n, c), dtype=torch.float32, device=grad_out.device)
        check(_lib.lib().hf_group_concat_grad(b, n, c, m, ns, width, xyz_last, ptr(grad_out), ptr(idx), ptr(g),
                                              stream_ptr()), "group_concat_grad")
        return g, None, None, None, None


def group_concat(points, idx, grouped_xyz, width=None, xyz_last=False):
    """[grouped_xyz, group_point(points, idx), zero padding] as one (B,M,K,width) tensor: the concat of
    sample_and_group (pointnet_util.py:58-60) without the grouped temporary; xyz_last gives the multi-scale module's
    order [features, xyz, padding] (pointnet_util.py:264).  width defaults to 3 + C rounded up to a multiple of 4.
    Gradient w.r.t. points only (coordinates are inputs)."""
    points = dev_tensor(points, torch.float32, "points")
    idx = dev_tensor(idx, torch.int32, "idx")
    grouped_xyz = dev_tensor(grouped_xyz.detach(), torch.float32, "grouped_xyz")
    require(points.dim() == 3 and idx.dim() == 3 and idx.shape[0] == points.shape[0],
            "GroupConcat expects (b,n,c) points and (b,m,k) idx")
    require(grouped_xyz.shape == (*idx.shape, 3), "GroupConcat expects (b,m,k,3) grouped_xyz")
    c = points.shape[2]
    if width is None:
        width = (3 + c + 3) // 4 * 4
    require(width >= 3 + c and width % 4 == 0, "GroupConcat expects width >= 3 + c, a multiple of 4")
    return _GroupConcat.apply(points, idx, grouped_xyz, width, bool(xyz_last))


def query_ball_group(radius, nsample, xyz1, xyz2, center=True, variant="auto"):
    """Fused query_ball_point + group_point(xyz1, idx) [- xyz2]: the op pair of
    pointnet_util.py:48-52 / 258-260 in one launch.  Returns (idx, pts_cnt, grouped_xyz);
    grouped_xyz carries the gradient of group_point w.r.t. xyz1 (and of the centring w.r.t. xyz2)
    only through the unfused ops -- use it where xyz needs no gradient (it never does in the
    reference models: coordinates are inputs)."""
    radius, nsample = float(radius), int(nsample)
    require(radius > 0, "QueryBallPoint expects positive radius")
    require(nsample > 0, "QueryBallPoint expects positive nsample")
    require(xyz1.dim() == 3 and xyz1.shape[2] == 3, "QueryBallPoint expects (batch_size, ndataset, 3) xyz1 shape.")
    require(xyz2.dim() == 3 and xyz2.shape[2] == 3, "QueryBallPoint expects (batch_size, npoint, 3) xyz2 shape.")
    require(xyz1.shape[0] == xyz2.shape[0], "QueryBallPoint expects xyz1 and xyz2 with the same batch_size")
    xyz1 = dev_tensor(xyz1.detach(), torch.float32, "xyz1")
    xyz2 = dev_tensor(xyz2.detach(), torch.float32, "xyz2")
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    idx = torch.empty((b, m, nsample), dtype=torch.int32, device=xyz1.device)
    cnt = torch.empty((b, m), dtype=torch.int32, device=xyz1.device)
    grouped = torch.empty((b, m, nsample, 3), dtype=torch.float32, device=xyz1.device)
    _ball_query(variant, b, n, m, radius, nsample, xyz1, xyz2, center, idx, cnt, grouped)
    return idx, cnt, grouped


def select_top_k(k, dist):
    """dist (B,M,N) -> (idx (B,M,N) int32, dist_out (B,M,N)); the first k of N are the k smallest.
    Reference: tf_grouping.py:29-38."""
    k = int(k)
    require(k > 0, "SelectionSort expects positive k")
    require(dist.dim() == 3, "SelectionSort expects (b,m,n) dist shape.")
    dist = dev_tensor(dist.detach(), torch.float32, "dist")
    b, m, n = dist.shape
    outi = torch.empty((b, m, n), dtype=torch.int32, device=dist.device)
    out = torch.empty((b, m, n), dtype=torch.float32, device=dist.device)
    check(_lib.lib().hf_select_top_k(b, n, m, k, ptr(dist), ptr(outi), ptr(out), stream_ptr()), "select_top_k")
    return outi, out


def knn_point(k, xyz1, xyz2, all_pairs=None, dense=False):
    """xyz1 (B,N,C) data, xyz2 (B,M,C) queries -> (val (B,M,k) squared L2 ascending, idx (B,M,k) int32).
    Reference: tf_grouping.py:62-95 (dense |q|^2 - 2 q.p^T + |p|^2 matrix + tf.nn.top_k).  For C == 3 this is
    the HIP kNN kernel (no (B,M,N) matrix; ties: lower index first): data binned into a 2-D grid + ring search for
    N <= 65536 (all_pairs=False forces it), the tiled all-pairs kernel beyond that, for tiny problems (N M <= 65536 per cloud) or
    with all_pairs=True.  Other channel counts or k > 67 RAISE
    unless dense=True is passed, which takes the reference's three-term formula in framework ops (torch.topk tie order).
    PARITY UNPINNED against the reference where it matters for ties: the reference ranks the fp32 three-term expansion
    with tf.nn.top_k, this kernel ranks (q - p)^2 summed per axis with ties to the lower index.  The neighbour sets agree
    wherever the k-th and (k+1)-th distances differ by more than the rounding of the expansion; the order among exact
    ties / near-ties has no fixture in the reference and TensorFlow is not available here."""
    k = int(k)
    require(k > 0, "knn_point expects positive k")
    require(xyz1.dim() == 3 and xyz2.dim() == 3 and xyz1.shape[0] == xyz2.shape[0] and
            xyz1.shape[2] == xyz2.shape[2], "knn_point expects (b,n,c) xyz1 and (b,m,c) xyz2")
    require(k <= xyz1.shape[1], "knn_point expects k <= ndataset")
    if xyz1.shape[2] == 3 and k <= 67:
        xyz1 = dev_tensor(xyz1.detach(), torch.float32, "xyz1")
        xyz2 = dev_tensor(xyz2.detach(), torch.float32, "xyz2")
        b, n, _ = xyz1.shape
        m = xyz2.shape[1]
        val = torch.empty((b, m, k), dtype=torch.float32, device=xyz1.device)
        idx = torch.empty((b, m, k), dtype=torch.int32, device=xyz1.device)
        L = _lib.lib()
        nbytes = L.hf_knn_workspace(b, n)
        # small clouds (the RCNN's RoI clouds: 512 x 512, 512 x 128, 128 x 32, 32 x 8 per RoI, 800 RoIs) are faster on the
        # all-pairs entry point -- its register-list kernel for k = 4 / 8 / 12 / 16 -- than through binning + ring search
        # (scripts/probes/knn_small_timing.py); both rank (q - p)^2 with ties to the lower index: same result
        all_pairs = (n * m <= 65536 or (n <= 1024 and k in (4, 8, 12, 16))) if all_pairs is None else bool(all_pairs)
        if nbytes and not all_pairs:  # grid ring-search kernels; larger clouds take the tiled all-pairs kernel
            ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=xyz1.device)
            check(L.hf_knn_point_sorted(b, n, m, k, ptr(xyz1), ptr(xyz2), ptr(val), ptr(idx), ptr(ws), nbytes, stream_ptr()),
                  "knn_point")
        else:
            check(L.hf_knn_point(b, n, m, k, ptr(xyz1), ptr(xyz2), ptr(val), ptr(idx), stream_ptr()), "knn_point")
        return val, idx
    # No shipped config reaches here (every caller searches 3-D coordinates with k <= 48).  The dense (b,m,n) form is the
    # reference's own expression in framework ops, with torch.topk's tie order -- never taken silently.
    require(dense, "knn_point: the HIP kernels cover c == 3 and k <= 67; pass dense=True to take the (b,m,n) "
                   "distance-matrix form in framework ops (torch.topk tie order, parity unpinned)")
    r1 = (xyz1 * xyz1).sum(dim=2, keepdim=True)              # (b,n,1)
    r2 = (xyz2 * xyz2).sum(dim=2, keepdim=True)              # (b,m,1)
    mul = torch.matmul(xyz2, xyz1.transpose(1, 2))           # (b,m,n)
    dist = r2 - 2 * mul + r1.transpose(1, 2)
    val, idx = torch.topk(-dist, k=k, dim=2)
    return -val, idx.to(torch.int32)
