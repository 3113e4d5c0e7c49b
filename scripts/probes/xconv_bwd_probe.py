"""Diagnostic: the two X-Conv backward kernels alone, through the folded entry hf_xconv_depthwise_gather_bn_grad, at two layer shapes
of rpn_multiclass at 8 frames:

  dec5  b 8, 16384 table rows and 16384 rows per cloud, K 8, c0 64, c1 256, M 1
  enc0  the same clouds, c1 1, M 4

Each shape is called once for grad_f + grad_wd (xconv_dw_bwd_fw_kernel<K, M, true, true>: the BN = true instantiation, then the
partial_rows_sum / finalize kernels) and once for grad_x
(xconv_bn_bwd_x_kernel), ITERS times each after one warm-up call.  Run it
  - under `rocprofv3 --kernel-trace --stats` for per-kernel durations, or
  - under `rocprofv3 --pmc SQ_INSTS_VALU SQ_INSTS_SALU SQ_BUSY_CYCLES SQ_WAVE_CYCLES` (a run of its own, no tracing) for the
    instruction counts and cycles per kernel (scripts/parse_pmc.py averages a counter per kernel).
HFOPS_LIBRARY selects the build.  Real kNN tables on bench.kitti_frustum clouds, seeded normals elsewhere."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import heterofusionrcnn_amd as hf  # noqa: E402,F401
from heterofusionrcnn_amd import _lib  # noqa: E402
from heterofusionrcnn_amd._lib import check, ptr, stream_ptr  # noqa: E402
from heterofusionrcnn_amd.grouping import index_inverse, knn_point  # noqa: E402
from bench import kitti_frustum  # noqa: E402

ITERS = int(os.environ.get("XCONV_BWD_PROBE_ITERS", "3"))
SHAPES = (("dec5", 64, 256, 1), ("enc0", 64, 1, 4))
B, N, K = 8, 16384, 8


def main():
    L = _lib.lib()
    print("library:", _lib.LIB_PATH, flush=True)
    rng = np.random.default_rng(1000)
    xyz = torch.from_numpy(kitti_frustum(rng, B, N)).cuda()
    _, idx = knn_point(K, xyz, xyz)
    idx = idx.contiguous()
    off, ent = index_inverse(idx, N)
    gen = torch.Generator(device="cuda").manual_seed(7)
    normal = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    for name, c0, c1, m in SHAPES:
        c = c0 + c1
        x, z1, fts = normal(B * N, K, K), normal(B * N * K, c0), normal(B * N, c1)
        wd, go = normal(K, c, m), normal(B * N, c * m)
        gamma, beta, mean, invstd = 1 + 0.1 * normal(c0), 0.1 * normal(c0), 0.1 * normal(c0), 1 + 0.1 * normal(c0).abs()
        gx, gf, gw = torch.empty_like(x), torch.empty_like(z1), torch.empty_like(wd)
        dg, db = torch.empty(c0, device="cuda"), torch.empty(c0, device="cuda")
        nbytes = L.hf_xconv_depthwise_gather_bn_grad_workspace(B, N, K, c0, c1, m)
        ws = torch.empty((nbytes // 4,), dtype=torch.float32, device="cuda")

        def call(want_x):
            check(L.hf_xconv_depthwise_gather_bn_grad(B, N, N, K, c0, c1, m, ptr(x), ptr(z1), ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                                      ptr(fts), ptr(idx), ptr(wd), ptr(go), ptr(off), ptr(ent), ptr(gx) if want_x else None,
                                                      None if want_x else ptr(gf), None, None if want_x else ptr(gw), ptr(dg), ptr(db),
                                                      ptr(ws), nbytes, stream_ptr()), name)

        for want_x in (False, True):
            for _ in range(1 + ITERS):
                call(want_x)
            torch.cuda.synchronize()
        print("%s: c0 %d c1 %d m %d, %d calls of each kernel" % (name, c0, c1, m, 1 + ITERS), flush=True)
        del x, z1, fts, wd, go, gx, gf, gw, ws
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
