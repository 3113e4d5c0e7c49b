"""Diagnostic: the two routes to the feature table's gradient in hf_xconv_depthwise_gather_grad, per layer shape.

  staged: xconv_dw_bwd_fw_kernel (here <K, M, true, false>: GATHER on, BN off) writes the gathered block's gradient (rows x K x c1)
          into the workspace and
          hf_group_point_grad_gather sums it per table row
  direct: xconv_dw_bwd_fts_kernel rebuilds it per table row from grad_out; xconv_dw_bwd_fw_kernel writes nothing for the gathered
          channels

Real kNN tables on bench.kitti_frustum clouds and their FPS levels: the ten gather layers of rpn_multiclass at 8 frames and at
1 frame, and the RCNN extractor's layers (128 and 512 RoIs of 512 points: 64 RoIs per frame at batch 2 and 8).  Each shape is timed through the C ABI
  - without grad_x (xconv_dw_bwd_fw_kernel + the table gradient: the sum the routing rule compares), and as the whole call,
  - with the workspace (the library's choice) and without it (always direct); xconv_dw_bwd_fts_kernel alone (only grad_fts asked for),
  - and, with the -DHF_DIAG build (scripts/probes/build_diag.sh, HFOPS_LIBRARY=.../libhfops_diag.so), with the route forced
    (HF_XDW_FTS_ROUTE = 1 staged / 2 direct).
Run it under rocprofv3 --kernel-trace --stats for per-kernel durations."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import heterofusionrcnn_amd as hf
from heterofusionrcnn_amd import _lib
from heterofusionrcnn_amd._lib import check, ptr, stream_ptr
from heterofusionrcnn_amd.grouping import index_inverse, knn_point
from bench import kitti_frustum, time_op

DIAG = "diag" in os.path.basename(_lib.LIB_PATH)
RPN = (("dec5", 16384, 16384, 64, 256, 1), ("dec4", 4096, 16384, 64, 256, 1), ("dec3", 1024, 4096, 128, 512, 1),
       ("dec2", 256, 1024, 256, 1024, 1), ("enc1", 16384, 4096, 64, 256, 1), ("dec1", 64, 256, 256, 1024, 1),
       ("enc2", 4096, 1024, 64, 256, 2), ("enc3", 1024, 256, 128, 512, 2), ("dec0", 64, 64, 256, 1280, 1), ("enc4", 256, 64, 256, 1024, 1))
RCNN = (("rcnn0", 512, 512, 4, 128, 544, 4), ("rcnn1", 512, 128, 8, 128, 512, 1), ("rcnn2", 128, 32, 12, 128, 512, 2),
        ("rcnn3", 32, 8, 12, 256, 1024, 1))


def levels(b, sizes):
    rng = np.random.default_rng(1000)
    lvl = {sizes[0]: torch.from_numpy(kitti_frustum(rng, b, sizes[0])).cuda()}
    for prev, n in zip(sizes, sizes[1:]):
        lvl[n] = hf.gather_point(lvl[prev], hf.farthest_point_sample(n, lvl[prev]))
    return lvl


def measure(name, b, lvl, n, p, k, c0, c1, m, report=True):
    L = _lib.lib()
    _, idx = knn_point(k, lvl[n], lvl[p])
    idx = idx.contiguous()
    off, ent = index_inverse(idx, n)
    c = c0 + c1
    x = torch.randn(b * p, k, k, device="cuda")
    fd = torch.randn(b * p, k, c0, device="cuda")
    fts = torch.randn(b, n, c1, device="cuda")
    wd = torch.randn(k, c, m, device="cuda")
    go = torch.randn(b * p, c * m, device="cuda")
    gx, gf, gt, gw = torch.empty_like(x), torch.empty_like(fd), torch.empty_like(fts), torch.empty_like(wd)
    nbytes = L.hf_xconv_depthwise_gather_grad_workspace(b, p, k, c0, c1, m)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device="cuda")

    def call(with_ws, with_x, table_only=False):
        check(L.hf_xconv_depthwise_gather_grad(b, n, p, k, c0, c1, m, ptr(x), ptr(fd), ptr(fts), ptr(idx), ptr(wd), ptr(go), ptr(off), ptr(ent),
                                               ptr(gx) if with_x else None, None if table_only else ptr(gf), ptr(gt),
                                               None if table_only else ptr(gw), ptr(ws) if with_ws else None,
                                               nbytes if with_ws else 0, stream_ptr()), name)

    def timed(with_ws, with_x, **env):
        for key, val in env.items():
            os.environ[key] = str(val)
        t = time_op(lambda: call(with_ws, with_x), iters=10, warm=3)
        for key in env:
            del os.environ[key]
        return round(t, 1)

    row = {"shape": name, "b": b, "n_src": n, "rows_per_cloud": p, "k": k, "c0": c0, "c1": c1, "m": m,
           "mean_list": round(p * k / n, 1), "staged_MB": round(b * p * k * c1 * 4 / 1e6, 1)}
    row["library_us"] = timed(True, False)
    row["no_workspace_us"] = timed(False, False)
    row["table_kernel_alone_us"] = round(time_op(lambda: call(False, False, True), iters=10, warm=3), 1)
    row["library_whole_call_us"] = timed(True, True)
    if DIAG:
        row["staged_us"] = timed(True, False, HF_XDW_FTS_ROUTE=1)
        row["direct_us"] = timed(True, False, HF_XDW_FTS_ROUTE=2)
        row["staged_whole_call_us"] = timed(True, True, HF_XDW_FTS_ROUTE=1)
        row["direct_whole_call_us"] = timed(True, True, HF_XDW_FTS_ROUTE=2)
    if report:
        print(json.dumps(row), flush=True)
    del x, fd, fts, wd, go, gx, gf, gt, gw, ws
    torch.cuda.empty_cache()


def main():
    print("library:", _lib.LIB_PATH, "(route forcing: %s)" % ("yes" if DIAG else "no, product build"), flush=True)
    for b in (8, 1):
        lvl = levels(b, (16384, 4096, 1024, 256, 64))
        if b == 8:      # the process's first kernels and allocations: one unreported pass over the first shape
            measure("warm-up", b, lvl, *RPN[0][1:3], 8, *RPN[0][3:], report=False)
        for name, n, p, c0, c1, m in RPN:
            measure("%s/%dframe" % (name, b), b, lvl, n, p, 8, c0, c1, m)
    for b in (128, 512):      # 64 RoIs per frame: the RCNN train step at batch 2 and 8
        lvl = levels(b, (512, 128, 32, 8))
        for name, n, p, k, c0, c1, m in RCNN:
            measure("%s/%droi" % (name, b), b, lvl, n, p, k, c0, c1, m)


if __name__ == "__main__":
    main()
