"""KITTI object evaluation (2D, BEV and 3D AP) on the device: the scoring step of the reference's offline evaluator,
scripts/offline_eval/kitti_native_eval/evaluate_object_3d_offline.cpp (and the _05_iou twin), which
hf/core/evaluator_utils.py:283-330 runs after every checkpoint.

Parsing and packing are host code; the overlaps, the matching passes, the thresholds and the precision arrays are one call of
hf_kitti_eval (csrc/kitti_eval.hip).  There is no CPU path.

    python -m heterofusionrcnn_amd.kitti_eval GT_DIR RESULT_DIR [--05-iou] [--out DIR]

Deviations from the reference, all on inputs it mishandles: a label line with other than 15 columns or a result line with other
than 16 raises ValueError (the reference's fscanf loop desynchronises), a NaN score raises ValueError (the reference sorts
scores with std::sort), and more than HF_KITTI_MAX_GT label rows or HF_KITTI_MAX_DET detections in one frame raise ValueError.
"""
import argparse
import os
import re
import sys

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr, require, stream_ptr

CLASSES = ("car", "pedestrian", "cyclist")
METRICS = ("image", "bev", "3d")
DIFFICULTIES = ("easy", "moderate", "hard")
TYPE_CODES = {"car": 0, "pedestrian": 1, "cyclist": 2, "van": 3, "person_sitting": 4, "dontcare": 5}
TYPE_OTHER = 6
MAX_GT, MAX_DET, COLS, STEPS = 128, 512, 13, 41
MIN_OVERLAP = {
    "kitti": np.array([[0.7, 0.5, 0.5]] * 3),                                   # evaluate_object_3d_offline.cpp:55
    "05_iou": np.array([[0.7, 0.5, 0.5], [0.5, 0.25, 0.25], [0.5, 0.25, 0.25]]),  # the _05_iou variant
}
_SUFFIX = ("", "_BEV", "_3D")


# ------------------------------------------------------------------------------------------------ parsing

def _parse(path, ncols):
    """(types, values): values (n, ncols - 1) float64, the numeric columns in file order"""
    types, rows = [], []
    with open(path) as f:
        for lineno, line in enumerate(f, 1):
            parts = line.split()
            if not parts:
                continue
            if len(parts) != ncols:
                raise ValueError("%s:%d: expected %d columns, got %d" % (path, lineno, ncols, len(parts)))
            try:
                vals = [float(v) for v in parts[1:]]
                int(parts[2])                                          # occlusion is read with %d
            except ValueError:
                raise ValueError("%s:%d: malformed line" % (path, lineno))
            types.append(parts[0])
            rows.append(vals)
    return types, np.asarray(rows, dtype=np.float64).reshape(-1, ncols - 1)


def read_gt(path):
    """A label_2 file -> (types, (n, 14) float64): truncated occluded alpha x1 y1 x2 y2 h w l x y z ry"""
    return _parse(path, 15)


def read_results(path):
    """A result file -> (types, (n, 15) float64): the label columns + score"""
    return _parse(path, 16)


def result_files(result_dir):
    """{frame index: path} of <result_dir>/data/*.txt (the reference's layout) or else <result_dir>/*.txt, stems all digits"""
    data = os.path.join(result_dir, "data")
    d = data if os.path.isdir(data) else result_dir
    out = {}
    for name in os.listdir(d):
        m = re.fullmatch(r"(\d+)\.txt", name)
        if m and os.path.isfile(os.path.join(d, name)):
            out[int(m.group(1))] = os.path.join(d, name)
    return out


def load_dirs(gt_dir, result_dir):
    """(indices, gt_frames, det_frames) for every frame that has a result file, sorted by index"""
    files = result_files(result_dir)
    if not files:
        raise ValueError("%s: no result files" % result_dir)
    idx = sorted(files)
    gts, dets = [], []
    for i in idx:
        gpath = os.path.join(gt_dir, "%06d.txt" % i)
        if not os.path.isfile(gpath):
            raise ValueError("%s: ground truth missing" % gpath)
        gts.append(read_gt(gpath))
        dets.append(read_results(files[i]))
    return idx, gts, dets


# ------------------------------------------------------------------------------------------------ packing

def type_code(name):
    return TYPE_CODES.get(name.lower(), TYPE_OTHER)


class Packed:
    """The frames in the CSR form hf_kitti_eval takes (host arrays)"""

    def __init__(self, gt_off, det_off, gt, gt_type, gt_occ, det, det_type, eval_mask, compute_aos):
        self.gt_off, self.det_off = gt_off, det_off
        self.gt, self.gt_type, self.gt_occ = gt, gt_type, gt_occ
        self.det, self.det_type = det, det_type
        self.eval_mask, self.compute_aos = eval_mask, compute_aos

    @property
    def n_frames(self):
        return len(self.gt_off) - 1

    def pair_off(self):
        n = np.diff(self.gt_off) * np.diff(self.det_off)
        return np.concatenate([[0], np.cumsum(n)]).astype(np.int64)

    def validate(self):
        """the checks the device cannot make: consistent offsets, per-frame caps, no NaN score"""
        for name, off, rows in (("gt", self.gt_off, self.gt), ("det", self.det_off, self.det)):
            require(isinstance(off, np.ndarray) and off.dtype == np.int64 and off.ndim == 1 and len(off) >= 2,
                    "%s offsets must be an int64 vector of n_frames + 1 entries" % name)
            require(off[0] == 0 and off[-1] == len(rows) and (np.diff(off) >= 0).all(),
                    "%s offsets do not match the %d rows" % (name, len(rows)))
            require(rows.ndim == 2 and rows.shape[1] == COLS and rows.dtype == np.float64, "%s rows must be (n, %d) float64" % (name, COLS))
        require(len(self.gt_off) == len(self.det_off), "gt and det offsets describe different frame counts")
        require(len(self.gt_type) == len(self.gt) and len(self.gt_occ) == len(self.gt) and len(self.det_type) == len(self.det),
                "type / occlusion vectors do not match the rows")
        ng, nd = np.diff(self.gt_off), np.diff(self.det_off)
        require(ng.max(initial=0) <= MAX_GT, "a frame has %d label rows; at most %d are supported" % (ng.max(initial=0), MAX_GT))
        require(nd.max(initial=0) <= MAX_DET, "a frame has %d detections; at most %d are supported" % (nd.max(initial=0), MAX_DET))
        require(not np.isnan(self.det[:, 12]).any(), "a detection score is NaN")


def pack_frames(gt_frames, det_frames):
    """per-frame (types, values) as read_gt / read_results return them -> Packed, with the reference's load-time flags"""
    require(len(gt_frames) == len(det_frames), "%d ground-truth frames but %d result frames" % (len(gt_frames), len(det_frames)))
    require(len(gt_frames) > 0, "no frames to evaluate")
    gt_rows, gt_type, gt_occ, det_rows, det_type = [], [], [], [], []
    gt_n, det_n = [], []
    compute_aos = True
    evalm = np.zeros((3, 3), bool)
    for (gtypes, gv), (dtypes, dv) in zip(gt_frames, det_frames):
        gv = np.asarray(gv, dtype=np.float64).reshape(-1, 14)
        dv = np.asarray(dv, dtype=np.float64).reshape(-1, 15)
        require(len(gtypes) == len(gv) and len(dtypes) == len(dv), "type names do not match the rows")
        # label columns: trunc occ alpha x1 y1 x2 y2 h w l x y z ry (+ score)
        g = np.empty((len(gv), COLS))
        g[:, 0:4], g[:, 4], g[:, 5:12], g[:, 12] = gv[:, 3:7], gv[:, 2], gv[:, 7:14], gv[:, 0]
        d = np.empty((len(dv), COLS))
        d[:, 0:4], d[:, 4], d[:, 5:12], d[:, 12] = dv[:, 3:7], dv[:, 2], dv[:, 7:14], dv[:, 14]
        gt_rows.append(g)
        det_rows.append(d)
        gt_type += [type_code(t) for t in gtypes]
        gt_occ += [int(v) for v in gv[:, 1]]
        dcodes = [type_code(t) for t in dtypes]
        det_type += dcodes
        gt_n.append(len(gv))
        det_n.append(len(dv))
        if (dv[:, 2] == -10).any():
            compute_aos = False
        for c, r in zip(dcodes, d):                                   # evaluate_object_3d_offline.cpp:158-168
            if c < 3:
                h, w, l, t1, t2, t3 = r[5:11]
                evalm[0, c] |= bool(r[0] >= 0)
                evalm[1, c] |= bool(t1 != -1000 and t3 != -1000 and w > 0 and l > 0)
                evalm[2, c] |= bool(t1 != -1000 and t2 != -1000 and t3 != -1000 and h > 0 and w > 0 and l > 0)
    off = lambda n: np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    mask = sum(1 << (m * 3 + c) for m in range(3) for c in range(3) if evalm[m, c])
    return Packed(off(gt_n), off(det_n), np.concatenate(gt_rows).reshape(-1, COLS), np.asarray(gt_type, np.int32),
                  np.asarray(gt_occ, np.int32), np.concatenate(det_rows).reshape(-1, COLS), np.asarray(det_type, np.int32),
                  mask, compute_aos)


def overlap_table(min_overlap):
    if isinstance(min_overlap, str):
        require(min_overlap in MIN_OVERLAP, "min_overlap must be 'kitti', '05_iou' or a 3x3 table, got %r" % min_overlap)
        return MIN_OVERLAP[min_overlap].copy()
    t = np.asarray(min_overlap, dtype=np.float64)
    require(t.shape == (3, 3), "min_overlap must be a 3x3 table [metric][class], got shape %s" % (t.shape,))
    require(np.isfinite(t).all() and (t >= 0).all() and (t < 1).all(), "min_overlap entries must lie in [0, 1)")
    return t


# ------------------------------------------------------------------------------------------------ device calls

def _dev(a, dtype, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)


def _require_device(device):
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("kitti_eval runs on the GPU: heterofusionrcnn_amd has no CPU implementation")
    return device


def _upload(p, device):
    t = {"gt_off": _dev(p.gt_off, torch.int64, device), "det_off": _dev(p.det_off, torch.int64, device),
         "pair_off": _dev(p.pair_off(), torch.int64, device),
         "gt": _dev(p.gt, torch.float64, device), "det": _dev(p.det, torch.float64, device),
         "gt_type": _dev(p.gt_type, torch.int32, device), "gt_occ": _dev(p.gt_occ, torch.int32, device),
         "det_type": _dev(p.det_type, torch.int32, device)}
    return t


def _sizes(p):
    return (p.n_frames, len(p.gt), len(p.det), int(p.pair_off()[-1]), int(np.diff(p.gt_off).max()), int(np.diff(p.det_off).max()))


def compute_overlaps(p, device="cuda"):
    """(n_pairs, 6) float64 on the device: hf_kitti_eval_overlaps of a Packed set"""
    device = _require_device(device)
    p.validate()
    frames, n_gt, n_det, n_pairs, max_gt, max_det = _sizes(p)
    t = _upload(p, device)
    out = torch.empty((n_pairs, 6), dtype=torch.float64, device=device)
    check(_lib.lib().hf_kitti_eval_overlaps(frames, ptr(t["gt_off"]), ptr(t["det_off"]), ptr(t["pair_off"]), n_gt, n_det, n_pairs,
                                            max_gt, max_det, ptr(t["gt"]), ptr(t["det"]), ptr(out), stream_ptr()),
          "kitti_eval_overlaps")
    return out


def evaluate_packed(p, min_overlap="kitti", device="cuda"):
    """One hf_kitti_eval call and one host read -> the raw arrays, each (3, 3, 3, ...) [metric][class][difficulty]"""
    table = overlap_table(min_overlap)
    p.validate()
    device = _require_device(device)
    frames, n_gt, n_det, n_pairs, max_gt, max_det = _sizes(p)
    L = _lib.lib()
    t = _upload(p, device)
    ovt = _dev(table, torch.float64, device)
    ws_bytes = L.hf_kitti_eval_workspace(frames, n_gt, n_pairs)
    ws = torch.empty((max(ws_bytes, 8) // 8,), dtype=torch.int64, device=device)
    # every output is a slice of one buffer: one copy to the host
    n = 27 * STEPS
    sizes = [("thresholds", torch.float64, n), ("precision", torch.float64, n), ("aos", torch.float64, n),
             ("aos_ground", torch.float64, n), ("counts", torch.int32, n * 3), ("n_thresholds", torch.int32, 27)]
    nbytes = [k * (8 if dt == torch.float64 else 4) for _, dt, k in sizes]
    blob = torch.empty((sum(nbytes),), dtype=torch.uint8, device=device)
    views, o = {}, 0
    for (name, dt, k), b in zip(sizes, nbytes):
        views[name] = blob[o:o + b].view(dt)
        o += b
    check(L.hf_kitti_eval(frames, ptr(t["gt_off"]), ptr(t["det_off"]), ptr(t["pair_off"]), n_gt, n_det, n_pairs, max_gt, max_det,
                          ptr(t["gt"]), ptr(t["gt_type"]), ptr(t["gt_occ"]), ptr(t["det"]), ptr(t["det_type"]), ptr(ovt),
                          p.eval_mask, int(p.compute_aos), ptr(views["thresholds"]), ptr(views["n_thresholds"]),
                          ptr(views["counts"]), ptr(views["precision"]), ptr(views["aos"]), ptr(views["aos_ground"]), ptr(ws),
                          ws_bytes, stream_ptr()), "kitti_eval")
    host = blob.cpu().numpy()
    out, o = {}, 0
    for (name, dt, k), b in zip(sizes, nbytes):
        arr = host[o:o + b].view(np.float64 if dt == torch.float64 else np.int32)
        out[name] = arr.reshape((3, 3, 3, STEPS, 3) if name == "counts" else (3, 3, 3) if name == "n_thresholds" else (3, 3, 3, STEPS))
        o += b
    out["min_overlap"] = table
    return out


# ------------------------------------------------------------------------------------------------ results

def ap11(vals):
    """printAp: the samples 0, 4, ..., 40 summed in a float accumulator, then / 11 * 100 in float"""
    s = np.float32(0)
    for i in range(0, STEPS, 4):
        s = np.float32(np.float64(s) + vals[i])
    return np.float32(np.float32(s / np.float32(11)) * np.float32(100))


def ap_r40(vals):
    """AP|R40 (not part of the reference's output): precision[1..40] / 40 * 100 in float64"""
    s = 0.0
    for i in range(1, STEPS):
        s += float(vals[i])
    return s / 40 * 100


def _finish(raw, compute_aos, eval_mask):
    res = dict(raw)
    res["compute_aos"] = bool(compute_aos)
    res["evaluated"] = [(METRICS[m], CLASSES[c]) for m in range(3) for c in range(3) if (eval_mask >> (m * 3 + c)) & 1]
    ap = np.zeros((3, 3, 3), np.float32)
    ap40 = np.zeros((3, 3, 3))
    ori = np.zeros((3, 3, 3), np.float32)
    for m in range(3):
        for c in range(3):
            for d in range(3):
                ap[m, c, d] = ap11(raw["precision"][m, c, d])
                ap40[m, c, d] = ap_r40(raw["precision"][m, c, d])
                ori[m, c, d] = ap11(raw["aos"][m, c, d] if m == 0 else raw["aos_ground"][m, c, d])
    res["ap"], res["ap_r40"], res["ap_orientation"] = ap, ap40, ori
    return res


def evaluate_frames(gt_frames, det_frames, min_overlap="kitti", device="cuda"):
    """In-memory frames: gt_frames[i] = (type names, (n, 14) label columns), det_frames[i] = (type names, (n, 15) with the
    score last), frame i of both the same image.  Returns the dict of evaluate_dirs (without file output)."""
    p = pack_frames(gt_frames, det_frames)
    return _finish(evaluate_packed(p, min_overlap, device), p.compute_aos, p.eval_mask)


def report_lines(result):
    """The reference's AP lines, in its order (image, then BEV, then 3D; classes in order within each)"""
    ev = set(result["evaluated"])
    lines = []
    fmt = lambda name, v: "%s AP: %f %f %f" % ((name,) + tuple(float(x) for x in v))
    for m in range(3):
        for c, cls in enumerate(CLASSES):
            if (METRICS[m], cls) not in ev:
                continue
            lines.append(fmt(cls + "_detection" + _SUFFIX[m], result["ap"][m, c]))
            if m == 0 and result["compute_aos"]:
                lines.append(fmt(cls + "_orientation", result["ap_orientation"][m, c]))
            elif m > 0:
                lines.append(fmt(cls + "_heading" + _SUFFIX[m], result["ap_orientation"][m, c]))
    return lines


def format_report(result):
    return "".join(l + "\n" for l in report_lines(result))


def write_plots(result, out_dir):
    """plot/<cls>_detection{,_BEV,_3D}.txt (and <cls>_orientation.txt with AOS): "%f %f %f %f" = recall, easy, moderate, hard"""
    plot = os.path.join(out_dir, "plot")
    os.makedirs(plot, exist_ok=True)
    ev = set(result["evaluated"])
    for m in range(3):
        for c, cls in enumerate(CLASSES):
            if (METRICS[m], cls) not in ev:
                continue
            files = [(cls + "_detection" + _SUFFIX[m], result["precision"][m, c])]
            if m == 0 and result["compute_aos"]:
                files.append((cls + "_orientation", result["aos"][m, c]))
            for name, vals in files:
                with open(os.path.join(plot, name + ".txt"), "w") as f:
                    for i in range(STEPS):
                        f.write("%f %f %f %f\n" % (i / (STEPS - 1.0), vals[0, i], vals[1, i], vals[2, i]))


def evaluate_dirs(gt_dir, result_dir, min_overlap="kitti", out_dir=None, device="cuda"):
    """Evaluate every <index>.txt of result_dir (or result_dir/data) against gt_dir/<index:06d>.txt.

    Returns a dict; arrays are indexed [metric (image, bev, 3d)][class (car, pedestrian, cyclist)][difficulty]:
      ap (3,3,3) float32 as printed, ap_r40 (3,3,3) float64 (AP|R40, not part of the reference's output),
      ap_orientation (3,3,3) float32 (orientation for the image metric, heading for BEV / 3D),
      precision / aos / aos_ground (3,3,3,41), thresholds (3,3,3,41), n_thresholds (3,3,3), counts (3,3,3,41,3) tp fp fn,
      evaluated [(metric, class)], compute_aos, frames (the evaluated indices), min_overlap (3,3)."""
    idx, gts, dets = load_dirs(gt_dir, result_dir)
    res = evaluate_frames(gts, dets, min_overlap, device)
    res["frames"] = idx
    if out_dir is not None:
        write_plots(res, out_dir)
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m heterofusionrcnn_amd.kitti_eval", description=__doc__.split("\n\n")[0])
    ap.add_argument("gt_dir")
    ap.add_argument("result_dir")
    ap.add_argument("--05-iou", dest="iou05", action="store_true", help="MIN_OVERLAP 0.5 / 0.25 for BEV and 3D")
    ap.add_argument("--out", default=None, help="also write plot/*.txt here")
    a = ap.parse_args(argv)
    res = evaluate_dirs(a.gt_dir, a.result_dir, "05_iou" if a.iou05 else "kitti", a.out)
    sys.stdout.write(format_report(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
