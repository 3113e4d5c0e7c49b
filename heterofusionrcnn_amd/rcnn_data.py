"""RCNN batches from KITTI files and the RPN's on-disk hand-off (hf/datasets/kitti/kitti_dataset.py:226-252 the hand-off
readers, :442-543 load_rcnn_samples; hf/core/evaluator.py:934-1035 the files export_rpn.py writes).

  hand-off       <handoff_dir>/proposals_and_scores/NAME.txt (m rows of 7 box columns + the score, %.3f),
                 <handoff_dir>/rpn_feature/NAME.npy ((P, 5 + c) float32 rows [x, y, z, intensity, fg, rpn_fts...]),
                 <handoff_dir>/proposals_iou/NAME.txt (the (m, g) 3D IoU matrix, %.3f; written, not read here)
  sample list    train: kitti_data.SampleList (every labelled frame x every combination of aug_list, default flipping and
                 pca_jitter, reshuffled per epoch); val: every frame of the split once, in order, no augmentation
  host work      a pool of `workers` threads reads each .npy payload straight into pinned staging (header parsed with
                 np.lib.format, then readinto: no intermediate array), the proposals, labels and calibration, flips the
                 proposal and GT boxes and P2 on flipped frames (kitti_data.flip_boxes_3d, flip_p2) and decodes the PNG; one
                 batch ahead of use
  device work    one copy per buffer, then hf_rcnn_batch_inputs (split of the rows, x negated on flipped frames) and
                 kitti_data.batch_image (flip, PCA jitter, 360 x 1200 resize); padded proposals (B, m, 7) with
                 proposal_count, GT (B, g, 8) [box, class 1..K] with gt_count, the resized P2 as calib

Deviations from the reference:
  (a) frames without a label of the configured classes leave the sample list up front (the reference returns a short batch):
      a fixed batch size is what lets the train step be captured;
  (b) the target layer recomputes the IoU on the device from the 3-decimal proposals instead of reading proposals_iou; it
      differs from the file only by that rounding;
  (c) P and c are read from the first .npy header and must be the same for every frame (ValueError naming the frame);
  (d) a missing hand-off file is a FileNotFoundError naming the frame;
  (e) the GT tensor is padded to max_gt columns and the proposals to the first file's row count (fixed shapes for the
      captured step); a frame with more is a ValueError naming it.
Nothing here synchronises with the device except check_status().
"""
import os

import numpy as np
import torch

from . import _lib, kitti_io
from . import kitti_data as KD
from ._lib import check, dev_tensor, ptr, require, stream_ptr
from .inference import CLASSES, rescale_p2

STATUS_BAD_FG = 1                                # include/hfops.h HF_RCNN_BATCH_BAD_FG
# the fields of the RCNN batch's meta buffer (the host views and, through kitti_data.upload_buffers, the device views)
META_DTYPES = {"img_offsets": np.int64, "wh": np.int32, "flip": np.int32, "jitter": np.int32, "proposals": np.float32,
               "proposal_count": np.int32, "gt": np.float32, "gt_count": np.int32, "calib": np.float32}
HANDOFF_DIRS = ("proposals_and_scores", "rpn_feature", "proposals_iou")


# ------------------------------------------------------------------------------------------------ device calls
def handoff_pack(xyz, intensity, fg_mask, rpn_fts):
    """hf_rpn_handoff_pack: xyz (B,P,3), intensity (B,P,1), fg_mask (B,P) bool / uint8, rpn_fts (B,P,c) -> rows (B,P,5+c)"""
    b, p, _ = xyz.shape
    c = rpn_fts.shape[-1]
    xyz = dev_tensor(xyz, torch.float32, "xyz")
    inten = dev_tensor(intensity, torch.float32, "intensity")
    fts = dev_tensor(rpn_fts, torch.float32, "rpn_fts")
    require(fg_mask.dtype in (torch.bool, torch.uint8), "fg_mask must be bool or uint8")
    fg = fg_mask.contiguous()
    require(tuple(inten.shape[:2]) == (b, p) and tuple(fg.shape) == (b, p) and tuple(fts.shape[:2]) == (b, p),
            "xyz, intensity, fg_mask and rpn_fts must share (B, P)")
    rows = torch.empty((b, p, 5 + c), dtype=torch.float32, device=xyz.device)
    check(_lib.lib().hf_rpn_handoff_pack(b, p, c, ptr(xyz), ptr(inten), ptr(fg), ptr(fts), ptr(rows), stream_ptr()),
          "rpn_handoff_pack")
    return rows


def batch_inputs(rows, flip):
    """hf_rcnn_batch_inputs: rows (B,P,5+c) float32, flip (B,) int32 -> xyz (B,P,3), intensity (B,P,1), fg_mask (B,P) bool,
    rpn_fts (B,P,c), status (B,) int32"""
    require(rows.dim() == 3 and rows.shape[2] >= 6, "rows must be (B, P, 5 + c)")
    b, p, w = rows.shape
    c = w - 5
    rows = dev_tensor(rows, torch.float32, "rows")
    flip = dev_tensor(flip, torch.int32, "flip")
    require(flip.numel() == b, "flip must be (B,)")
    dev = rows.device
    xyz = torch.empty((b, p, 3), dtype=torch.float32, device=dev)
    inten = torch.empty((b, p, 1), dtype=torch.float32, device=dev)
    fg = torch.empty((b, p), dtype=torch.bool, device=dev)
    fts = torch.empty((b, p, c), dtype=torch.float32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    check(_lib.lib().hf_rcnn_batch_inputs(b, p, c, ptr(rows), ptr(flip), ptr(xyz), ptr(inten), ptr(fg), ptr(fts), ptr(status),
                                          stream_ptr()), "rcnn_batch_inputs")
    return xyz, inten, fg, fts, status


def box3d_iou_matrix(proposals, proposal_count, gt, gt_count):
    """hf_box3d_iou_matrix: proposals (B,m,7), gt (B,g,8), counts (B,) int32 -> (B,m,g) 3D IoU, zeros in the padding"""
    require(proposals.dim() == 3 and proposals.shape[2] == 7, "proposals must be (B, m, 7)")
    require(gt.dim() == 3 and gt.shape[2] == 8 and gt.shape[0] == proposals.shape[0], "gt must be (B, g, 8)")
    b, m, _ = proposals.shape
    g = gt.shape[1]
    props = dev_tensor(proposals, torch.float32, "proposals")
    gts = dev_tensor(gt, torch.float32, "gt")
    pc = dev_tensor(proposal_count, torch.int32, "proposal_count")
    gc = dev_tensor(gt_count, torch.int32, "gt_count")
    require(pc.numel() == b and gc.numel() == b, "counts must be (B,)")
    iou = torch.zeros((b, m, g), dtype=torch.float32, device=props.device)
    check(_lib.lib().hf_box3d_iou_matrix(b, m, g, ptr(props), ptr(pc), ptr(gts) if g > 0 else None, ptr(gc), ptr(iou),
                                         stream_ptr()), "box3d_iou_matrix")
    return iou


# ------------------------------------------------------------------------------------------------ the hand-off in memory
def round_like_handoff_file(x):
    """float32 tensor (host or device) -> the float32 the second stage reads after the value went through
    proposals_and_scores/NAME.txt ("%.3f", kitti_io.save_proposals_and_scores) and back (np.loadtxt, then float32):
    rint(double(x) * 1000.0) / 1000.0 in fp64, cast to float32.  Bit for bit the file route's value, because
      - a float32 (24 significant bits) times 1000 (10 bits) has at most 34 significant bits: the product is exact in fp64;
      - rint and glibc's "%.3f" both round that exact value half to even, so both arrive at the same integer k of thousandths;
      - k / 1000.0 is the correctly rounded double of k/1000 (IEEE division), and so is what loadtxt parses from the decimal
        string, which denotes k/1000 exactly; the cast to float32 is the same on both routes;
      - a value that rounds to zero from below, such as -0.0004, is "-0.000" in the file and -0.0 here."""
    return (torch.round(x.to(torch.float64) * 1000.0) / 1000.0).to(torch.float32)


def handoff_in_memory(rpn_out, xyz, intensity, handoff_rounding=False):
    """What RpnModel.propose returned (proposals, rpn_fts, fg_mask) with the cloud it ran on -> the leading arguments of
    RcnnModel.detect as a dict (xyz, rpn_fts, intensity, fg_mask, proposals), the tensors used in place: no
    hf_rpn_handoff_pack / hf_rcnn_batch_inputs round trip and no copy of the (B,P,c) feature tensor.
    handoff_rounding: the proposals as the file route hands them over, three decimals (round_like_handoff_file); the default
    is the unrounded boxes, the better input and what two_stage.TwoStageDetector passes."""
    proposals = rpn_out["proposals"]
    if handoff_rounding:
        proposals = round_like_handoff_file(proposals)
    return {"xyz": xyz, "rpn_fts": rpn_out["rpn_fts"], "intensity": intensity, "fg_mask": rpn_out["fg_mask"], "proposals": proposals}


# ------------------------------------------------------------------------------------------------ host reading
def handoff_paths(handoff_dir, name):
    return {"proposals": os.path.join(handoff_dir, "proposals_and_scores", name + ".txt"),
            "features": os.path.join(handoff_dir, "rpn_feature", name + ".npy"),
            "iou": os.path.join(handoff_dir, "proposals_iou", name + ".txt")}


def read_npy_header(f):
    """np.lib.format header of an open .npy file -> (shape, dtype); the file is left at the start of the payload"""
    major, _ = np.lib.format.read_magic(f)
    if major == 1:
        shape, fortran, dtype = np.lib.format.read_array_header_1_0(f)
    else:
        shape, fortran, dtype = np.lib.format.read_array_header_2_0(f)
    if fortran and len(shape) > 1:
        raise ValueError("Fortran-ordered arrays are not supported")
    return tuple(shape), np.dtype(dtype)


def feature_shape(path):
    """(P, 5 + c) of a hand-off .npy (the header only)"""
    with open(path, "rb") as f:
        shape, dtype = read_npy_header(f)
    if dtype != np.dtype("<f4") or len(shape) != 2 or shape[1] < 6:
        raise ValueError("%s: expected a (P, 5 + c) float32 array, got %s %s" % (path, shape, dtype))
    return shape


def read_npy_into(path, out, shape, name):
    """the float32 payload of `path` straight into the writable buffer `out` (a numpy view of pinned memory)"""
    if not os.path.isfile(path):
        raise FileNotFoundError("frame %s: hand-off file %s is missing" % (name, path))
    with open(path, "rb") as f:
        got, dtype = read_npy_header(f)
        if got != tuple(shape) or dtype != np.dtype("<f4"):
            raise ValueError("frame %s: %s holds %s %s, the hand-off of this split is %s float32" % (name, path, got, dtype, tuple(shape)))
        mv = memoryview(out.reshape(-1).view(np.uint8))
        n = f.readinto(mv)
        if n != mv.nbytes:
            raise ValueError("frame %s: %s is truncated" % (name, path))


def read_proposals(path, name):
    if not os.path.isfile(path):
        raise FileNotFoundError("frame %s: hand-off file %s is missing" % (name, path))
    boxes, scores = kitti_io.load_proposals_and_scores(path)
    return boxes, scores


class RcnnBatch(KD.RpnBatch):
    """device tensors of one batch (xyz, intensity, fg_mask, rpn_fts, proposals, proposal_count, gt, gt_count, image, calib,
    status, noise) plus the host lists names / augs / p2 (original P2) / image_size (original (w, h)) and position (train mode)"""

    def train_inputs(self):
        """the dict graph_step.TrainStep takes with rcnn_train.rcnn_train_loss (the image in the img_fts slot, which
        rcnn_train.RcnnWithImageBranch reads)"""
        d = {k: self[k] for k in ("xyz", "rpn_fts", "intensity", "fg_mask", "proposals", "proposal_count", "gt", "gt_count", "calib")}
        d["img_fts"] = self["image"]
        return d


class KittiRcnnBatches:
    """RCNN batches of `batch` samples from <dataset_dir>/{calib,label_2,image_2} and the RPN's hand-off under handoff_dir.

      data = KittiRcnnBatches(root, handoff, "train", batch=2, seed=0)
      b = data.next()                    # device tensors, enqueued on the current stream
      step = TrainStep(trainer, opt, b.train_inputs(), None, loss_fn=rcnn_train_loss)
      ...; step(**data.next().train_inputs())

    mode="train": endless, shuffled per epoch, aug_list default (flipping, pca_jitter).  mode="val": every frame once in split
    order, no augmentation; iterate (the last batch may be short) or call next() until StopIteration.  keep_unlabelled (val
    only): frames without a label of the classes stay (gt_count 0; also frames without a label file).

    Resuming (train mode): state_dict([batch.position]) and KittiRcnnBatches(..., state=...) as kitti_data.KittiRpnBatches."""

    RNG_CALLS_PER_BATCH = 1      # hf_rpn_batch_image advances rng_state[1] by one

    def __init__(self, dataset_dir, handoff_dir, split="train", mode="train", batch=2, seed=0, aug_list=None, workers=8,
                 classes=CLASSES, img_hw=(360, 1200), max_gt=128, rank=0, world=1, keep_unlabelled=False, device=None, state=None):
        if mode not in ("train", "val"):
            raise ValueError("mode must be 'train' or 'val'")
        self.dataset_dir, self.handoff_dir, self.mode = dataset_dir, handoff_dir, mode
        self.classes, self.batch, self.img_hw, self.max_gt = list(classes), int(batch), tuple(img_hw), int(max_gt)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if mode == "train":
            aug = (KD.AUG_FLIPPING, KD.AUG_PCA_JITTER) if aug_list is None else tuple(aug_list)
            self.list = KD.SampleList(dataset_dir, split, self.classes, aug, seed, rank, world)
            self.samples = self.list.samples
            self._queue = None
        else:
            names = KD.read_split(dataset_dir, split)
            if not keep_unlabelled:
                names = [n for n in names if len(KD.read_frame_labels(dataset_dir, n, self.classes)[1]) > 0]
            self.list = None
            self.samples = [(n, ()) for n in names]
            self._queue = [self.samples[i:i + self.batch] for i in range(0, len(self.samples), self.batch)]
        if not self.samples:
            raise ValueError("no frame to load")
        self._rng_host = [int(seed), 0]
        if state is not None:
            if self.list is None:
                raise ValueError("a loader position applies to mode='train' only")
            self.list.load_state_dict(state["samples"])
            self._rng_host = [int(v) for v in state["rng_state"]]
        first = self.samples[0][0]
        fpath = handoff_paths(handoff_dir, first)
        if not os.path.isfile(fpath["features"]):
            raise FileNotFoundError("frame %s: hand-off file %s is missing" % (first, fpath["features"]))
        self.num_points, w = feature_shape(fpath["features"])
        self.channels = w - 5
        self.num_proposals = max(1, len(read_proposals(fpath["proposals"], first)[0]))
        self.rng_state = torch.tensor(self._rng_host, dtype=torch.int64, device=self.device)
        self._feed = KD.ReadAhead(self._prepare, workers)
        self._status = []
        self._feed.submit(self._take())

    def __len__(self):
        return len(self.samples)

    def _take(self):
        if self.list is not None:
            self._pending_pos = self.list.position()
            return self.list.take(self.batch)
        return self._queue.pop(0) if self._queue else None

    def state_dict(self, position=None):
        """train mode: the position of the batch the next next() returns, or of a batch (batch.position), as plain host values"""
        if self.list is None:
            raise ValueError("a loader position applies to mode='train' only")
        lp, rng = (self._pending_pos, self._rng_host) if position is None else position
        return {"samples": self.list.state_dict(lp), "rng_state": [int(v) for v in rng]}

    # --------------------------------------------------------------- host side
    def _read(self, i, name, augs, rows):
        """one sample: the .npy payload into rows (a pinned view), everything else into a dict"""
        paths = handoff_paths(self.handoff_dir, name)
        read_npy_into(paths["features"], rows, (self.num_points, self.channels + 5), name)
        props, _ = read_proposals(paths["proposals"], name)
        if len(props) > self.num_proposals:
            raise ValueError("frame %s: %d proposals, the batch holds %d" % (name, len(props), self.num_proposals))
        calib = kitti_io.read_calib(os.path.join(self.dataset_dir, "calib", name + ".txt"))
        image = KD.read_png(os.path.join(self.dataset_dir, "image_2", name + ".png"))
        h0, w0 = image.shape[:2]
        if os.path.isfile(os.path.join(self.dataset_dir, "label_2", name + ".txt")):
            boxes, cls = KD.read_frame_labels(self.dataset_dir, name, self.classes)
        else:
            boxes, cls = np.zeros((0, 7)), np.zeros((0,), np.int32)
        if len(cls) > self.max_gt:
            raise ValueError("frame %s: %d labels, max_gt is %d" % (name, len(cls), self.max_gt))
        p2 = calib["p2"]
        flip = KD.AUG_FLIPPING in augs
        if flip:
            boxes, props = KD.flip_boxes_3d(boxes), KD.flip_boxes_3d(props)
            p2_aug = KD.flip_p2(p2, (h0, w0))
        else:
            p2_aug = p2
        return {"name": name, "augs": tuple(augs), "image": image, "wh": (w0, h0), "flip": int(flip),
                "jitter": int(KD.AUG_PCA_JITTER in augs), "proposals": np.asarray(props, np.float32).reshape(-1, 7),
                "boxes": np.asarray(boxes, np.float32).reshape(-1, 7), "cls": cls, "p2": np.asarray(p2, np.float32),
                "calib": rescale_p2(p2_aug.astype(np.float32), (w0, h0), (self.img_hw[1], self.img_hw[0]))}

    def _prepare(self, picks, staging, pool):
        b, p, w = len(picks), self.num_points, self.channels + 5
        rows = staging.get("rows", 4 * b * p * w).view(torch.float32).numpy().reshape(b, p, w)
        frames = list(pool.map(lambda a: self._read(a[0], a[1][0], a[1][1], rows[a[0]]), enumerate(picks)))
        return self._pack(frames, staging, rows), [f["name"] for f in frames], [f["augs"] for f in frames], \
            [f["p2"] for f in frames], [f["wh"] for f in frames]

    def _pack(self, frames, staging, rows):
        b, m, g = len(frames), self.num_proposals, self.max_gt
        pix = [f["image"].shape[0] * f["image"].shape[1] for f in frames]
        imgs = staging.get("images", 3 * sum(pix)).numpy()
        parts = [("img_offsets", 8 * b), ("wh", 8 * b), ("flip", 4 * b), ("jitter", 4 * b), ("proposals", 28 * b * m),
                 ("proposal_count", 4 * b), ("gt", 32 * b * g), ("gt_count", 4 * b), ("calib", 48 * b)]
        lay, total = KD._layout(parts)
        meta = staging.get("meta", total)
        mv = meta.numpy()
        view = {k: mv[o:o + n].view(META_DTYPES[k]) for k, (o, n) in lay.items()}
        view["proposals"][:] = 0
        view["gt"][:] = 0
        byte = 0
        for i, f in enumerate(frames):
            im = f["image"].reshape(-1)
            imgs[byte:byte + im.size] = im
            view["img_offsets"][i] = byte
            byte += im.size
            view["wh"][2 * i:2 * i + 2] = f["wh"]
            view["flip"][i] = f["flip"]
            view["jitter"][i] = f["jitter"]
            n = len(f["proposals"])
            view["proposals"][i * m * 7:(i * m + n) * 7] = f["proposals"].reshape(-1)
            view["proposal_count"][i] = n
            ng = len(f["cls"])
            gt = np.concatenate([f["boxes"], np.asarray(f["cls"], np.float32).reshape(-1, 1)], axis=1)
            view["gt"][i * g * 8:(i * g + ng) * 8] = gt.reshape(-1)
            view["gt_count"][i] = ng
            view["calib"][12 * i:12 * i + 12] = f["calib"].reshape(-1)
        return {"layout": lay, "b": b, "max_pixels": max(pix),
                "host": {"rows": staging.get("rows", rows.nbytes), "images": staging.get("images", 3 * sum(pix)), "meta": meta}}

    # --------------------------------------------------------------- device side
    def next(self):
        packed, names, augs, p2, wh = self._feed.take()
        position = (self._pending_pos, tuple(self._rng_host)) if self.list is not None else None
        self._rng_host[1] += self.RNG_CALLS_PER_BATCH
        b, m, g = packed["b"], self.num_proposals, self.max_gt
        with torch.cuda.device(self.device):
            dev, meta = KD.upload_buffers(packed, self.device, META_DTYPES)
            self._feed.uploaded()
            self._feed.submit(self._take())
            rows = dev["rows"].view(torch.float32).view(b, self.num_points, self.channels + 5)
            xyz, inten, fg, fts, status = batch_inputs(rows, meta["flip"])
            image, noise = KD.batch_image(dev["images"], meta["img_offsets"], meta["wh"], meta["flip"], meta["jitter"], self.rng_state,
                                          self.img_hw, packed["max_pixels"])
        self._status.append(status)
        return RcnnBatch(xyz=xyz, intensity=inten, fg_mask=fg, rpn_fts=fts, proposals=meta["proposals"].view(b, m, 7),
                         proposal_count=meta["proposal_count"], gt=meta["gt"].view(b, g, 8), gt_count=meta["gt_count"], image=image,
                         calib=meta["calib"].view(b, 3, 4), status=status, noise=noise, names=names, augs=augs, p2=p2, image_size=wh,
                         position=position)

    def __iter__(self):
        while True:
            try:
                yield self.next()
            except StopIteration:
                return

    def check_status(self):
        """the one synchronising call: {"bad_fg": frames whose fg column held a value other than 0 / 1} since the last check"""
        if not self._status:
            return {"bad_fg": 0}
        st = torch.cat(self._status).cpu().numpy()
        self._status = []
        return {"bad_fg": int(((st & STATUS_BAD_FG) != 0).sum())}

    def close(self):
        self._feed.close()


# ------------------------------------------------------------------------------------------------ second stage on val
@torch.no_grad()
def run_rcnn_from_handoff(trainer_or_model, dataset_dir, handoff_dir, names, out_dir, batch=2, workers=4, score_threshold=0.1):
    """val-mode batches of `names` (every frame, labelled or not) -> RcnnModel.detect -> <out_dir>/<name>.txt KITTI result files
    (original P2 and image size, inference.write_frame_results).  trainer_or_model: an rcnn_train.RcnnTrainer, an
    RcnnWithImageBranch or an RcnnModel (then the image goes in as the feature map).  -> {name: boxes written}"""
    from .inference import write_frame_results
    from .rcnn_train import RcnnTrainer
    model = trainer_or_model.model if isinstance(trainer_or_model, RcnnTrainer) else trainer_or_model
    was_training = model.training
    model.eval()
    os.makedirs(out_dir, exist_ok=True)
    data = KittiRcnnBatches(dataset_dir, handoff_dir, list(names), mode="val", batch=batch, workers=workers,
                            keep_unlabelled=True, device=next(model.parameters()).device)
    written = {}
    try:
        for bt in data:
            dets, _ = model.detect(bt.xyz, bt.rpn_fts, bt.intensity, bt.fg_mask, bt.proposals, bt.image, bt.calib)
            for name, det, p2, wh in zip(bt.names, dets, bt.p2, bt.image_size):
                written[name] = write_frame_results(os.path.join(out_dir, name + ".txt"), det, p2, wh, score_threshold)
    finally:
        data.close()
        model.train(was_training)
    return written
