"""RPN training batches from KITTI files (hf/datasets/kitti/kitti_dataset.py:113-129 sample list, :291-440 load_rpn_samples,
:781-841 next_batch; hf/datasets/kitti/kitti_aug.py).

  sample list     every frame of the split x every combination of the augmentation list (none, each alone, both), frames
                  without a label of the configured classes dropped up front (the reference skips them in next_batch and
                  refills the batch); shuffled by a seeded host RNG at the start of each epoch, rank-strided shards of the
                  same permutation (dp.shard_frames)
  host work       a pool of `workers` threads reads scans, calibration, labels and PNGs (PIL), flips the boxes and P2
                  (kitti_aug.flip_boxes_3d, flip_stereo_calib_p2) and rescales P2 (inference.rescale_p2); everything is
                  packed into pinned staging buffers, one batch ahead of use
  device work     one copy per buffer, then csrc/rpn_batch.hip: hf_rpn_batch_points (view filter, 16384-point sampling,
                  flip), hf_rpn_point_labels (last box wins, the ring of the enlarged box = -1), hf_rpn_batch_image (flip,
                  PCA jitter, 360 x 1200 bilinear resize)

Random numbers on the device come from a [seed, call] pair that each call advances; they do not follow NumPy's stream.
Nothing here synchronises with the device except check_status().
"""
import concurrent.futures
import copy
import itertools
import os

import numpy as np
import torch

from . import _lib, dp, kitti_io
from ._lib import check, ptr, stream_ptr
from .inference import CLASSES, rescale_p2

AUG_FLIPPING, AUG_PCA_JITTER = "flipping", "pca_jitter"
EXPAND_GT_SIZE = 0.2                         # rpn_multiclass.config:265
STATUS_EMPTY, STATUS_TOO_MANY_FAR = 1, 2     # include/hfops.h HF_RPN_BATCH_*


# ------------------------------------------------------------------------------------------------ host rules
def read_split(dataset_dir, split):
    """frame names: a list as given, or the lines of a list file (a path, or <dataset_dir>/../<split>.txt / <dataset_dir>/<split>.txt)"""
    if not isinstance(split, str):
        return [str(s) for s in split]
    candidates = [split, os.path.join(dataset_dir, split + ".txt"), os.path.join(os.path.dirname(os.path.abspath(dataset_dir)), split + ".txt")]
    for path in candidates:
        if os.path.isfile(path):
            with open(path) as f:
                return [line.strip() for line in f if line.strip()]
    raise FileNotFoundError("split %r: none of %s exists" % (split, candidates))


def aug_combinations(aug_list):
    """(), then each augmentation alone, then pairs, ... (itertools.combinations by length, kitti_dataset.py:118-126)"""
    return [c for k in range(len(aug_list) + 1) for c in itertools.combinations(tuple(aug_list), k)]


def build_sample_list(names, aug_list):
    """[(name, augs)]: the combinations in the outer loop, frames in the inner one, as the reference orders them"""
    return [(n, augs) for augs in aug_combinations(aug_list) for n in names]


def flip_boxes_3d(boxes):
    """kitti_aug.flip_boxes_3d: ry -> pi - ry (ry >= 0) or -pi - ry, x -> -x"""
    out = np.array(boxes, dtype=np.float64, copy=True).reshape(-1, 7)
    ry = out[:, 6].copy()
    out[:, 6] = np.where(ry >= 0, np.pi - ry, -np.pi - ry)
    out[:, 0] = -out[:, 0]
    return out


def flip_p2(p2, image_hw):
    """kitti_aug.flip_stereo_calib_p2: p2[0, 2] -> w - p2[0, 2], p2[0, 3] -> -p2[0, 3]"""
    out = np.array(p2, copy=True)
    out[0, 2] = image_hw[1] - p2[0, 2]
    out[0, 3] = -p2[0, 3]
    return out


def velo_to_rect_matrix(calib):
    """rows 0..2 of R0_rect (padded) . Tr_velo_to_cam (padded), fp64, composed as kitti_io.lidar_to_rect composes it"""
    r0 = np.eye(4)
    r0[:3, :3] = calib["r0_rect"]
    tr = np.eye(4)
    tr[:3, :4] = calib["tr_velo_to_cam"]
    return (r0 @ tr)[:3]


def read_frame_labels(dataset_dir, name, classes):
    """(boxes (G, 7) fp64, classes (G,) int32 1..K) of the configured classes"""
    types, boxes, _, _ = kitti_io.read_labels(os.path.join(dataset_dir, "label_2", name + ".txt"), classes)
    return boxes, np.array([classes.index(t) + 1 for t in types], dtype=np.int32)


def read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


def read_frame(dataset_dir, name, augs, classes, img_hw):
    """every host-side input of one sample"""
    calib = kitti_io.read_calib(os.path.join(dataset_dir, "calib", name + ".txt"))
    image = read_png(os.path.join(dataset_dir, "image_2", name + ".png"))
    h0, w0 = image.shape[:2]
    boxes, cls = read_frame_labels(dataset_dir, name, classes)
    p2 = calib["p2"]
    flip = AUG_FLIPPING in augs
    if flip:
        boxes = flip_boxes_3d(boxes)
        p2_aug = flip_p2(p2, (h0, w0))
    else:
        p2_aug = p2
    return {"name": name, "augs": tuple(augs), "points": kitti_io.read_velodyne(os.path.join(dataset_dir, "velodyne", name + ".bin")),
            "velo_to_rect": velo_to_rect_matrix(calib), "p2": np.asarray(p2, np.float64), "wh": (w0, h0), "image": image,
            "flip": int(flip), "jitter": int(AUG_PCA_JITTER in augs), "boxes": boxes, "cls": cls,
            "calib": rescale_p2(p2_aug.astype(np.float32), (w0, h0), (img_hw[1], img_hw[0]))}


# ------------------------------------------------------------------------------------------------ device calls
def _ws(nbytes, device):
    return torch.empty((max(int(nbytes), 1),), dtype=torch.uint8, device=device)


def batch_points(points, offsets, velo_to_rect, p2, image_wh, flip, rng_state, num_points, max_frame_points):
    """hf_rpn_batch_points on device tensors -> xyz (B,P,3), intensity (B,P,1), src_index (B,P), status (B,)"""
    L = _lib.lib()
    b = offsets.numel() - 1
    dev = offsets.device
    xyz = torch.empty((b, num_points, 3), dtype=torch.float32, device=dev)
    inten = torch.empty((b, num_points, 1), dtype=torch.float32, device=dev)
    src = torch.empty((b, num_points), dtype=torch.int32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    total = points.shape[0]
    nbytes = L.hf_rpn_batch_points_workspace(b, total, max_frame_points)
    ws = _ws(nbytes, dev)
    check(L.hf_rpn_batch_points(b, num_points, total, max_frame_points, ptr(points), ptr(offsets), ptr(velo_to_rect), ptr(p2),
                                ptr(image_wh), ptr(flip), ptr(rng_state), ptr(xyz), ptr(inten), ptr(src), ptr(status), ptr(ws),
                                nbytes, stream_ptr()), "rpn_batch_points")
    return xyz, inten, src, status


def point_labels(xyz, boxes, classes, gt_count, expand=EXPAND_GT_SIZE):
    """hf_rpn_point_labels -> label_cls (B,P) int32 in {-1, 0..K}, label_reg (B,P,7)"""
    b, p, _ = xyz.shape
    g = boxes.shape[1]
    label_cls = torch.empty((b, p), dtype=torch.int32, device=xyz.device)
    label_reg = torch.empty((b, p, 7), dtype=torch.float32, device=xyz.device)
    check(_lib.lib().hf_rpn_point_labels(b, p, g, ptr(xyz), ptr(boxes), ptr(classes), ptr(gt_count), float(expand), ptr(label_cls),
                                         ptr(label_reg), stream_ptr()), "rpn_point_labels")
    return label_cls, label_reg


def batch_image(images, offsets, image_wh, flip, jitter, rng_state, img_hw, max_pixels, stats=False):
    """hf_rpn_batch_image -> image (B,H,W,3) float32 0..255, noise (B,3) fp64[, pca stats (B,21) fp64]"""
    L = _lib.lib()
    b = offsets.numel()
    dev = offsets.device
    image = torch.empty((b, img_hw[0], img_hw[1], 3), dtype=torch.float32, device=dev)
    noise = torch.empty((b, 3), dtype=torch.float64, device=dev)
    st = torch.empty((b, 21), dtype=torch.float64, device=dev) if stats else None
    nbytes = L.hf_rpn_batch_image_workspace(b, max_pixels)
    ws = _ws(nbytes, dev)
    check(L.hf_rpn_batch_image(b, max_pixels, images.numel(), ptr(images), ptr(offsets), ptr(image_wh), ptr(flip), ptr(jitter),
                               img_hw[0], img_hw[1], ptr(rng_state), ptr(image), ptr(noise), ptr(st), ptr(ws), nbytes, stream_ptr()),
          "rpn_batch_image")
    return (image, noise, st) if stats else (image, noise)


# ------------------------------------------------------------------------------------------------ packing
class _Staging:
    """pinned host buffers of one batch (grown on demand) and the event that says their last copy has finished"""

    def __init__(self):
        self.bufs = {}
        self.event = None

    def get(self, key, nbytes):
        buf = self.bufs.get(key)
        if buf is None or buf.numel() < nbytes:
            buf = torch.empty((max(nbytes, 1) * 5 // 4,), dtype=torch.uint8).pin_memory()
            self.bufs[key] = buf
        return buf[:nbytes]


class ReadAhead:
    """Host work one batch ahead of the device: the reader pool (`workers` threads), the single ahead thread and the two
    _Staging sets used in turn.  submit(picks) runs prepare(picks, staging, pool) on the ahead thread once the copy that last
    read that staging's pinned buffers has finished (picks None: nothing is pending); take() returns what prepare returned and
    raises what it raised (nothing pending: StopIteration); uploaded(), called after the caller has enqueued its host-to-device
    copies, records the staging's event on the current stream and passes the turn to the other staging.
    event: the event class (record(), synchronize()), a seam for tests without a device."""

    def __init__(self, prepare, workers, event=torch.cuda.Event):
        self._prepare, self._event = prepare, event
        self._pool = concurrent.futures.ThreadPoolExecutor(max_workers=max(1, int(workers)), thread_name_prefix="hf-read-pool")
        self._ahead = concurrent.futures.ThreadPoolExecutor(max_workers=1, thread_name_prefix="hf-read-ahead")
        self._staging, self._turn, self._pending = [_Staging(), _Staging()], 0, None

    def _run(self, picks, staging):
        if staging.event is not None:
            staging.event.synchronize()        # the copy that last read these pinned buffers has finished
        return self._prepare(picks, staging, self._pool)

    def submit(self, picks):
        self._pending = None if picks is None else self._ahead.submit(self._run, picks, self._staging[self._turn])

    def take(self):
        if self._pending is None:
            raise StopIteration
        return self._pending.result()

    def uploaded(self):
        staging = self._staging[self._turn]
        staging.event = self._event()
        staging.event.record()
        self._turn ^= 1

    def close(self):
        self._ahead.shutdown(wait=True)
        self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _layout(parts):
    """[(name, nbytes)] -> ({name: (offset, nbytes)}, total) with every segment 16-byte aligned"""
    out, off = {}, 0
    for name, n in parts:
        out[name] = (off, n)
        off += (n + 15) & ~15
    return out, off


def _torch_dtype(np_dtype):
    return torch.from_numpy(np.empty(0, np_dtype)).dtype


# the fields of the RPN batch's meta buffer; rcnn_data has its own table, and both cut the host and the device bytes by one
META_DTYPES = {"offsets": np.int64, "velo_to_rect": np.float64, "p2": np.float64, "img_offsets": np.int64, "wh": np.int32,
               "flip": np.int32, "jitter": np.int32, "boxes": np.float32, "cls": np.int32, "gt_count": np.int32, "calib": np.float32}


def pack_frames(frames, staging):
    """frames (read_frame dicts) -> host views of the staging buffers + the shapes the device calls need"""
    b = len(frames)
    counts = [len(f["points"]) for f in frames]
    pix = [f["image"].shape[0] * f["image"].shape[1] for f in frames]
    g = max(1, max(len(f["cls"]) for f in frames))
    pts = staging.get("points", 16 * sum(counts)).view(torch.float32).numpy().reshape(-1, 4)
    imgs = staging.get("images", 3 * sum(pix)).numpy()
    meta_parts = [("offsets", 8 * (b + 1)), ("velo_to_rect", 96 * b), ("p2", 96 * b), ("img_offsets", 8 * b), ("wh", 8 * b),
                  ("flip", 4 * b), ("jitter", 4 * b), ("boxes", 28 * b * g), ("cls", 4 * b * g), ("gt_count", 4 * b), ("calib", 48 * b)]
    lay, total = _layout(meta_parts)
    meta = staging.get("meta", total)
    mv = meta.numpy()
    view = {k: mv[o:o + n].view(META_DTYPES[k]) for k, (o, n) in lay.items()}
    view["boxes"][:] = 0
    view["cls"][:] = 0
    row, byte = 0, 0
    for i, f in enumerate(frames):
        n = counts[i]
        pts[row:row + n] = f["points"]
        view["offsets"][i] = row
        row += n
        im = f["image"].reshape(-1)
        imgs[byte:byte + im.size] = im
        view["img_offsets"][i] = byte
        byte += im.size
        view["velo_to_rect"][12 * i:12 * i + 12] = f["velo_to_rect"].reshape(-1)
        view["p2"][12 * i:12 * i + 12] = f["p2"].reshape(-1)
        view["wh"][2 * i:2 * i + 2] = f["wh"]
        view["flip"][i] = f["flip"]
        view["jitter"][i] = f["jitter"]
        ng = len(f["cls"])
        view["boxes"][i * g * 7:(i * g + ng) * 7] = f["boxes"].astype(np.float32).reshape(-1)
        view["cls"][i * g:i * g + ng] = f["cls"]
        view["gt_count"][i] = ng
        view["calib"][12 * i:12 * i + 12] = f["calib"].reshape(-1)
    view["offsets"][b] = row
    return {"layout": lay, "g": g, "b": b, "max_frame_points": max(counts), "max_pixels": max(pix),
            "host": {"points": staging.get("points", 16 * sum(counts)), "images": staging.get("images", 3 * sum(pix)), "meta": meta}}


def upload_buffers(packed, device, dtypes):
    """one non-blocking copy per pinned buffer -> ({buffer: device bytes}, meta cut into typed views by `dtypes`, a META_DTYPES)"""
    dev = {k: torch.empty(v.shape, dtype=torch.uint8, device=device) for k, v in packed["host"].items()}
    for k, v in packed["host"].items():
        dev[k].copy_(v, non_blocking=True)
    return dev, {k: dev["meta"][o:o + n].view(_torch_dtype(dtypes[k])) for k, (o, n) in packed["layout"].items()}


def upload(packed, device):
    """upload_buffers of an RPN batch (pack_frames) -> points (N, 4), image bytes, meta with boxes, cls and calib in shape"""
    dev, meta = upload_buffers(packed, device, META_DTYPES)
    b, g = packed["b"], packed["g"]
    meta["boxes"] = meta["boxes"].view(b, g, 7)
    meta["cls"] = meta["cls"].view(b, g)
    meta["calib"] = meta["calib"].view(b, 3, 4)
    return dev["points"].view(torch.float32).view(-1, 4), dev["images"], meta


# ------------------------------------------------------------------------------------------------ the loader
class SampleList:
    """the sample list of a split and its per-epoch order (host only): every labelled frame x every augmentation combination,
    reshuffled by the seeded host RNG at the start of each epoch, this rank's rank-strided shard of the permutation"""

    def __init__(self, dataset_dir, split, classes=CLASSES, aug_list=(AUG_FLIPPING, AUG_PCA_JITTER), seed=0, rank=0, world=1):
        names = read_split(dataset_dir, split)
        labelled = [n for n in names if len(read_frame_labels(dataset_dir, n, list(classes))[1]) > 0]
        self.dropped = [n for n in names if n not in set(labelled)]
        self.samples = build_sample_list(labelled, aug_list)
        if not self.samples:
            raise ValueError("no frame of the split has a label of %s" % (list(classes),))
        self.rank, self.world = rank, world
        self.rng = np.random.default_rng(seed)
        self.epoch, self.order, self._pos = 0, [], 0
        self.next_epoch()

    def __len__(self):
        return len(self.samples)

    def next_epoch(self):
        perm = self.rng.permutation(len(self.samples))
        self.order = [int(perm[i]) for i in dp.shard_frames(len(perm), self.rank, self.world)]
        self._pos = 0
        self.epoch += 1
        self._rng_after = self.rng.bit_generator.state      # the generator moves only here: position() needs no copy per take

    def position(self):
        """where take() stands: (host generator state, epoch, order, pos); order is never changed in place, so this is cheap"""
        return (self._rng_after, self.epoch, self.order, self._pos)

    def state_dict(self, position=None):
        """a position() (default: the current one) as plain Python values"""
        rng, epoch, order, pos = self.position() if position is None else position
        return {"rng": copy.deepcopy(rng), "epoch": int(epoch), "order": [int(i) for i in order], "pos": int(pos),
                "num_samples": len(self.samples)}

    def load_state_dict(self, state):
        """continue from a state_dict(): the next take() returns what it returned after that state was recorded"""
        if int(state["num_samples"]) != len(self.samples):
            raise ValueError("sample list position: %d samples saved, this split has %d" % (int(state["num_samples"]), len(self.samples)))
        self.rng.bit_generator.state = copy.deepcopy(state["rng"])
        self._rng_after = self.rng.bit_generator.state
        self.epoch, self.order, self._pos = int(state["epoch"]), [int(i) for i in state["order"]], int(state["pos"])

    def take(self, n):
        """the next n samples of this rank, crossing into the next epoch when this one runs out"""
        out = []
        while len(out) < n:
            if self._pos >= len(self.order):
                self.next_epoch()
            out.append(self.samples[self.order[self._pos]])
            self._pos += 1
        return out


class RpnBatch(dict):
    """device tensors of one batch (xyz, intensity, label_cls, label_reg, image, calib, gt_boxes, gt_cls, gt_count, status,
    src_index, noise) plus the host lists names / augs and `position` (where the loader stood before drawing this batch: its
    state_dict(position) is what a checkpoint taken before training on the batch records); attribute access reads the dict"""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def train_inputs(self):
        """the dict graph_step.TrainStep takes (the image in the img_fts slot, which RpnWithImageBranch reads)"""
        return {"xyz": self["xyz"], "intensity": self["intensity"], "label_cls": self["label_cls"], "label_reg": self["label_reg"],
                "calib": self["calib"], "img_fts": self["image"]}


class KittiRpnBatches:
    """RPN training batches of `batch` samples from <dataset_dir>/{velodyne,calib,label_2,image_2}.

      data = KittiRpnBatches(root, "train", CLASSES, batch=8, seed=0)
      b = data.next()                   # device tensors, enqueued on the current stream
      step = TrainStep(model, opt, b.train_inputs(), model.geometry(b.xyz))
      ...; step.load(**data.next().train_inputs())

    Host reading runs one batch ahead on `workers` threads; next() issues the copies and the three device calls.

    Resuming: state_dict() is the position of the next batch next() returns (host generator, epoch, order, position in it, and
    the device [seed, call] pair that batch starts from), state_dict(batch.position) that of a batch already drawn (the loader
    works one batch ahead, the trainers hold one more), and KittiRpnBatches(..., state=that) draws the same frames, flips,
    sampled points and jitter from there on."""

    RNG_CALLS_PER_BATCH = 2      # hf_rpn_batch_points, hf_rpn_batch_image: each advances rng_state[1] by one (rpn_batch.hip)

    def __init__(self, dataset_dir, split, classes=CLASSES, batch=8, num_points=16384, img_hw=(360, 1200),
                 aug_list=(AUG_FLIPPING, AUG_PCA_JITTER), seed=0, rank=0, world=1, workers=8, device=None, state=None):
        self.dataset_dir, self.classes = dataset_dir, list(classes)
        self.batch, self.num_points, self.img_hw = int(batch), int(num_points), tuple(img_hw)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.list = SampleList(dataset_dir, split, self.classes, aug_list, seed, rank, world)
        self.samples = self.list.samples
        # the device [seed, call] pair, mirrored on the host (the kernels advance the call number by one per call)
        self._rng_host = [int(seed), 0]
        if state is not None:
            self.list.load_state_dict(state["samples"])
            self._rng_host = [int(v) for v in state["rng_state"]]
        self.rng_state = torch.tensor(self._rng_host, dtype=torch.int64, device=self.device)
        self._feed = ReadAhead(self._prepare, workers)
        self._status = []
        self._pending_pos = self.list.position()
        self._feed.submit(self.list.take(self.batch))

    def state_dict(self, position=None):
        """the position of the batch the next next() returns, or of a batch (batch.position), as plain host values (no
        synchronisation)"""
        lp, rng = (self._pending_pos, self._rng_host) if position is None else position
        return {"samples": self.list.state_dict(lp), "rng_state": [int(v) for v in rng]}

    def __len__(self):
        return len(self.samples)

    def _prepare(self, picks, staging, pool):
        frames = list(pool.map(lambda s: read_frame(self.dataset_dir, s[0], s[1], self.classes, self.img_hw), picks))
        return pack_frames(frames, staging), [f["name"] for f in frames], [f["augs"] for f in frames]

    # --------------------------------------------------------------- device side
    def next(self):
        packed, names, augs = self._feed.take()
        position = (self._pending_pos, tuple(self._rng_host))     # raw: state_dict(position) makes it plain values
        self._rng_host[1] += self.RNG_CALLS_PER_BATCH
        with torch.cuda.device(self.device):
            points, images, meta = upload(packed, self.device)
            self._feed.uploaded()
            self._pending_pos = self.list.position()
            self._feed.submit(self.list.take(self.batch))
            xyz, inten, src, status = batch_points(points, meta["offsets"], meta["velo_to_rect"], meta["p2"], meta["wh"], meta["flip"],
                                                   self.rng_state, self.num_points, packed["max_frame_points"])
            label_cls, label_reg = point_labels(xyz, meta["boxes"], meta["cls"], meta["gt_count"])
            image, noise = batch_image(images, meta["img_offsets"], meta["wh"], meta["flip"], meta["jitter"], self.rng_state,
                                       self.img_hw, packed["max_pixels"])
        self._status.append(status)
        return RpnBatch(xyz=xyz, intensity=inten, label_cls=label_cls, label_reg=label_reg, image=image, calib=meta["calib"],
                        gt_boxes=meta["boxes"], gt_cls=meta["cls"], gt_count=meta["gt_count"], status=status, src_index=src,
                        noise=noise, names=names, augs=augs, position=position)

    def check_status(self):
        """the one synchronising call: status bits of every batch since the last check -> {"empty": frames with no point in
        view (zeros were written), "too_many_far": frames that kept a random P of more than P far points}"""
        if not self._status:
            return {"empty": 0, "too_many_far": 0}
        st = torch.cat(self._status).cpu().numpy()
        self._status = []
        return {"empty": int(((st & STATUS_EMPTY) != 0).sum()), "too_many_far": int(((st & STATUS_TOO_MANY_FAR) != 0).sum())}

    def close(self):
        self._feed.close()
