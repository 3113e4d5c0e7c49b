"""NumPy restatement of the RPN -> RCNN hand-off (hf/core/evaluator.py:963-983, hf/datasets/kitti/kitti_dataset.py:238-245,
:473-487) and of the padding rcnn_data.KittiRcnnBatches applies to a batch."""
import numpy as np


def pack(xyz, intensity, fg_mask, rpn_fts):
    """np.hstack((pts, intensity, fg_mask, pc_fts | proj_img_fts)) per frame: (B,P,3), (B,P,1), (B,P) bool, (B,P,c) -> (B,P,5+c)"""
    b, p, _ = xyz.shape
    fg = (np.asarray(fg_mask).reshape(b, p, 1) != 0).astype(np.float32)
    return np.concatenate([xyz.astype(np.float32), intensity.reshape(b, p, 1).astype(np.float32), fg,
                           rpn_fts.astype(np.float32)], axis=-1)


def split(rows, flip):
    """get_rpn_features + kitti_aug.flip_points on flipped frames -> xyz, intensity (B,P,1), fg_mask bool, rpn_fts, status"""
    xyz = rows[..., 0:3].copy()
    for f, fl in enumerate(flip):
        if fl:
            xyz[f, :, 0] = -xyz[f, :, 0]
    m = rows[..., 4]
    status = (~((m == 0) | (m == 1))).any(axis=1).astype(np.int32)
    return xyz, rows[..., 3:4].copy(), m != 0, rows[..., 5:].copy(), status


def pad_proposals(props, m):
    """list of (n_f, 7) -> (B, m, 7) float32 zero-padded, counts (B,)"""
    out = np.zeros((len(props), m, 7), np.float32)
    for f, p in enumerate(props):
        out[f, :len(p)] = p
    return out, np.array([len(p) for p in props], np.int32)


def pad_gt(boxes, classes, g):
    """lists of (n_f, 7) boxes and (n_f,) classes 1..K -> (B, g, 8) [box, class] zero-padded, counts (B,)"""
    out = np.zeros((len(boxes), g, 8), np.float32)
    for f, (bx, c) in enumerate(zip(boxes, classes)):
        out[f, :len(c), :7] = bx
        out[f, :len(c), 7] = c
    return out, np.array([len(c) for c in classes], np.int32)


def flip_boxes(boxes):
    """kitti_aug.flip_boxes_3d"""
    out = np.array(boxes, dtype=np.float64, copy=True).reshape(-1, 7)
    ry = out[:, 6].copy()
    out[:, 6] = np.where(ry >= 0, np.pi - ry, -np.pi - ry)
    out[:, 0] = -out[:, 0]
    return out
