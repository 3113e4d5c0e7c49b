"""NumPy restatement of the reference's RPN sample rules (hf/datasets/kitti/kitti_dataset.py:291-440, kitti_aug.py,
obj_utils.py:221-275 and :425-482, box_8c_encoder.np_box_3d_to_box_8co), written the way the reference writes them.
The tests hold heterofusionrcnn_amd.kitti_data and csrc/rpn_batch.hip against these functions."""
import numpy as np


# ------------------------------------------------------------------ points
def view_filter(points, velo_to_rect, p2, wh):
    """raw (N, 4) rows -> (rect (N, 3) fp64, uv (N, 2) fp64 (nan behind the camera), in-view mask, margin): the reference's
    z > 0 and strict 0 < u < w, 0 < v < h; margin = the distance to the nearest of those bounds (px, or m for z)"""
    hom = np.concatenate([points[:, :3].astype(np.float64), np.ones((len(points), 1))], axis=1)
    rect = hom @ np.vstack([velo_to_rect, [0, 0, 0, 1]]).T
    rect = rect[:, :3]
    front = rect[:, 2] > 0
    uvw = np.concatenate([rect, np.ones((len(rect), 1))], axis=1) @ np.asarray(p2, np.float64).T
    with np.errstate(divide="ignore", invalid="ignore"):
        uv = uvw[:, :2] / uvw[:, 2:3]
    w, h = wh
    inside = front & (uv[:, 0] > 0) & (uv[:, 0] < w) & (uv[:, 1] > 0) & (uv[:, 1] < h)
    with np.errstate(invalid="ignore"):
        margin_px = np.min(np.abs(np.stack([uv[:, 0], w - uv[:, 0], uv[:, 1], h - uv[:, 1]], 1)), axis=1)
    return rect, uv, inside, margin_px, np.abs(rect[:, 2])


# ------------------------------------------------------------------ labels
def box_corners(boxes):
    """box_8c_encoder.np_box_3d_to_box_8co: (N, 7) -> (N, 8, 3); float32 corner templates, fp64 rotation"""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    n = len(boxes)
    l, w, h = boxes[:, 3], boxes[:, 4], boxes[:, 5]
    xc = np.array([l / 2.0, l / 2.0, -l / 2.0, -l / 2.0, l / 2.0, l / 2.0, -l / 2.0, -l / 2.0], dtype=np.float32).T
    zc = np.array([w / 2.0, -w / 2.0, -w / 2.0, w / 2.0, w / 2.0, -w / 2.0, -w / 2.0, w / 2.0], dtype=np.float32).T
    yc = np.zeros((n, 8), dtype=np.float32)
    yc[:, 4:8] = -h.reshape(n, 1).repeat(4, axis=1)
    ry = boxes[:, 6]
    zeros, ones = np.zeros(n, np.float32), np.ones(n, np.float32)
    rot = np.transpose(np.array([[np.cos(ry), zeros, -np.sin(ry)], [zeros, ones, zeros], [np.sin(ry), zeros, np.cos(ry)]]), (2, 0, 1))
    temp = np.concatenate((xc.reshape(-1, 8, 1), yc.reshape(-1, 8, 1), zc.reshape(-1, 8, 1)), axis=2)
    r = np.matmul(temp, rot)
    return np.stack([boxes[:, 0:1] + r[:, :, 0], boxes[:, 1:2] + r[:, :, 1], boxes[:, 2:3] + r[:, :, 2]], axis=2)


def is_point_inside(points, corners):
    """obj_utils.is_point_inside: points (3, N), corners (3, 8) -> mask, plus each point's distance (m) to the nearest face"""
    p1, p2, p4, p5 = corners[:, 0], corners[:, 1], corners[:, 3], corners[:, 4]
    u, v, w = p2 - p1, p4 - p1, p5 - p1
    mask = np.ones(points.shape[1], bool)
    dist = np.full(points.shape[1], np.inf)
    for e, a, b in ((u, p1, p2), (v, p1, p4), (w, p1, p5)):
        d = np.dot(e, points)
        lo, hi = np.dot(e, a), np.dot(e, b)
        mask &= (lo < d) & (d < hi)
        n = np.linalg.norm(e)
        dist = np.minimum(dist, np.minimum(np.abs(d - lo), np.abs(d - hi)) / n)
    return mask, dist


def rpn_labels(pts, boxes, classes, expand=0.2):
    """generate_rpn_training_labels -> (cls (N,) int32, reg (N, 7) float32, near_face (N,) distance to the nearest face of any
    box or enlarged box)"""
    n = len(pts)
    cls = np.zeros(n, np.int32)
    reg = np.zeros((n, 7), np.float32)
    boxes = np.asarray(boxes, np.float64).reshape(-1, 7)
    ext = boxes.copy()
    ext[:, 3:6] += expand * 2
    ext[:, 1] += expand
    gc, ec = box_corners(boxes), box_corners(ext)
    near = np.full(n, np.inf)
    for k in range(len(boxes)):
        fg, d1 = is_point_inside(pts.T.astype(np.float64), gc[k].T)
        cls[fg] = classes[k]
        reg[fg, :] = boxes[k]
        en, d2 = is_point_inside(pts.T.astype(np.float64), ec[k].T)
        cls[np.logical_xor(fg, en)] = -1
        near = np.minimum(near, np.minimum(d1, d2))
    return cls, reg, near


# ------------------------------------------------------------------ image
def covariance(img):
    """np.cov of the pixels / 255 in fp64 (ddof 1)"""
    return np.cov((img.reshape(-1, 3) / 255.0).T)


def jitter(img, noise):
    """kitti_aug.add_pca_jitter given the noise vector: trunc(clip(f64(f32(x) / 255) + noise, 0, 1) * 255)"""
    v = img.astype(np.float32) / np.float32(255.0)
    v = v.astype(np.float64) + noise
    np.clip(v, 0.0, 1.0, out=v)
    return (v * 255).astype(np.uint8)


def _axis(d_size, s_size):
    d = np.arange(d_size, dtype=np.float64)
    f = ((d + 0.5) * (s_size / d_size) - 0.5).astype(np.float32)
    s = np.floor(f)
    w = (f - s).astype(np.float32)
    s = s.astype(np.int64)
    lo = s < 0
    w[lo], s[lo] = 0, 0
    hi = s >= s_size - 1
    w[hi], s[hi] = 0, s_size - 1
    return s, np.minimum(s + 1, s_size - 1), w


def resize_linear(img, out_hw):
    """cv2 INTER_LINEAR geometry with fp32 weights, rounded to nearest (the device's rule, not cv2's fixed-point path)"""
    h0, w0 = img.shape[:2]
    x0, x1, wx = _axis(out_hw[1], w0)
    y0, y1, wy = _axis(out_hw[0], h0)
    src = img.astype(np.float32)
    ux, uy = (np.float32(1) - wx)[None, :, None], (np.float32(1) - wy)[:, None, None]
    wx, wy = wx[None, :, None], wy[:, None, None]
    top = src[y0][:, x0] * ux + src[y0][:, x1] * wx
    bot = src[y1][:, x0] * ux + src[y1][:, x1] * wx
    return np.clip(np.rint(top * uy + bot * wy), 0, 255).astype(np.float32)


def image_sample(img, flip, noise, out_hw=(360, 1200)):
    """flip, jitter (noise None: no jitter), resize"""
    x = img[:, ::-1] if flip else img
    if noise is not None:
        x = jitter(x, noise)
    return resize_linear(np.ascontiguousarray(x), out_hw)
