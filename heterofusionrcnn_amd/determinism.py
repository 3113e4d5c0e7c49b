"""Bit-reproducible training as an opt-in mode with three levels, in the style of mlp.training_precision:

    with heterofusionrcnn_amd.deterministic(True): ...          # or @heterofusionrcnn_amd.deterministic(True) on a function
    with heterofusionrcnn_amd.deterministic("image"): ...       # the same, and the image-feature gradients in ordered form

False is off.  Inside a scope of level True or "image"
  * the routes of the training path whose floating-point sum has no fixed order raise a RuntimeError that names the op instead of
    running: a gradient without its inverse index (group_point / concat_group / the fused gather layers beyond INVERSE_MAX_TARGETS,
    three_interpolate beyond INVERSE_MAX_KNOWN), xconv_depthwise_gather(use_workspace=False), the tensor forms of the image ops on
    device tensors with a gradient (their index gradient adds atomically), and the two raw gradient ops pc_crop_and_sample_grad_fts
    and three_interpolate_channel_first_grad;
  * the fused dense X-Conv gradient takes its fixed-order workspace form (hf_xconv_depthwise_grad_ws);
  * torch.backends.cudnn.deterministic is True and .benchmark False (stock convolutions), restored on exit.
The two levels differ in the image-feature gradients of project_gather and image_crop_and_resize, which by default are summed by
fp32 atomics.  Level True refuses them like every other unordered route, so only the point-cloud configurations train under it.
Level "image" takes their ordered form (hf_project_gather_grad_ordered / hf_crop_and_resize_grad_ordered, csrc/ordered_scatter.h:
every pixel's terms added in ascending entry order), so every configuration trains under it; it costs what DESIGN.md section 8,
"Reproducible training", reports.  Either op also takes ordered_grad=True / False to choose its backward whatever the level (the
atomic one is refused under both levels).
One rule for every op: the mode is read when the op's FORWARD is recorded, where a gradient is actually wanted (an op whose inputs
need no gradient never refuses), and the backward acts on what the forward recorded, inside the scope or not (record(ctx) /
refuse_unordered(..., ctx=ctx)).  The raw gradient ops have no forward: they read the mode when called.  Ops outside the training
path that add with atomics and are not listed above (the raw C ABI, hf_group_concat_grad of the PointNet++ modules) are outside
the mode.  The default routes are untouched outside the scope.  The mode sets no environment variable and changes nothing about
how a captured graph is replayed."""
import contextlib

import torch

LEVELS = (False, True, "image")
_DETERMINISTIC = [False]          # the level: one of LEVELS


def as_level(enabled):
    """False / True / "image" from what a caller passes (any other truthy value is True, as before the third level)"""
    if isinstance(enabled, str):
        if enabled != "image":
            raise ValueError("deterministic: the levels are False, True and \"image\", not %r" % (enabled,))
        return "image"
    return bool(enabled)


def level():
    '''the level in force: False, True or "image"'''
    return _DETERMINISTIC[0]


def is_deterministic():
    """True under either level"""
    return bool(_DETERMINISTIC[0])


def covers_image():
    """True under the level whose image-feature gradients take their ordered form"""
    return _DETERMINISTIC[0] == "image"


class deterministic(contextlib.ContextDecorator):
    """the scope of the mode at a level; deterministic(False) inside it switches the mode off for its own scope"""

    def __init__(self, enabled=True):
        self.enabled = as_level(enabled)
        self._saved = []

    def __enter__(self):
        self._saved.append((_DETERMINISTIC[0], torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark))
        _DETERMINISTIC[0] = self.enabled
        if self.enabled:
            torch.backends.cudnn.deterministic = True
            torch.backends.cudnn.benchmark = False
        return self

    def __exit__(self, *exc):
        _DETERMINISTIC[0], torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = self._saved.pop()
        return False


def record(ctx):
    """in an autograd Function's forward: keep the level for its backward"""
    ctx.hf_deterministic = _DETERMINISTIC[0]
    return ctx.hf_deterministic


def refuse_unordered(op, why, ctx=None):
    """called where a route would sum in an order that is not fixed: under the mode (ctx given: the mode its forward recorded) it
    raises, outside it does nothing"""
    if ctx.hf_deterministic if ctx is not None else _DETERMINISTIC[0]:
        raise RuntimeError("%s: deterministic mode refuses this route (%s): its floating-point sum has no fixed order" % (op, why))


IMAGE_CONFIGS_REFUSED = ("deterministic training does not cover the configurations that fuse the image: the gradient of the image feature "
                         "map (project_gather, image_crop_and_resize) is summed by fp32 atomics; train rpn_multiclass_points under it, "
                         "or ask for the level that orders those sums (deterministic=\"image\", --deterministic-image)")


def refuse_image_config(what):
    """train_rpn / train_rcnn: a run that fuses the image is refused before anything is built"""
    raise RuntimeError("%s: %s" % (what, IMAGE_CONFIGS_REFUSED))
