"""heterofusionrcnn_amd.deterministic on any machine: the scope (context manager and decorator, nesting, the cudnn flags set and
restored), refuse_unordered, the keyword on train_loop.run and both trainers, and --deterministic on both command lines."""
import inspect

import pytest
import torch

import heterofusionrcnn_amd as hf
from heterofusionrcnn_amd import determinism as det


def test_scope_nesting_and_the_cudnn_flags():
    before = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = False, True
    try:
        assert not det.is_deterministic()
        det.refuse_unordered("op", "outside the mode nothing happens")
        with hf.deterministic(True):
            assert det.is_deterministic() and torch.backends.cudnn.deterministic and not torch.backends.cudnn.benchmark
            with pytest.raises(RuntimeError, match="some_op.*why"):
                det.refuse_unordered("some_op", "why")
            with hf.deterministic(False):
                assert not det.is_deterministic()
                det.refuse_unordered("op", "switched off for the inner scope")
            assert det.is_deterministic()
        assert not det.is_deterministic() and torch.backends.cudnn.benchmark and not torch.backends.cudnn.deterministic

        @hf.deterministic(True)
        def inside():
            return det.is_deterministic()
        assert inside() and inside() and not det.is_deterministic()
        with pytest.raises(KeyError):
            with hf.deterministic(True):
                raise KeyError("leaves the scope")
        assert not det.is_deterministic() and torch.backends.cudnn.benchmark
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


def test_the_keyword_is_a_trailing_default_everywhere():
    from heterofusionrcnn_amd import train_loop, train_rcnn, train_rpn
    for fn in (train_loop.run, train_rpn.train, train_rcnn.train):
        p = list(inspect.signature(fn).parameters.values())[-1]
        assert p.name == "deterministic" and p.default is False, fn


def test_both_command_lines_accept_the_flag():
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    assert train_rpn.build_parser().parse_args(["d", "--deterministic"]).deterministic is True
    assert train_rpn.build_parser().parse_args(["d"]).deterministic is False
    assert train_rcnn.build_parser().parse_args(["d", "h", "--deterministic"]).deterministic is True
    assert train_rcnn.build_parser().parse_args(["d", "h"]).deterministic is False


def test_runs_that_fuse_the_image_are_refused_before_anything_is_built(capsys):
    """at the command line when the arguments are parsed, and at the top of train(): no loader, no model (the directories do not exist)"""
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    for main, argv in ((train_rpn.main, ["/nowhere", "--deterministic"]), (train_rcnn.main, ["/nowhere", "/nowhere", "--deterministic"])):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and "fuse the image" in capsys.readouterr().err
    with pytest.raises(RuntimeError, match="rpn_multiclass.*fuse the image"):
        train_rpn.train("/nowhere", deterministic=True)
    with pytest.raises(RuntimeError, match="train_rcnn.*fuse the image"):
        train_rcnn.train("/nowhere", "/nowhere", deterministic=True)
    with hf.deterministic(True):
        with pytest.raises(RuntimeError, match="fuse the image"):
            train_rcnn.train("/nowhere", "/nowhere")


def test_host_tensor_forms_are_not_refused():
    """the refusals are about device sums: the host forms of the image ops keep working under the mode"""
    from heterofusionrcnn_amd import fusion
    img = torch.randn(1, 5, 6, 3, requires_grad=True)
    with hf.deterministic(True):
        out = fusion.image_crop_and_resize(img, torch.tensor([[0.1, 0.1, 0.9, 0.9]]), torch.zeros(1, dtype=torch.int32), 3)
        out.sum().backward()
    assert img.grad is not None and float(img.grad.abs().sum()) > 0
