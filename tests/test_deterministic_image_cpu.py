"""The third level of heterofusionrcnn_amd.deterministic on any machine: deterministic("image") keeps its level through nesting and
restore, is_deterministic() stays a bool that is true for both levels, level() and covers_image() tell them apart, record(ctx) keeps
the level; --deterministic-image parses on both command lines and implies the mode; train_rpn.train / train_rcnn.train with
deterministic="image" get past the refusal of the configurations that fuse the image (they fail in the loader instead),
while deterministic=True is refused as before."""
import types

import pytest
import torch

import heterofusionrcnn_amd as hf
from heterofusionrcnn_amd import checkpoint as C
from heterofusionrcnn_amd import determinism as det


def test_levels_nest_and_restore():
    before = (torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark)
    torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = False, True
    try:
        assert det.level() is False and not det.is_deterministic() and not det.covers_image()
        with hf.deterministic("image"):
            assert det.level() == "image" and det.is_deterministic() is True and det.covers_image()
            assert torch.backends.cudnn.deterministic and not torch.backends.cudnn.benchmark
            with pytest.raises(RuntimeError, match="some_op.*why"):
                det.refuse_unordered("some_op", "why")
            with hf.deterministic(True):
                assert det.level() is True and det.is_deterministic() is True and not det.covers_image()
                with hf.deterministic("image"):
                    assert det.level() == "image" and det.covers_image()
                assert det.level() is True
            assert det.level() == "image"
            with hf.deterministic(False):
                assert det.level() is False and det.is_deterministic() is False and not det.covers_image()
            assert det.level() == "image" and det.covers_image()
        assert det.level() is False and torch.backends.cudnn.benchmark and not torch.backends.cudnn.deterministic
        with hf.deterministic(True):
            assert det.level() is True and not det.covers_image()
        with hf.deterministic(1):                          # any other truthy value is the level True, as before
            assert det.level() is True

        @hf.deterministic("image")
        def inside():
            return det.level()
        assert inside() == "image" and inside() == "image" and det.level() is False
        with pytest.raises(KeyError):
            with hf.deterministic("image"):
                raise KeyError("leaves the scope")
        assert det.level() is False
        with pytest.raises(ValueError, match="image"):
            hf.deterministic("images")
    finally:
        torch.backends.cudnn.deterministic, torch.backends.cudnn.benchmark = before


def test_record_keeps_the_level():
    ctx = types.SimpleNamespace()
    with hf.deterministic("image"):
        assert det.record(ctx) == "image"
    assert ctx.hf_deterministic == "image"
    with pytest.raises(RuntimeError, match="op"):
        det.refuse_unordered("op", "recorded under the level", ctx=ctx)
    with hf.deterministic(True):
        assert det.record(ctx) is True
    assert det.record(ctx) is False
    with hf.deterministic("image"):
        det.refuse_unordered("op", "recorded outside", ctx=ctx)


def test_both_command_lines_accept_the_new_flag():
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    for parser, argv in ((train_rpn.build_parser(), ["d"]), (train_rcnn.build_parser(), ["d", "h"])):
        args = parser.parse_args(argv + ["--deterministic-image"])
        assert args.deterministic_image is True and args.deterministic is False and C.deterministic_level(args) == "image"
        args = parser.parse_args(argv + ["--deterministic", "--deterministic-image"])
        assert C.deterministic_level(args) == "image"
        assert C.deterministic_level(parser.parse_args(argv + ["--deterministic"])) is True
        args = parser.parse_args(argv)
        assert args.deterministic_image is False and C.deterministic_level(args) is False


def test_the_image_level_gets_past_the_refusal(capsys):
    """nothing exists at /nowhere: the run fails in the loader (on the missing directory; without a GPU on the missing device before
    it looks), not with the refusal"""
    from heterofusionrcnn_amd import train_rcnn, train_rpn
    for run in (lambda: train_rpn.train("/nowhere", deterministic="image", log=lambda s: None),
                lambda: train_rcnn.train("/nowhere", "/nowhere", deterministic="image", log=lambda s: None),
                lambda: train_rpn.main(["/nowhere", "--deterministic-image"]),
                lambda: train_rcnn.main(["/nowhere", "/nowhere", "--deterministic-image"])):
        with pytest.raises(Exception) as e:
            run()
        assert not isinstance(e.value, SystemExit) and "fuse the image" not in str(e.value), repr(e.value)
        assert "nowhere" in str(e.value) or not torch.cuda.is_available(), repr(e.value)
    with hf.deterministic("image"):
        with pytest.raises(Exception) as e:
            train_rcnn.train("/nowhere", "/nowhere", log=lambda s: None)
        assert "fuse the image" not in str(e.value)
    assert det.level() is False
    # the level True is refused as before, and names the way out
    with pytest.raises(RuntimeError, match="rpn_multiclass.*fuse the image"):
        train_rpn.train("/nowhere", deterministic=True)
    with pytest.raises(RuntimeError, match="train_rcnn.*fuse the image.*deterministic-image"):
        train_rcnn.train("/nowhere", "/nowhere", deterministic=True)
    for main, argv in ((train_rpn.main, ["/nowhere", "--deterministic"]), (train_rcnn.main, ["/nowhere", "/nowhere", "--deterministic"])):
        with pytest.raises(SystemExit) as e:
            main(argv)
        assert e.value.code == 2 and "fuse the image" in capsys.readouterr().err
