"""CPU tests of heterofusionrcnn_amd/validate.py: the CSV rows, the skip rule of --checkpoint-dir and the totals arithmetic."""
import os

import numpy as np
import pytest

from heterofusionrcnn_amd import validate as V

RPN_TOT = {"segmentation": 0.123456789, "bin_classification": 1.5, "regression": 2.25, "total": 3.873456789, "seg_accuracy": 0.987654321,
           "recall_50": 2.0 / 3.0, "recall_70": 0.25, "avg_proposals": 100.0, "iou_2d": 0.31415926, "iou_3d": 0.2718281, "angle_residual": 1.0471975}
RCNN_TOT = {"box_classification": 0.693147, "bin_classification": 2.0794415, "regression": 0.5, "total": 3.2725885, "cls_accuracy": 0.8125}


def _read(path):
    with open(path) as f:
        return f.read()


def test_csv_rows_are_the_reference_lines(tmp_path):
    out = str(tmp_path / "pred")
    V.append_csv(out, "rpn", 2000, RPN_TOT)
    assert sorted(os.listdir(out)) == ["rpn_avg_losses.csv", "rpn_avg_seg_acc.csv", "rpn_total_recall.csv"]
    # evaluator.py:696: the last column of the losses file is "%5f" (six decimals), the others "%.5f"
    assert _read(os.path.join(out, "rpn_avg_losses.csv")) == "2000, 0.12346, 1.50000, 2.25000, 3.873457\n"
    assert _read(os.path.join(out, "rpn_avg_seg_acc.csv")) == "2000, 0.98765\n"
    assert _read(os.path.join(out, "rpn_total_recall.csv")) == "2000, 0.66667, 0.25000, 100.00000, 0.31416, 0.27183, 1.04720\n"
    V.append_csv(out, "rcnn", 7, RCNN_TOT)
    assert _read(os.path.join(out, "rcnn_avg_losses.csv")) == "7, 0.69315, 2.07944, 0.50000, 3.27259\n"
    assert _read(os.path.join(out, "rcnn_avg_cls_acc.csv")) == "7, 0.81250\n"
    # np.savetxt with the reference's fmt writes the same line
    import io
    buf = io.BytesIO()
    np.savetxt(buf, np.reshape([2000, RPN_TOT["segmentation"], RPN_TOT["bin_classification"], RPN_TOT["regression"], RPN_TOT["total"]], (1, 5)),
               fmt="%d, %.5f, %.5f, %.5f, %5f")
    assert buf.getvalue().decode() == _read(os.path.join(out, "rpn_avg_losses.csv"))


def test_csv_rows_are_appended(tmp_path):
    out = str(tmp_path)
    V.append_csv(out, "rpn", 1, RPN_TOT)
    V.append_csv(out, "rpn", 2, dict(RPN_TOT, seg_accuracy=0.5))
    assert _read(os.path.join(out, "rpn_avg_seg_acc.csv")) == "1, 0.98765\n2, 0.50000\n"
    assert len(_read(os.path.join(out, "rpn_avg_losses.csv")).splitlines()) == 2
    assert V.evaluated_steps(out, "rpn") == {1, 2} and V.evaluated_steps(out, "rcnn") == set()


def test_a_step_already_in_the_losses_file_is_skipped(tmp_path):
    out = str(tmp_path)
    found = [(3, "c"), (1, "a"), (2, "b"), (10, "d")]
    assert V.pending_checkpoints(found, V.evaluated_steps(out, "rpn")) == [(1, "a"), (2, "b"), (3, "c"), (10, "d")]
    assert V.evaluated_steps(None, "rpn") == set()
    V.append_csv(out, "rpn", 2, RPN_TOT)
    assert V.pending_checkpoints(found, V.evaluated_steps(out, "rpn")) == [(1, "a"), (3, "c"), (10, "d")]
    # the RCNN's files do not count for the RPN and the other way round
    V.append_csv(out, "rcnn", 1, RCNN_TOT)
    assert V.pending_checkpoints(found, V.evaluated_steps(out, "rpn")) == [(1, "a"), (3, "c"), (10, "d")]
    assert V.pending_checkpoints(found, V.evaluated_steps(out, "rcnn")) == [(2, "b"), (3, "c"), (10, "d")]
    # a single row (np.loadtxt gives a 1-D array there, evaluator.py:866-868) and a blank last line
    with open(os.path.join(out, "rpn_avg_losses.csv"), "a") as f:
        f.write("\n")
    assert V.evaluated_steps(out, "rpn") == {2}


def test_rpn_totals_from_per_frame_rows():
    """five frames in batches of 2, 2, 1 (a short last batch); the third frame has no label"""
    rows = {"proposals": np.array([100, 100, 100, 100, 60]), "labels": np.array([3, 1, 0, 4, 2]), "recall_50": np.array([2, 1, 0, 3, 0]),
            "recall_70": np.array([1, 0, 0, 2, 0]), "sum_iou2d": np.array([30.0, 10.0, 0.0, 45.5, 6.0]),
            "sum_iou3d": np.array([20.0, 5.0, 0.0, 40.25, 3.0]), "sum_angle": np.array([50.0, 75.0, 0.0, 25.0, 80.0]),
            "correct": np.array([16000, 16384, 16384, 15000, 8192]), "points": np.full(5, 16384)}
    losses = np.array([[0.5, 1.0, 2.0, 3.5], [0.25, 0.5, 1.0, 1.75], [1.0, 4.0, 8.0, 13.0]], np.float32)
    tot = V.rpn_totals(rows, losses, [2, 2, 1])
    assert tot["frames"] == 5 and tot["labels"] == 10
    assert tot["recall_50"] == 6 / 10 and tot["recall_70"] == 3 / 10
    assert tot["avg_proposals"] == 460 / 5
    assert tot["iou_2d"] == 91.5 / 460 and tot["iou_3d"] == 68.25 / 460 and tot["angle_residual"] == 230.0 / 460
    assert tot["seg_accuracy"] == (16000 + 16384 + 16384 + 15000 + 8192) / (5 * 16384)
    assert tot["segmentation"] == (0.5 * 2 + 0.25 * 2 + 1.0) / 5 and tot["total"] == (3.5 * 2 + 1.75 * 2 + 13.0) / 5
    assert tot["bin_classification"] == (1.0 * 2 + 0.5 * 2 + 4.0) / 5 and tot["regression"] == (2.0 * 2 + 1.0 * 2 + 8.0) / 5
    # at a batch size of 1 the average is the reference's sum / samples
    one = V.frame_weighted_losses(losses, [1, 1, 1], V.RPN_LOSSES)
    assert one["total"] == pytest.approx(float(losses[:, 3].astype(np.float64).sum()) / 3, rel=1e-15)
    # a split without any label: recall 0, no division by zero
    empty = V.rpn_totals({k: (np.zeros(2) if k not in ("proposals", "points") else np.full(2, 100)) for k in rows}, losses[:1], [2])
    assert empty["recall_50"] == 0.0 and empty["recall_70"] == 0.0 and empty["labels"] == 0


def test_rcnn_totals_and_summary_lines():
    tot = V.rcnn_totals({"correct": np.array([90, 80, 100]), "rois": np.array([100, 100, 100])},
                        np.array([[1.0, 2.0, 3.0, 6.0], [0.5, 0.5, 0.5, 1.5]], np.float32), [2, 1])
    assert tot["cls_accuracy"] == 270 / 300 and tot["frames"] == 3
    assert tot["box_classification"] == 2.5 / 3 and tot["total"] == 13.5 / 3
    lines = V.summary_lines("rcnn", 12, tot)
    assert lines[0] == "Step 12: Average RCNN Losses: cls 0.83333, bin_cls 1.50000, reg 2.16667, total 4.50000 "
    assert lines[1] == "Step 12: Average Classification Accuracy: 0.900 "
    lines = V.summary_lines("rpn", 2000, RPN_TOT)
    assert lines == ["Step 2000: Average RPN Losses: segmentation 0.123, bin_cls 1.500, regression 2.250, total 3.873",
                     "Step 2000: Average Segmentation Accuracy:0.988 ",
                     "Step 2000: Total RPN Recall@3DIoU=0.5: 0.667  Recall@3DIoU=0.7: 0.250, Average Proposals: 100.000",
                     "Step 2000: Average RPN IoU_2D: 0.314 , IoU_3D: 0.272, Average Angel Residual: 1.047"]


def test_cli_needs_exactly_one_model_source(capsys):
    for argv in (["rpn", "data"], ["rpn", "data", "m.pt", "--checkpoint-dir", "d"]):
        with pytest.raises(SystemExit):
            V.main(argv)
    assert "MODEL.pt or --checkpoint-dir" in capsys.readouterr().err


def test_the_package_exports_the_two_functions():
    import heterofusionrcnn_amd as hf
    assert hf.validate_rpn is V.validate_rpn and hf.validate_rcnn is V.validate_rcnn
    assert "validate_rpn" in hf.__all__ and "validate_rcnn" in hf.__all__
