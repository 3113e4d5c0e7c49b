"""CPU tests (-m "not gpu") of the reference's train op and the resumable checkpoints: the argument checks of the two new entry
points (hf_adam_sqnorm_partials, hf_adam_multi_sched) before any launch, the host restatement of the learning-rate schedule,
the checkpoint files (names, rotation, the newest, no partial file), the sample list's position and the trainers' flags."""
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD_KITTI = os.path.join(ROOT, "tests", "golden", "kitti")


# ------------------------------------------------------------------------------------------------ entry points
def test_new_entry_points_refuse_bad_arguments_before_any_launch():
    from heterofusionrcnn_amd import _lib
    L = _lib.lib()
    fake = 16                       # a non-null address that is never dereferenced: every call below fails its checks first
    E = _lib.HF_EINVAL
    # partials: null table / map / partials, negative count
    assert L.hf_adam_sqnorm_partials(1, None, fake, 1.0, fake, None) == E
    assert L.hf_adam_sqnorm_partials(1, fake, None, 1.0, fake, None) == E
    assert L.hf_adam_sqnorm_partials(1, fake, fake, 1.0, None, None) == E
    assert L.hf_adam_sqnorm_partials(-1, fake, fake, 1.0, fake, None) == E
    assert L.hf_adam_sqnorm_partials(0, None, None, 1.0, None, None) == _lib.HF_OK       # nothing to do, nothing launched

    def sched(n=1, table=fake, cmap=fake, step=fake, partials=fake, clip=1.0, lr=1e-3, decay=2, steps=20000.0, factor=0.8, b1=0.9,
              b2=0.999, eps=1e-8, scale=1.0, mode=0):
        return L.hf_adam_multi_sched(n, table, cmap, step, partials, clip, lr, decay, steps, factor, b1, b2, eps, scale, mode, None)

    assert sched(table=None) == E
    assert sched(cmap=None) == E
    assert sched(step=None) == E
    assert sched(partials=None) == E                       # clipping reads the partials
    assert sched(n=-1) == E
    assert sched(clip=-1.0) == E
    assert sched(clip=float("nan")) == E
    assert sched(steps=0.0) == E and sched(steps=-3.0) == E
    assert sched(factor=0.0) == E and sched(factor=-0.5) == E
    assert sched(decay=3) == E and sched(decay=-1) == E
    assert sched(mode=2) == E and sched(b1=1.0) == E and sched(b2=-0.1) == E
    assert sched(n=0, table=None, cmap=None, step=None, partials=None) == _lib.HF_OK
    # decay off: decay_steps / decay_factor are not read; clipping off: partials are not read -- still no launch with n = -1
    assert sched(n=-1, decay=0, steps=0.0, factor=0.0, clip=0.0, partials=None) == E


# ------------------------------------------------------------------------------------------------ schedule
def test_lr_at_is_tensorflow_exponential_decay():
    from heterofusionrcnn_amd.optim import lr_at
    f32 = lambda x: float(np.float32(x))
    ref = (20000, 0.8)                                      # rpn_multiclass.config / rcnn_multiclass.config
    assert lr_at(1e-3, None, 123456) == f32(1e-3)
    assert lr_at(1e-3, ref, 0) == f32(1e-3)
    assert lr_at(1e-3, ref, 19999) == f32(1e-3)             # staircase by default
    assert lr_at(1e-3, ref, 20000) == pytest.approx(8e-4, rel=1e-6)
    assert lr_at(1e-3, ref, 20001) == pytest.approx(8e-4, rel=1e-6)
    assert lr_at(1e-3, ref, 39999) == pytest.approx(8e-4, rel=1e-6)
    assert lr_at(1e-3, ref, 40000) == pytest.approx(6.4e-4, rel=1e-6)
    assert lr_at(1e-3, ref, 239999) == pytest.approx(1e-3 * 0.8 ** 11, rel=1e-6)
    smooth = (20000, 0.8, False)
    assert lr_at(1e-3, smooth, 0) == f32(1e-3)
    assert lr_at(1e-3, smooth, 10000) == pytest.approx(1e-3 * 0.8 ** 0.5, rel=1e-6)
    assert lr_at(1e-3, smooth, 19999) == pytest.approx(1e-3 * 0.8 ** (19999 / 20000), rel=1e-6)
    assert lr_at(1e-3, smooth, 20000) == pytest.approx(8e-4, rel=1e-6)
    assert lr_at(1e-3, smooth, 20001) == pytest.approx(1e-3 * 0.8 ** (20001 / 20000), rel=1e-6)
    assert lr_at(0.5, (3, 0.5), 2) == 0.5 and lr_at(0.5, (3, 0.5), 3) == 0.25 and lr_at(0.5, (3, 0.5), 9) == 0.0625
    with pytest.raises(ValueError):
        lr_at(1e-3, (0, 0.8), 1)
    with pytest.raises(ValueError):
        lr_at(1e-3, (100, 0.0), 1)


def test_optimizer_refuses_negative_clip_norm_without_a_gpu():
    from heterofusionrcnn_amd.optim import MultiTensorAdam
    with pytest.raises(ValueError, match="clip_norm"):
        MultiTensorAdam([torch.zeros(3, requires_grad=True)], clip_norm=-1.0)


# ------------------------------------------------------------------------------------------------ checkpoint files
def _payload(v):
    return {"model": {"w": torch.full((4,), float(v))}, "optimizer": {"step_count": torch.tensor(float(v))}}


def test_checkpoint_names_rotation_and_latest(tmp_path):
    from heterofusionrcnn_amd import checkpoint as C
    d = str(tmp_path / "ck")
    assert C.latest_checkpoint(d) is None and C.list_checkpoints(d) == []
    assert os.path.basename(C.checkpoint_path(d, 2000)) == "ckpt-00002000.pt"
    for s in (2, 4, 6, 8):
        p = C.save_checkpoint(d, s, _payload(s), keep=2)
        assert p == C.checkpoint_path(d, s)
    assert sorted(os.listdir(d)) == ["ckpt-00000006.pt", "ckpt-00000008.pt"]
    assert C.latest_checkpoint(d) == C.checkpoint_path(d, 8)
    got = C.load_checkpoint(C.latest_checkpoint(d))
    assert got["global_step"] == 8 and torch.equal(got["model"]["w"], torch.full((4,), 8.0))
    assert C.is_checkpoint(got) and C.model_state(got) is got["model"]
    assert C.model_state({"w": 1}) == {"w": 1}
    # past 10^8 steps the name widens and still sorts by step; unrelated files are ignored
    open(os.path.join(d, "ckpt-12.pt"), "w").close()
    open(os.path.join(d, "notes.txt"), "w").close()
    C.save_checkpoint(d, 123456789, _payload(1), keep=None)
    assert C.latest_checkpoint(d) == C.checkpoint_path(d, 123456789)
    assert [s for s, _ in C.list_checkpoints(d)] == [6, 8, 123456789]
    with pytest.raises(ValueError):
        C.save_checkpoint(d, 10, _payload(10), keep=0)


def test_an_interrupted_write_leaves_no_partial_file(tmp_path, monkeypatch):
    from heterofusionrcnn_amd import checkpoint as C
    d = str(tmp_path)
    C.save_checkpoint(d, 2, _payload(2), keep=1)
    real_save = torch.save

    def dies_half_way(obj, f, *a, **k):
        f.write(b"\x80\x02partial")
        raise KeyboardInterrupt

    monkeypatch.setattr(torch, "save", dies_half_way)
    with pytest.raises(KeyboardInterrupt):
        C.save_checkpoint(d, 4, _payload(4), keep=1)
    monkeypatch.setattr(torch, "save", real_save)
    assert os.listdir(d) == ["ckpt-00000002.pt"]            # no ckpt-00000004.pt, no temporary file, the old one kept
    assert C.load_checkpoint(C.latest_checkpoint(d))["global_step"] == 2


def test_non_finite_check_names_the_first_bad_step():
    from heterofusionrcnn_amd import checkpoint as C
    losses = [torch.tensor(v) for v in (1.0, 0.5, float("inf"), float("nan"))]
    assert C.first_nonfinite(losses[:2], 11) is None
    assert C.first_nonfinite(losses, 11) == 13
    keeper = C.Checkpointer(None, 2000, None, "c", {}, None, None, None, 10, print)
    keeper.check(losses[:2], 11)
    assert keeper.checked == 12
    with pytest.raises(FloatingPointError, match="global step 13"):
        keeper.check(losses, 11)


def test_resume_refuses_another_config_or_other_settings(tmp_path):
    from heterofusionrcnn_amd import checkpoint as C
    s = C.train_op_settings(1e-3, (20000, 0.8, True), 1.0, True)
    C.save_checkpoint(str(tmp_path), 4, dict(_payload(4), config="rpn_multiclass", settings=s))
    ck, path = C.resume_state(str(tmp_path), "rpn_multiclass", s)
    assert ck["global_step"] == 4 and path.endswith("ckpt-00000004.pt")
    with pytest.raises(ValueError, match="config"):
        C.resume_state(str(tmp_path), "rpn_multiclass_points", s)
    with pytest.raises(ValueError, match="settings"):
        C.resume_state(str(tmp_path), "rpn_multiclass", C.train_op_settings(1e-3, None, 0.0, False))
    with pytest.raises(FileNotFoundError):
        C.resume_state(str(tmp_path / "empty"), "rpn_multiclass", s)


# ------------------------------------------------------------------------------------------------ loader position
def test_sample_list_position_round_trip():
    from heterofusionrcnn_amd import kitti_data as KD
    names = ["000000", "000001", "000002", "000003"]
    a = KD.SampleList(GOLD_KITTI, names, KD.CLASSES, seed=5)
    a.take(3)
    saved = a.state_dict()
    raw = a.position()
    want = [a.take(3) for _ in range(7)]                   # crosses several epochs (8 samples each)
    b = KD.SampleList(GOLD_KITTI, names, KD.CLASSES, seed=99)
    b.load_state_dict(saved)
    assert [b.take(3) for _ in range(7)] == want
    c = KD.SampleList(GOLD_KITTI, names, KD.CLASSES, seed=99)
    c.load_state_dict(a.state_dict(raw))                   # a position recorded earlier, serialised later
    assert [c.take(3) for _ in range(7)] == want
    with pytest.raises(ValueError):
        KD.SampleList(GOLD_KITTI, names[:2], KD.CLASSES).load_state_dict(saved)


# ------------------------------------------------------------------------------------------------ the trainers' flags
@pytest.mark.parametrize("module", ["train_rpn", "train_rcnn"])
def test_cli_flags(module, monkeypatch):
    import importlib
    m = importlib.import_module("heterofusionrcnn_amd." + module)
    seen = []
    monkeypatch.setattr(m, "train", lambda *a, **k: (seen.append((a, k)), ([1.0], {}) if module == "train_rpn" else ([1.0], None))[1])
    pos = ["DATA"] if module == "train_rpn" else ["DATA", "HANDOFF"]
    assert m.main(pos + ["--steps", "5"]) == 0
    _, k = seen[-1]
    assert k["lr"] == 1e-3 and "clip_norm" not in k and "lr_decay" not in k and "tf_epsilon" not in k
    assert k["checkpoint_dir"] is None and k["checkpoint_every"] == 2000 and k["max_checkpoints"] is None and not k["resume"]
    assert m.main(pos + ["--reference-train-op", "--checkpoint-dir", "D", "--checkpoint-every", "7", "--max-checkpoints", "3",
                         "--resume", "--steps", "240000", "--lr", "5"]) == 0
    a, k = seen[-1]
    assert 240000 in a
    assert k["lr"] == pytest.approx(0.001) and k["clip_norm"] == 1.0 and k["lr_decay"] == (20000, 0.8, True)
    assert k["tf_epsilon"] is True and k["check_numerics"] is True
    assert k["checkpoint_dir"] == "D" and k["checkpoint_every"] == 7 and k["max_checkpoints"] == 3 and k["resume"] is True
    with pytest.raises(SystemExit):
        m.main(pos + ["--resume"])                         # nothing to resume from
    with pytest.raises(SystemExit):
        m.main(pos + ["--checkpoint-dir", "D", "--max-checkpoints", "0"])


def test_reference_train_op_values():
    from heterofusionrcnn_amd import checkpoint as C
    assert C.reference_train_op() == {"lr": 0.001, "lr_decay": (20000, 0.8, True), "clip_norm": 1.0, "tf_epsilon": True,
                                      "check_numerics": True}
    assert C.reference_train_op(8)["lr"] == pytest.approx(0.008)
    assert C.CHECKPOINT_INTERVAL == 2000
