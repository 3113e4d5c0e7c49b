"""CPU tests (-m "not gpu") of train_loop.run, the one loop of train_rpn.train and train_rcnn.train, driven by a recording fake stage
with the device-bound names of the loop's module substituted (MultiTensorAdam, TrainStep, GeometryPrefetcher, the generator-state
pair of checkpoint, torch.save): the order in which a fresh and a resumed run are put together, what happens when inside an
iteration, the meaning of `steps` under resume, the loader position a checkpoint records, close() on every way out and the
prefetcher's submit / get rhythm.  Every fake appends to one list of events; checkpoint files are real ones in tmp_path."""
import os
import shutil

import pytest
import torch

from heterofusionrcnn_amd import checkpoint as C
from heterofusionrcnn_amd import train_loop as TL

SETTINGS = dict(lr=1e-3, clip_norm=1.0, lr_decay=(2, 0.8, True), tf_epsilon=True)


class Batch:
    def __init__(self, k):                     # the k-th batch of the sample stream: global step k + 1 trains on it
        self.k, self.xyz, self.position = k, "xyz%d" % k, {"drawn": k}


class Loader:
    def __init__(self, ev, state):
        self.ev, self.drawn = ev, state["drawn"] if state else 0

    def next(self):
        self.ev.append(("next", self.drawn))
        self.drawn += 1
        return Batch(self.drawn - 1)

    def state_dict(self, position=None):
        self.ev.append(("position", position))
        return dict(position) if position is not None else {"drawn": self.drawn}

    def check_status(self):
        self.ev.append(("status",))
        return {"seen": self.drawn}

    def close(self):
        self.ev.append(("close",))


class Module(torch.nn.Module):
    def __init__(self, ev):
        super().__init__()
        self.ev, self.w = ev, torch.nn.Parameter(torch.ones(3))

    def load_state_dict(self, sd, strict=False):
        self.ev.append(("weights", strict))
        return super().load_state_dict(sd, strict=strict)


class Stage:
    """what train_loop.run asks of a stage; fail: the name of a method that raises; nan_at: the global step whose loss is NaN"""
    config = "fake"

    def __init__(self, ev, geometry=False, fail=None, nan_at=None):
        self.ev, self.fail, self.nan_at = ev, fail, nan_at
        self.geometry = None
        self._geometry = (lambda xyz: "geo:" + xyz) if geometry else None

    def open(self, state):
        self.ev.append(("open", state))
        return Loader(self.ev, state)

    def build(self, data):
        self.ev.append(("build",))
        if self.fail == "build":
            raise RuntimeError("build")
        self.geometry = self._geometry
        return Module(self.ev)

    def inputs(self, b):
        return {"k": b.k}

    def loss(self, m, inputs, geometry):
        g = inputs["k"] + 1
        return torch.tensor(float("nan") if g == self.nan_at else 1.0 / g), {"k": inputs["k"]}

    def log_parts(self, parts):
        return "k %d" % parts["k"]

    def epoch_status(self, i, data, log):
        self.ev.append(("epoch", i))

    def finish(self, status, log):
        self.ev.append(("finish", status))
        return "result"


@pytest.fixture
def ev(monkeypatch):
    """the list of events, with the loop's device-bound names replaced by fakes that record into it"""
    class Events(list):
        pass

    ev = Events()
    ev.fail = set()                           # names of the fakes that raise ("opt_state", "step_built", "step")

    class Adam:
        def __init__(self, params, lr, tf_epsilon, clip_norm, lr_decay):
            assert [tuple(p.shape) for p in params] == [(3,)]
            ev.append(("optimizer",))

        def load_state_dict(self, sd):
            ev.append(("opt_state",))
            if "opt_state" in ev.fail:
                raise ValueError("refused")

        def state_dict(self):
            return {"step_count": torch.tensor(0.0)}

        def lr_at(self, g):
            return 1e-3

    class Step:
        def __init__(self, module, opt, inputs, geometry, graph, loss_fn):
            ev.append(("step_built", inputs["k"], geometry))
            if "step_built" in ev.fail:
                raise RuntimeError("capture")
            self.module, self.loss_fn = module, loss_fn

        def __call__(self, geometry=None, **inputs):
            ev.append(("step", inputs["k"], geometry))
            if "step" in ev.fail and inputs["k"] == 1:
                raise RuntimeError("step")
            return self.loss_fn(self.module, inputs, geometry)

    class Prefetcher:
        def __init__(self, fn, depth):
            ev.append(("prefetcher", depth))
            self.fn, self.queue = fn, []

        def submit(self, xyz):
            ev.append(("submit", xyz))
            self.queue.append(self.fn(xyz))

        def get(self):
            ev.append(("get",))
            return self.queue.pop(0)

    class Keeper(C.Checkpointer):
        def __init__(self, *a):
            ev.append(("keeper",))
            super().__init__(*a)

        def check(self, losses, first_step):
            ev.append(("check", first_step + len(losses) - 1))
            super().check(losses, first_step)

    real_save = torch.save

    def save(obj, f, *a, **k):
        if isinstance(f, str):
            ev.append(("save", f))
        else:
            real_save(obj, f, *a, **k)          # a checkpoint, through checkpoint.save_checkpoint's open file

    def recorded(name, fn):
        return lambda *a, **k: (ev.append((name,)), fn(*a, **k))[1]

    monkeypatch.setattr(TL, "MultiTensorAdam", Adam)
    monkeypatch.setattr(TL, "TrainStep", Step)
    monkeypatch.setattr(TL, "GeometryPrefetcher", Prefetcher)
    monkeypatch.setattr(C, "rng_states", lambda: {"cpu": torch.zeros(2, dtype=torch.uint8)})
    monkeypatch.setattr(C, "load_rng_states", lambda states: ev.append(("rng",)))
    monkeypatch.setattr(torch, "save", save)
    monkeypatch.setattr(C, "Checkpointer", Keeper)
    monkeypatch.setattr(C, "train_op_settings", recorded("settings", C.train_op_settings))
    monkeypatch.setattr(C, "resume_state", recorded("resume_state", C.resume_state))
    monkeypatch.setattr(C, "load_drop_states", recorded("drop_states", C.load_drop_states))
    monkeypatch.setattr(torch, "manual_seed", recorded("seed", torch.manual_seed))
    return ev


def run(ev, stage, steps, **kw):
    a = dict(SETTINGS, seed=0, save=None, log_every=0, graph=True, log=lambda s: ev.append(("log", s)), check_numerics=False,
             checkpoint_dir=None, checkpoint_every=2000, max_checkpoints=None, resume=False, precision="fp32")
    a.update(kw)
    return TL.run(stage, steps, **a)


def kinds(ev, *names):
    return [e for e in ev if e[0] in names]


@pytest.fixture
def step3(ev, tmp_path):
    """a directory holding the step-3 checkpoint of a 6-step run (the events of that run are dropped)"""
    full = str(tmp_path / "full")
    run(ev, Stage(ev), 6, checkpoint_dir=full, checkpoint_every=3)
    assert [s for s, _ in C.list_checkpoints(full)] == [3, 6]
    d = str(tmp_path / "resume")
    os.makedirs(d)
    shutil.copy(C.checkpoint_path(full, 3), d)
    del ev[:]
    return d


def assembly(ev):
    """the events up to the first iteration, without their details"""
    out = []
    for e in ev:
        if e[0] == "step":
            break
        out.append(e[0])
    return out


def test_a_fresh_run_is_put_together_in_order(ev):
    losses, result = run(ev, Stage(ev, geometry=True), 2, save="model.pt")
    assert assembly(ev) == ["settings", "seed", "open", "build", "next", "optimizer", "step_built", "keeper", "prefetcher", "submit",
                            "next", "get", "submit"]
    assert ev[2] == ("open", None) and kinds(ev, "step_built") == [("step_built", 0, "geo:xyz0")]
    assert losses == pytest.approx([1.0, 0.5]) and result == "result"
    # after the loop: the final status, close, what the stage does with the status, save
    assert [e[0] for e in ev[-4:]] == ["status", "close", "finish", "save"]
    assert ev[-2] == ("finish", {"seen": 2}) and ev[-1] == ("save", "model.pt")


def test_a_resumed_run_is_put_together_in_order(ev, step3):
    losses, _ = run(ev, Stage(ev, geometry=True), 6, checkpoint_dir=step3, resume=True, log_every=1)
    assert assembly(ev) == ["settings", "resume_state", "log", "seed", "open", "build", "weights", "drop_states", "next", "optimizer",
                            "opt_state", "step_built", "rng", "keeper", "prefetcher", "submit", "next", "get", "submit"]
    assert ev[2][1].startswith("resuming from %s (global step 3)" % C.checkpoint_path(step3, 3))
    assert kinds(ev, "open") == [("open", {"drawn": 3})] and kinds(ev, "weights") == [("weights", True)]
    names = [e[0] for e in ev]
    assert names.index("rng") > names.index("step_built") > names.index("opt_state")      # generator states last, Adam's first
    assert names.index("drop_states") < names.index("next")                                # weights and counters before a batch
    # `steps` is the final global step: three iterations, logged as global steps 4 to 6
    assert [e[1] for e in kinds(ev, "step")] == [3, 4, 5]
    assert [e[1].split(" loss")[0] for e in kinds(ev, "log")[1:]] == ["step 4", "step 5", "step 6"]
    assert losses == pytest.approx([1.0 / 4, 1.0 / 5, 1.0 / 6])


def test_resume_at_the_final_step_runs_nothing_and_closes(ev, step3):
    losses, result = run(ev, Stage(ev), 3, checkpoint_dir=step3, resume=True, log_every=1, check_numerics=True)
    assert losses == [] and result == "result"
    assert kinds(ev, "step") == [] and len(kinds(ev, "close")) == 1 and len(kinds(ev, "log")) == 1
    assert [s for s, _ in C.list_checkpoints(step3)] == [3]


def test_checks_logs_and_checkpoints_inside_the_iterations(ev, tmp_path):
    d = str(tmp_path / "ck")
    run(ev, Stage(ev), 6, checkpoint_dir=d, checkpoint_every=3, log_every=2, check_numerics=True)
    seen = [(e[0], e[1].split(" loss")[0].split("/")[-1]) if e[0] == "log" else e for e in kinds(ev, "check", "log", "position")]
    assert seen == [("check", 2), ("log", "step 2"),
                    ("check", 3), ("position", {"drawn": 3}), ("log", "ckpt-00000003.pt"),     # the batch of step 4
                    ("check", 4), ("log", "step 4"),
                    ("check", 6), ("log", "step 6"), ("check", 6), ("position", None), ("log", "ckpt-00000006.pt"),
                    ("check", 6)]
    assert [s for s, _ in C.list_checkpoints(d)] == [3, 6]
    assert C.load_checkpoint(C.checkpoint_path(d, 3))["loader"] == {"drawn": 3}
    assert C.load_checkpoint(C.checkpoint_path(d, 6))["loader"] == {"drawn": 6}
    assert kinds(ev, "log")[0][1].startswith("step 2 loss 0.50000 k 1  lr 0.001  ")
    assert kinds(ev, "log")[0][1].endswith(" ms/step")
    # within an iteration: the next batch, the step, (check, log), (checkpoint), the end-of-epoch hook
    i = ev.index(("step", 2, None))
    assert ev[i - 1] == ("next", 3) and ev[i + 1] == ("check", 3) and ev[i + 4] == ("epoch", 2)
    assert [e[1] for e in kinds(ev, "epoch")] == list(range(6)) and kinds(ev, "next")[-1] == ("next", 5)


@pytest.mark.parametrize("case", ["build", "opt_state", "step_built", "step", "check", "normal"])
def test_the_loader_is_closed_exactly_once(ev, step3, case):
    stage = Stage(ev, fail=case, nan_at=2 if case == "check" else None)
    ev.fail.add(case)
    kw = dict(checkpoint_dir=step3, resume=True) if case == "opt_state" else {}
    error = {"build": RuntimeError, "opt_state": ValueError, "step_built": RuntimeError, "step": RuntimeError,
             "check": FloatingPointError}.get(case)
    if error:
        with pytest.raises(error, match={"opt_state": "refused", "step_built": "capture", "check": "global step 2"}.get(case, case)):
            run(ev, stage, 6, log_every=1, check_numerics=True, save="model.pt", **kw)
        assert kinds(ev, "save") == [] and kinds(ev, "finish") == []
    else:
        run(ev, stage, 6, log_every=1, check_numerics=True, save="model.pt", **kw)
    assert len(kinds(ev, "open")) == 1 and len(kinds(ev, "close")) == 1


def test_the_prefetcher_runs_one_batch_ahead(ev):
    run(ev, Stage(ev, geometry=True), 3)
    assert kinds(ev, "prefetcher", "submit", "get", "step") == [
        ("prefetcher", 1), ("submit", "xyz0"),
        ("get",), ("submit", "xyz1"), ("step", 0, "geo:xyz0"),
        ("get",), ("submit", "xyz2"), ("step", 1, "geo:xyz1"),
        ("get",), ("step", 2, "geo:xyz2")]


def test_no_prefetcher_without_a_geometry_function(ev):
    stage = Stage(ev)
    stage.epoch_status = None
    run(ev, stage, 2)
    assert kinds(ev, "prefetcher", "submit", "get", "epoch") == []
    assert kinds(ev, "step_built", "step") == [("step_built", 0, None), ("step", 0, None), ("step", 1, None)]


def test_nan_loss_stops_the_run_before_the_next_checkpoint_and_the_save(ev, tmp_path):
    d = str(tmp_path / "ck")
    with pytest.raises(FloatingPointError, match="global step 4"):
        run(ev, Stage(ev, nan_at=4), 6, checkpoint_dir=d, checkpoint_every=2, check_numerics=True, save="model.pt")
    assert os.listdir(d) == ["ckpt-00000002.pt"]
    assert kinds(ev, "save") == [] and len(kinds(ev, "close")) == 1
