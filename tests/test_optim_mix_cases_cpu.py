"""tests/optim_mix_cases.py on any machine: the scenario table is well formed and reaches the four situations it exists for, the fp64
reference is Adam (torch.optim.Adam's placement of epsilon, TensorFlow's formula with clip_by_norm and staircase decay, the rule for a
tensor without a gradient), and every scenario is sharp: a step that consumed the other form's table misses the GPU test's tolerance by
a factor of 100 at the very operation where it happens."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import optim_mix_cases as mc  # noqa: E402

NAMES = list(mc.SCENARIOS)
_TRAJ = {}


def _trajectories(name):
    if name not in _TRAJ:
        _TRAJ[name] = mc.trajectories(name)
    return _TRAJ[name]


# ------------------------------------------------------------------------------------------------------------------ the table
def test_the_table_holds_the_five_scenarios_over_the_first_six_shapes():
    assert NAMES == ["eager_replay_eager", "capture_on_matching_key", "two_captures", "sched", "reload"]
    assert mc.SHAPES == [(3,), (64, 3), (16385,), (257, 129), (1, 1), (40000,)]
    assert (mc.RTOL, mc.ATOL, mc.SHARP) == (3e-5, 3e-6, 100.0)


@pytest.mark.parametrize("name", NAMES)
def test_scenario_is_well_formed(name):
    sc = mc.SCENARIOS[name]
    assert sc["grads"] in ("pool", "slots") and set(sc["hyper"]) == set(mc.PLAIN)
    captured, seeds, saved = {}, [], False
    for op in sc["ops"]:
        assert op.kind in ("eager", "capture", "replay", "save", "load")
        if op.kind == "eager":
            assert op.where in ("slots", "fresh") and op.graph is None
        if op.kind in ("eager", "capture"):
            assert op.live and set(op.live) <= set(mc.ALL) and list(op.live) == sorted(set(op.live))
        if op.kind == "capture":
            assert op.graph not in captured and op.seed is None                  # a capture executes nothing: no values of its own
            captured[op.graph] = op.live
        if op.kind == "replay":
            assert op.graph in captured, "replay of a graph that was never captured"
        if op.kind in ("eager", "replay"):
            seeds.append(op.seed)
        if op.kind == "load":
            assert saved
        saved = saved or op.kind == "save"
    assert len(set(seeds)) == len(seeds), "every step has gradient values of its own"
    assert len(captured) <= 2, "the optimizer reserves staging for two captures between eager steps"
    recs = mc.walk(name)
    assert [r["index"] for r in recs] == list(range(len(sc["ops"])))
    assert recs[-1]["uploads"] <= len(captured) + sum(op.kind == "eager" for op in sc["ops"])


def test_the_scenarios_are_the_sequences_the_issue_names():
    kinds = {n: "".join(dict(eager="E", capture="C", replay="R", save="s", load="l")[op.kind] + (op.graph or "")
                        for op in mc.SCENARIOS[n]["ops"]) for n in NAMES}
    assert kinds["eager_replay_eager"] == kinds["sched"] == "ECARAERAERAE"
    assert kinds["capture_on_matching_key"] == "ECAERAERA"
    assert kinds["two_captures"] == "CACBRARBERBRAERA"
    assert kinds["reload"] == "ECARAsRAERAlRAERA"
    ops = mc.SCENARIOS["capture_on_matching_key"]["ops"]
    assert mc.SCENARIOS["capture_on_matching_key"]["grads"] == "slots"
    assert 3 not in ops[2].live and len(ops[2].live) == 5 and ops[4].where == "fresh" and ops[4].live == mc.ALL
    two = mc.SCENARIOS["two_captures"]["ops"]
    assert two[0].live == mc.ALL and 2 not in two[1].live and len(two[1].live) == 5
    h = mc.SCENARIOS["sched"]["hyper"]
    assert (h["clip_norm"], h["lr_decay"], h["grad_scale"]) == (1.0, (3, 0.5), 0.25)
    # reload: saved after step 2, loaded after step 5, three more steps
    steps = [r["steps"] for r in mc.walk("reload")]
    ops = mc.SCENARIOS["reload"]["ops"]
    assert steps[[op.kind for op in ops].index("save")] == 2 and steps[[op.kind for op in ops].index("load") - 1] == 5
    assert steps[-1] == 5 and [op.kind for op in ops[-3:]] == ["replay", "eager", "replay"]


def test_the_table_reaches_all_four_situations():
    tags = {n: set().union(*(r["tags"] for r in mc.walk(n))) for n in NAMES}
    assert set().union(*tags.values()) == set(mc.COVERAGE)
    assert "eager_hit_after_replay" in tags["eager_replay_eager"] and "eager_hit_after_replay" in tags["sched"]
    assert "eager_hit_after_replay" in tags["two_captures"] and "two_graphs_with_different_sets" in tags["two_captures"]
    assert "replay_after_eager_rewrite" in tags["capture_on_matching_key"] and "capture_on_matching_key" in tags["capture_on_matching_key"]
    assert not tags["reload"] & {"eager_hit_after_replay", "capture_on_matching_key"}     # reload is about the state alone
    # both graphs of two_captures are replayed, before and after an eager step
    ops = mc.SCENARIOS["two_captures"]["ops"]
    first_eager = [op.kind for op in ops].index("eager")
    for g in "AB":
        assert any(op.kind == "replay" and op.graph == g for op in ops[:first_eager])
        assert any(op.kind == "replay" and op.graph == g for op in ops[first_eager:])


def test_uploads_under_the_documented_cache_rule():
    """eager steps on unmoved gradients upload once, a capture records one upload, a replay none"""
    assert [r["uploads"] for r in mc.walk("eager_replay_eager")] == [1, 2, 2, 2, 2, 2, 2, 2]
    assert [r["uploads"] for r in mc.walk("capture_on_matching_key")] == [1, 2, 3, 3, 4, 4]
    assert [r["uploads"] for r in mc.walk("two_captures")] == [1, 2, 2, 2, 3, 3, 3, 3, 3]
    assert mc.walk("reload")[-1]["uploads"] == 4


# ------------------------------------------------------------------------------------------------------------------ the reference
def _few_line_adam(p, grads, lr, b1, b2, eps, scale=1.0, clip=None, decay=None, torch_eps=False):
    """one tensor, written independently of mc.Ref: clip_by_norm, staircase decay, Adam; a gradient of None skips the tensor"""
    p = np.array(p, dtype=np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for t, g in enumerate(grads, start=1):
        if g is None:
            continue
        x = np.array(g, dtype=np.float64) * scale
        if clip is not None and np.linalg.norm(x) > clip:
            x *= clip / np.linalg.norm(x)
        m += (1 - b1) * (x - m)
        v += (1 - b2) * (x * x - v)
        rate = lr * (decay[1] ** ((t - 1) // decay[0]) if decay else 1.0)
        mhat, vhat = m / (1 - b1 ** t), v / (1 - b2 ** t)
        p -= rate * mhat / (np.sqrt(vhat) + eps) if torch_eps else rate * mhat / (np.sqrt(vhat) + eps / np.sqrt(1 - b2 ** t))
    return p


def test_reference_is_torch_adam_where_tf_epsilon_is_off():
    hyper = dict(mc.PLAIN, tf_epsilon=False, lr=3e-3)
    p0 = mc.initial_params(5)
    steps = [{i: mc.gradient(s, i, hyper) * 10.0 ** (s % 3 - 1) for i in mc.ALL} for s in range(9)]
    mine = mc.reference(p0, steps, hyper)[-1]
    ps = [torch.from_numpy(a).double().requires_grad_(True) for a in p0]
    opt = torch.optim.Adam(ps, lr=3e-3, betas=(0.9, 0.999), eps=1e-8)
    for gs in steps:
        for i, p in enumerate(ps):
            p.grad = torch.from_numpy(np.array(gs[i])).double()
        opt.step()
    for a, p in zip(mine, ps):
        np.testing.assert_allclose(a, p.detach().numpy(), rtol=1e-12, atol=1e-14)
    # epsilon placement matters at this size: eps 1e-3 separates the two forms far beyond that bound
    big = dict(hyper, eps=1e-3)
    assert mc.miss(mc.reference(p0, steps, big)[-1], mc.reference(p0, steps, dict(big, tf_epsilon=True))[-1]) > mc.SHARP


@pytest.mark.parametrize("hyper", [mc.PLAIN, mc.SCHED, dict(mc.SCHED, tf_epsilon=False), dict(mc.PLAIN, eps=1e-3)])
def test_reference_against_a_few_line_loop_on_one_tensor(hyper):
    p0 = mc.initial_params(2)
    for i in (1, 3):                                                   # norms around the clip norm / far over it
        seq = [s if s != 4 else None for s in range(1, 9)]              # step 4: no gradient
        steps = [({i: mc.gradient(s, i, hyper)} if s is not None else {}) for s in seq]
        want = _few_line_adam(p0[i], [None if s is None else mc.gradient(s, i, hyper) for s in seq], hyper["lr"], *hyper["betas"],
                              hyper["eps"], hyper["grad_scale"], hyper["clip_norm"] or None, hyper["lr_decay"], not hyper["tf_epsilon"])
        traj = mc.reference(p0, steps, hyper)
        np.testing.assert_allclose(traj[-1][i], want, rtol=1e-11, atol=1e-13)
        # the skipped step: the tensor keeps its bits, and the global step advanced (step 5's bias correction is that of t = 5)
        assert np.array_equal(traj[3][i], traj[2][i]) and not np.array_equal(traj[4][i], traj[3][i])
        for j in mc.ALL:
            if j != i:
                assert np.array_equal(traj[-1][j], p0[j].astype(np.float64))


def test_scheduled_gradients_clip_some_tensors_and_not_others():
    h = mc.SCHED
    for seed in (1, 2):
        norms = [float(np.linalg.norm(mc.gradient(seed, i, h).astype(np.float64) * h["grad_scale"])) for i in mc.ALL]
        want = [mc.norm_factor(i, seed) for i in mc.ALL]
        np.testing.assert_allclose(norms, want, rtol=1e-6)
        assert norms[1] < h["clip_norm"] < norms[2] and norms[4] == 0.0 and norms[3] > 50
    assert mc.gradient(1, 2, mc.PLAIN) is mc.gradient(1, 2, mc.PLAIN) and not mc.gradient(1, 2, mc.PLAIN).flags.writeable


def test_reload_restarts_from_the_saved_step():
    right, _ = _trajectories("reload")
    ops = mc.SCENARIOS["reload"]["ops"]
    kinds = [op.kind for op in ops]
    s, l = kinds.index("save"), kinds.index("load")
    assert all(np.array_equal(a, b) for a, b in zip(right[l], right[s]))
    h = mc.SCENARIOS["reload"]["hyper"]
    order = [op for op in ops[:s] if op.seed is not None] + [op for op in ops[l:] if op.seed is not None]
    live = lambda op: mc.ALL if op.kind == "replay" else op.live
    want = mc.reference(mc.initial_params(), [{i: mc.gradient(op.seed, i, h) for i in live(op)} for op in order], h)[-1]
    assert all(np.array_equal(a, b) for a, b in zip(right[-1], want))
    assert mc.miss(right[l - 1], right[-1]) > mc.SHARP                              # the steps that were undone mattered


# ------------------------------------------------------------------------------------------------------------------ sharpness
@pytest.mark.parametrize("name", NAMES)
def test_a_stale_table_misses_the_tolerance_a_hundredfold_where_it_first_acts(name):
    right, wrong = _trajectories(name)
    modes = {mode for _, mode, _ in wrong}
    assert modes == {"stale_eager", "stale_replay"}, "every scenario mixes both forms, so it can express both failures"
    for k, mode, params in wrong:
        gap = mc.miss(params, right[k])
        assert gap >= mc.SHARP, "%s: %s at operation %d misses by only %.1f tolerances" % (name, mode, k, gap)


def test_every_expressible_failure_of_every_stepping_operation_is_listed():
    for name in NAMES:
        recs = mc.walk(name)
        _, wrong = _trajectories(name)
        assert [(k, m) for k, m, _ in wrong] == [(r["index"], m) for r in recs for m in ("stale_eager", "stale_replay") if r[m] is not None]
        seen_replay = seen_eager = False
        for r in recs:
            if r["op"].kind == "eager":
                # inexpressible only before the first replay, or when the stale table would name the same memory and tensors
                assert r["stale_eager"] is not None or not seen_replay or mc.SCENARIOS[name]["grads"] == "slots"
                seen_eager = True
            if r["op"].kind == "replay":
                assert r["stale_replay"] is not None or not seen_eager
                seen_replay = True
    # the operations at which the parent's cache would have gone wrong are among them
    assert {(5, "stale_eager"), (7, "stale_eager")} <= {(k, m) for k, m, _ in _trajectories("eager_replay_eager")[1]}
    assert {(3, "stale_replay"), (5, "stale_replay")} <= {(k, m) for k, m, _ in _trajectories("capture_on_matching_key")[1]}
    assert (7, "stale_eager") in {(k, m) for k, m, _ in _trajectories("two_captures")[1]}
