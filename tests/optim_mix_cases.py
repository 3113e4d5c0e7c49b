"""Scenario table, fp64 reference and wrong trajectories for optim.MultiTensorAdam's bookkeeping: which tensors a step updates, and from
which gradients, when eager steps, captures and graph replays are mixed on ONE optimizer.  tests/test_optim_mix.py runs the scenarios on
the GPU, tests/test_optim_mix_cases_cpu.py checks this module on any machine.  A plain helper module: NumPy only, it imports neither the
library nor a test, and every gradient value of every scenario comes from gradient() below.

The kernels are pinned elsewhere (tests/optim_cases.py); what is pinned here is the host code that tells them what to update.  The optimizer
keeps a table of (parameter, gradient, moments) addresses in device memory.  An eager step rewrites it when a gradient moved; a captured step
carries upload nodes that rewrite a table at every replay.  Two ways to get that wrong, neither of which any address-free test can see:
  stale eager    an eager step launches on the table the last replay left behind: it consumes the last replay's tensor set and whatever
                 values sit in that graph's gradient memory now
  stale replay   a replay launches on the table the last eager step uploaded: it consumes that step's tensor set and whatever values sit in
                 the eager gradients' memory now

A scenario is a list of Op(kind, graph, live, seed, where) on one optimizer over SHAPES:
  kind   "eager" (one step() outside a capture), "capture" (record one step() into graph `graph`; nothing executes), "replay" (of `graph`),
         "save" (state_dict() and a copy of the parameters), "load" (load_state_dict() of the saved state, the parameters copied back)
  live   the tensors that carry a gradient (a capture freezes its set; a replay repeats its graph's)
  seed   of that step's gradient values: every step has its own, so that a step that consumed another step's gradients shows
  where  eager only: "slots" (the gradients are static tensors, refilled per step: every eager key is the same, a cache hit is certain) or
         "fresh" (new tensors at addresses no other live tensor has: a certain miss)
and `grads`: how a graph gets its gradients.  "pool": the capture runs sum((p * slot_i).sum()).backward() with .grad = None, so each
gradient lives in the graph's own pool and equals slot_i bit for bit at every replay.  "slots": the capture records a bare step() on the
eager steps' static slots (the key can match at capture).

walk() follows a scenario with a symbolic memory (which seed's values each gradient location holds) and yields, per operation: the right
gradients, the gradients each failure mode would consume there (None where the mode cannot be expressed: no earlier replay / eager step, or
it would consume exactly the right gradients), the host uploads so far under the documented cache rule (an eager step uploads iff its
addresses differ from the last EAGER upload's; a capture always records one; a replay costs none), and coverage tags.  trajectories() turns
that into fp64 parameters after every operation: the right ones, and for every expressible failure the parameters had the bug acted at that
operation (and nowhere before).  The buggy code is never run for this.

reference(): TensorFlow's Adam in fp64 (tf_epsilon False: torch.optim.Adam's placement of epsilon), optionally per-tensor clip_by_norm of
the scaled gradient and exponential_decay of the rate, with the optimizer's documented rule for a tensor without a gradient: its moments
and its values stay, the single global step still advances."""
import collections
import functools

import numpy as np

SHAPES = [(3,), (64, 3), (16385,), (257, 129), (1, 1), (40000,)]          # tests/test_optim.py SHAPES[:6]: crosses a chunk edge (16384)
ALL = tuple(range(len(SHAPES)))
RTOL, ATOL = 3e-5, 3e-6             # the GPU test's tolerance against fp64 (tests/test_train_op.py, tests/test_optim.py)
SHARP = 100.0                       # a wrong trajectory must miss the right one by this many tolerances

Op = collections.namedtuple("Op", "kind graph live seed where")


def E(seed, live=ALL, where="slots"):
    return Op("eager", None, tuple(live), seed, where)


def C(graph, live=ALL):
    return Op("capture", graph, tuple(live), None, None)


def R(graph, seed):
    return Op("replay", graph, None, seed, None)


SAVE, LOAD = Op("save", None, None, None, None), Op("load", None, None, None, None)

PLAIN = dict(lr=1e-2, betas=(0.9, 0.999), eps=1e-8, tf_epsilon=True, grad_scale=1.0, clip_norm=0.0, lr_decay=None)
SCHED = dict(PLAIN, grad_scale=0.25, clip_norm=1.0, lr_decay=(3, 0.5))

_ERE = [E(1), C("A"), R("A", 2), E(3), R("A", 4), E(5), R("A", 6), E(7)]
NO2, NO3 = tuple(i for i in ALL if i != 2), tuple(i for i in ALL if i != 3)

SCENARIOS = {
    "eager_replay_eager": dict(grads="pool", hyper=PLAIN, ops=_ERE),
    "capture_on_matching_key": dict(grads="slots", hyper=PLAIN,
                                    ops=[E(1), C("A"), E(2, live=NO3), R("A", 3), E(4, where="fresh"), R("A", 5)]),
    "two_captures": dict(grads="pool", hyper=dict(PLAIN, tf_epsilon=False),
                         ops=[C("A"), C("B", live=NO2), R("A", 1), R("B", 2), E(3), R("B", 4), R("A", 5), E(6), R("A", 7)]),
    "sched": dict(grads="pool", hyper=SCHED, ops=_ERE),
    # eager gradients at fresh addresses: no step here depends on the cache, the scenario is about the state that is put back
    "reload": dict(grads="pool", hyper=PLAIN,
                   ops=[E(1, where="fresh"), C("A"), R("A", 2), SAVE, R("A", 3), E(4, where="fresh"), R("A", 5), LOAD,
                        R("A", 6), E(7, where="fresh"), R("A", 8)]),
}
COVERAGE = ("eager_hit_after_replay", "replay_after_eager_rewrite", "capture_on_matching_key", "two_graphs_with_different_sets")


# ------------------------------------------------------------------------------------------------------------------ values
def initial_params(seed=0):
    return [np.random.default_rng([seed, i]).standard_normal(s).astype(np.float32) for i, s in enumerate(SHAPES)]


def norm_factor(i, step):
    """tests/test_train_op.py's _norm_factor for these six tensors: the L2 norm of tensor i's scaled gradient in units of the clip norm --
    under it, a hair under and over it, far over it, an all-zero tensor, and norms that move between steps"""
    return [0.3 * (1 + 4 * (step % 2)), 0.999, 1.001, 50.0 * (1 + step), 0.0, 0.3][i]


@functools.lru_cache(maxsize=None)
def _gradient(seed, i, clip_norm, grad_scale):
    g = np.random.default_rng([1000 + seed, i]).standard_normal(SHAPES[i])
    if clip_norm > 0:
        f = norm_factor(i, seed) * clip_norm
        g = g / np.sqrt((g * g).sum()) * f / grad_scale if f > 0 else np.zeros(SHAPES[i])
    g = g.astype(np.float32)
    g.setflags(write=False)
    return g


def gradient(seed, i, hyper):
    """the fp32 gradient of tensor i at the step with this seed (read-only, shared).  Without clipping: independent standard normals;
    with it: scaled as _gradients of tests/test_train_op.py does, so that some tensors clip and some do not"""
    return _gradient(seed, i, float(hyper["clip_norm"]), float(hyper["grad_scale"]))


# ------------------------------------------------------------------------------------------------------------------ reference
class Ref:
    """the optimizer's state in fp64: parameters, both moments, the global step"""

    def __init__(self, p0, hyper):
        self.p = [np.asarray(a, dtype=np.float64).copy() for a in p0]
        self.m = [np.zeros_like(a) for a in self.p]
        self.v = [np.zeros_like(a) for a in self.p]
        self.t, self.hyper = 0, hyper

    def copy(self):
        c = Ref(self.p, self.hyper)
        c.m, c.v, c.t = [a.copy() for a in self.m], [a.copy() for a in self.v], self.t
        return c

    def step(self, grads):
        """grads: {tensor index: gradient}; a tensor that is missing keeps parameters and moments, the step counts all the same"""
        h = self.hyper
        b1, b2 = h["betas"]
        self.t += 1
        t, lr = self.t, h["lr"]
        if h["lr_decay"] is not None:
            steps, factor = h["lr_decay"][:2]
            lr = lr * factor ** np.floor((t - 1) / steps)                       # staircase, Adam step t runs at global step t - 1
        for i, g in grads.items():
            x = np.asarray(g, dtype=np.float64) * h["grad_scale"]
            if h["clip_norm"] > 0:
                x = x * h["clip_norm"] / max(np.sqrt((x * x).sum()), h["clip_norm"])
            self.m[i] = b1 * self.m[i] + (1 - b1) * x
            self.v[i] = b2 * self.v[i] + (1 - b2) * x * x
            if h["tf_epsilon"]:
                self.p[i] = self.p[i] - lr * np.sqrt(1 - b2 ** t) / (1 - b1 ** t) * self.m[i] / (np.sqrt(self.v[i]) + h["eps"])
            else:
                self.p[i] = self.p[i] - lr / (1 - b1 ** t) * self.m[i] / (np.sqrt(self.v[i]) / np.sqrt(1 - b2 ** t) + h["eps"])
        return [a.copy() for a in self.p]


def reference(p0, steps, hyper):
    """the parameters after every step, in fp64.  steps: one {tensor index: gradient} per step"""
    ref = Ref(p0, hyper)
    return [ref.step(g) for g in steps]


# ------------------------------------------------------------------------------------------------------------------ the walk
def walk(name):
    """one record per operation of the scenario, see the module docstring.  A gradient set is {tensor index: seed}"""
    sc = SCENARIOS[name]
    mem = collections.defaultdict(dict)            # location -> {tensor: the seed whose values it holds}
    graphs = {}                                    # name -> (location, live)
    eager_key, uploads, steps = None, 0, 0
    last_eager = last_replay = None                # (location, live) of the table that step launched on
    replayed_since_upload, rewritten_since = False, {}
    saved_steps = None
    out = []
    for k, op in enumerate(sc["ops"]):
        rec = dict(index=k, op=op, right=None, stale_eager=None, stale_replay=None, tags=set())
        if op.kind == "eager":
            loc = "slots" if op.where == "slots" else ("fresh", k)
            for i in op.live:
                mem[loc][i] = op.seed
            rec["right"] = {i: op.seed for i in op.live}
            if last_replay is not None:
                rec["stale_eager"] = {i: mem[last_replay[0]][i] for i in last_replay[1]}
            if (loc, op.live) == eager_key:
                if replayed_since_upload:
                    rec["tags"].add("eager_hit_after_replay")
            else:
                eager_key, uploads, replayed_since_upload = (loc, op.live), uploads + 1, False
                rewritten_since = {g: True for g in graphs}
            last_eager = (loc, op.live)
            steps += 1
        elif op.kind == "capture":
            assert op.graph not in graphs
            loc = "slots" if sc["grads"] == "slots" else ("pool", op.graph)
            graphs[op.graph] = (loc, op.live)
            if (loc, op.live) == eager_key:
                rec["tags"].add("capture_on_matching_key")
            if any(live != op.live for _, live in graphs.values()):
                rec["tags"].add("two_graphs_with_different_sets")
            rewritten_since[op.graph] = False
            uploads += 1                           # a capture always records its own upload
        elif op.kind == "replay":
            loc, live = graphs[op.graph]
            for i in live:
                mem[loc][i] = op.seed
            rec["right"] = {i: op.seed for i in live}
            if last_eager is not None:
                rec["stale_replay"] = {i: mem[last_eager[0]][i] for i in last_eager[1]}
            if rewritten_since[op.graph]:
                rec["tags"].add("replay_after_eager_rewrite")
            last_replay, replayed_since_upload = (loc, live), True
            steps += 1
        elif op.kind == "save":
            saved_steps = steps
        elif op.kind == "load":
            steps = saved_steps
        for mode in ("stale_eager", "stale_replay"):
            if rec[mode] == rec["right"]:
                rec[mode] = None                   # the mode cannot be expressed here: it would consume the right gradients
        rec["steps"], rec["uploads"] = steps, uploads
        out.append(rec)
    return out


def trajectories(name, p0=None):
    """(right, wrong): right[k] = the fp64 parameters after operation k; wrong = [(k, mode, parameters after operation k had that failure
    acted at k, everything before it being right)]"""
    hyper = SCENARIOS[name]["hyper"]
    ref, saved = Ref(initial_params() if p0 is None else p0, hyper), None
    right, wrong = [], []
    for rec in walk(name):
        kind = rec["op"].kind
        if kind == "save":
            saved = ref.copy()
        elif kind == "load":
            ref = saved.copy()
        elif rec["right"] is not None:
            for mode in ("stale_eager", "stale_replay"):
                if rec[mode] is not None:
                    wrong.append((rec["index"], mode, ref.copy().step({i: gradient(s, i, hyper) for i, s in rec[mode].items()})))
            ref.step({i: gradient(s, i, hyper) for i, s in rec["right"].items()})
        right.append([a.copy() for a in ref.p])
    return right, wrong


def miss(got, want):
    """the largest |got - want| over all tensors, in units of the tolerance atol + rtol |want|"""
    return max(float(np.max(np.abs(np.asarray(g, dtype=np.float64) - w) / (ATOL + RTOL * np.abs(w)))) for g, w in zip(got, want))
