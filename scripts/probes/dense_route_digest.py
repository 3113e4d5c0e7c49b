"""One SHA-256 per dense / BatchNorm route of mlp.py and pointcnn.py, for telling two trees of the package apart bit by bit.

  python scripts/probes/dense_route_digest.py [--values OUT.pt] > digests.json

Every entry builds its modules and draws its tensors from a seed of its own, in a fixed order (the dropout seeds of BatchNormReLU follow
the order in which layers are built), runs forward and -- where the route has one -- backward, and hashes, in this order: the outputs,
the gradients of the inputs, the gradients of the parameters, the running statistics afterwards.  Only public names and the private
names the tests already use are touched, so the same file runs against an older tree (DENSE_DIGEST_TREE = its root) with the same
libhfops.so (HFOPS_LIBRARY).  --values also saves the hashed tensors, for comparing values where two runs of one tree already differ:
the entries that scatter a gradient with atomicAdd (shared_mlp_grouped/train/c32/*: hf_group_point_grad; PointCnnBackbone/train/with_x:
the X-Conv weight gradients) do, by a few ulps (profiles/dense_launch_sites_ab.md).  "_routes" holds, per entry, how often each autograd
node (and linear_bn_fwd, _lift_chain_eval) ran in it; the entries that are named after a route assert theirs (took=...), so a shape
that falls to another branch fails here instead of hashing the wrong thing.  "_nodes" is the same count over the two backbones.
Small shapes: 32768 rows where a route asks for FUSED_FWD_MIN_ROWS, 4096 for the library-GEMM branches, 3 / 6 / 32 / 64 channels
(257 -> 128 once: cin % 4 != 0), K = 8, B = 2, 4096 x 256 x 256 for bf16."""
import argparse
import collections
import dataclasses
import hashlib
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.environ.get("DENSE_DIGEST_TREE") or os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import heterofusionrcnn_amd as hf  # noqa: E402
from heterofusionrcnn_amd import mlp, pointcnn  # noqa: E402
from heterofusionrcnn_amd.modules import PointnetFPModule, SharedMLPLayer  # noqa: E402

TALL, SHORT = 32768, 4096
RESULTS, VALUES = collections.OrderedDict(), collections.OrderedDict()
RESULTS["_routes"] = {}
CALLS, SEEN = collections.Counter(), collections.Counter()


def count_routes():
    """count the forward calls of every autograd node of the two modules, and of the two route functions that are no node"""
    def counting(f, name):
        def run(*a, **k):
            CALLS[name] += 1
            return f(*a, **k)
        return run
    for module in (mlp, pointcnn):
        for name, cls in sorted(vars(module).items()):
            if isinstance(cls, type) and issubclass(cls, torch.autograd.Function) and cls.__module__ == module.__name__:
                cls.forward = staticmethod(counting(cls.forward, name))
    mlp.linear_bn_fwd = counting(mlp.linear_bn_fwd, "linear_bn_fwd")
    pointcnn._lift_chain_eval = counting(pointcnn._lift_chain_eval, "_lift_chain_eval")


def _flat(ts):
    return [t for t in ts if t is not None]


def record(name, outputs, inputs=(), modules=(), params=(), took=None):
    """hash outputs | input gradients | parameter gradients | buffers; backward (seeded cotangents) when an output carries a graph.
    took: {node or function: calls} this entry must have made since the entry before it (0: must not have run)"""
    outputs = list(outputs)
    ran = {k: CALLS[k] - SEEN[k] for k in sorted(CALLS) if CALLS[k] != SEEN[k]}
    SEEN.update({k: CALLS[k] - SEEN[k] for k in CALLS})
    assert all(ran.get(k, 0) == v for k, v in (took or {}).items()), (name, took, ran)
    RESULTS["_routes"][name] = ran
    live = [o for o in outputs if o.requires_grad]
    if live:
        g = torch.Generator().manual_seed(len(RESULTS) + 1)
        torch.autograd.backward(live, [torch.randn(o.shape, generator=g).to(o.device) for o in live])
    params = list(params) + [p for m in modules for p in m.parameters()]
    buffers = [b for m in modules for b in m.buffers()]
    parts = [("out", outputs), ("dinput", [t.grad for t in _flat(inputs)]), ("dparam", [p.grad for p in params]), ("buffers", buffers)]
    torch.cuda.synchronize()
    h, kept = hashlib.sha256(), []
    for tag, ts in parts:
        for i, t in enumerate(ts):
            h.update(("%s%d:" % (tag, i)).encode())
            if t is None:
                h.update(b"none")
                continue
            a = t.detach().contiguous().cpu()
            h.update(("%s%s" % (a.dtype, tuple(a.shape))).encode())
            h.update(a.view(torch.uint8).numpy().tobytes() if a.numel() else b"")
            kept.append(a)
    assert name not in RESULTS, name
    RESULTS[name], VALUES[name] = h.hexdigest(), kept


def rand(*shape, seed, grad=False, shift=0.0):
    t = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) + shift).cuda()
    return t.requires_grad_(True) if grad else t


def randomise(bn, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(bn.num_features, generator=g) + 0.5)
        bn.bias.copy_(torch.rand(bn.num_features, generator=g) * 0.6 - 0.3)
        bn.running_mean.copy_(torch.randn(bn.num_features, generator=g) * 0.3)
        bn.running_var.copy_(torch.rand(bn.num_features, generator=g) * 4 + 0.5)


def shared_layers(seed, widths, cin, last_relu=True):
    torch.manual_seed(seed)
    layers = []
    for i, w in enumerate(widths):
        layers.append(SharedMLPLayer(cin, w, relu=last_relu or i < len(widths) - 1).cuda().train())
        cin = w
    for i, l in enumerate(layers):
        randomise(l.bn, seed * 100 + i)
        with torch.no_grad():
            l.fc.bias.uniform_(-0.1, 0.1)
    return layers


def mode(layers, training):
    for l in layers:
        l.train(training)


# ------------------------------------------------------------------------------------------------ BatchNormReLU and the single layers
def batchnorm_entries():
    for tag, kw in (("relu", dict(relu=True)), ("elu_in", dict(relu=False, elu_in=True))):
        torch.manual_seed(11)
        bn = mlp.BatchNormReLU(32, **kw).cuda().train()
        randomise(bn, 12)
        for what, drop in (("train", 0.0), ("train_dropout", 0.5)):
            bn.zero_grad(set_to_none=True)
            x = rand(SHORT, 32, seed=13, grad=True, shift=0.2)
            record("BatchNormReLU/%s/%s" % (tag, what), [bn(x, dropout=drop)], [x], [bn],
                   took={"_BNDropoutTrain" if drop else "_BNReLUTrain": 1})
        bn.eval().zero_grad(set_to_none=True)
        with torch.no_grad():
            record("BatchNormReLU/%s/eval" % tag, [bn(rand(SHORT, 32, seed=14))], [], [bn])


def single_layer_entries():
    torch.manual_seed(21)
    bn = mlp.BatchNormReLU(64).cuda().train()
    randomise(bn, 22)
    w, b = rand(64, 32, seed=23, grad=True), rand(64, seed=24, grad=True)
    x = rand(SHORT, 32, seed=25, grad=True)
    record("linear_bn_relu/train", [mlp.linear_bn_relu(x, w, b, bn)], [x], [bn], [w, b], took={"_LinearBNReLU": 1})
    for t in (w, b, x):
        t.grad = None
    bn.zero_grad(set_to_none=True)
    record("linear_bn_relu_maxpool/train", [mlp.linear_bn_relu_maxpool(x, w, b, bn, 8)], [x], [bn], [w, b],
           took={"_LinearBNReLUMaxPool": 1})
    bn.eval()
    with torch.no_grad():
        record("linear_bn_relu_maxpool/eval", [mlp.linear_bn_relu_maxpool(x.detach(), w.detach(), b.detach(), bn, 8)], [], [bn])
    w2, b2, x2 = rand(2, 64, seed=26, grad=True), rand(2, seed=27, grad=True), rand(SHORT, 64, seed=28, grad=True)
    record("linear_narrow", [mlp.linear_narrow(x2, w2, b2)], [x2], [], [w2, b2], took={"_NarrowLinear": 1})
    for rows, tag in ((SHORT, "splitk"), (TALL, "mfma_narrow_output")):
        w3, x3 = rand(64, 32, seed=29, grad=True), rand(rows, 32, seed=30, grad=True)
        record("linear_nobias/%s" % tag, [mlp.linear_nobias(x3, w3)], [x3], [], [w3],
               took={"_LinearSplitK": 1, "linear_bn_fwd": int(rows == TALL)})


# ------------------------------------------------------------------------------------------------ shared MLPs
def shared_mlp_entries():
    for rows in (TALL, SHORT):
        for pool_k in (0, 8):
            layers = shared_layers(31, (32, 64), 6)
            x = rand(rows, 6, seed=32, grad=True)
            record("shared_mlp/train/rows%d/pool%d" % (rows, pool_k), [mlp.shared_mlp(layers, x, pool_k=pool_k)], [x], layers,
                   took={"_SharedMLPChain": 1, "linear_bn_fwd": 2 * (rows == TALL)})
            mode(layers, False)
            with torch.no_grad():
                record("shared_mlp/eval/rows%d/pool%d" % (rows, pool_k), [mlp.shared_mlp(layers, x.detach(), pool_k=pool_k)], [], layers,
                       took={"_SharedMLPChain": 0, "linear_bn_fwd": 2 * (rows == TALL)})
    layers = shared_layers(33, (32, 64), 6)
    x = torch.nn.functional.pad(rand(SHORT, 6, seed=34), (0, 2)).requires_grad_(True)       # two zero columns appended by the producer
    record("shared_mlp/train/padded_input", [mlp.shared_mlp(layers, x, pool_k=8)], [x], layers, took={"_SharedMLPChain": 1})
    layers = shared_layers(35, (32, 64), 6, last_relu=False)
    x = rand(SHORT, 6, seed=36, grad=True)
    record("shared_mlp/layer_by_layer/train", [mlp.shared_mlp(layers, x)], [x], layers, took={"_SharedMLPChain": 0})
    layers = shared_layers(37, (32, 64), 6)
    mode(layers, False)
    x = rand(SHORT, 6, seed=38, grad=True)
    record("shared_mlp/layer_by_layer/eval_with_autograd/pool8", [mlp.shared_mlp(layers, x, pool_k=8)], [x], layers,
           took={"_SharedMLPChain": 0})


def grouped_entries():
    rng = np.random.default_rng(41)
    xyz = torch.from_numpy(rng.random((2, 4096, 3), dtype=np.float32)).cuda()
    new_xyz = hf.gather_point(xyz, hf.farthest_point_sample(2048, xyz))
    idx, _, gxyz = hf.query_ball_group(0.25, 8, xyz, new_xyz, center=True)                   # 2 x 2048 x 8 = 32768 rows
    for c in (0, 32):
        for pool in (True, False):
            layers = shared_layers(42 + c, (32, 64), c + 3)
            pts = rand(2, 4096, c, seed=43, grad=True) if c else None
            tag = "c%d/%s" % (c, "pool" if pool else "rows")
            record("shared_mlp_grouped/train/" + tag, [mlp.shared_mlp_grouped(layers, pts, idx, gxyz, xyz_first=bool(c), pool=pool)], [pts], layers,
                   took={"_GatherLinear": 1, "_SharedMLPChain": 1})
            mode(layers, False)
            with torch.no_grad():
                out = mlp.shared_mlp_grouped(layers, pts.detach() if c else None, idx, gxyz, xyz_first=bool(c), pool=pool)
            record("shared_mlp_grouped/eval/" + tag, [out], [], layers, took={"_GatherLinear": 1, "_SharedMLPChain": 0})


def interp_entries():
    rng = np.random.default_rng(51)
    b, n, m = 2, 16384, 1024                                                                 # 2 x 16384 = 32768 rows
    xyz1 = rng.random((b, n, 3), dtype=np.float32)
    xyz2 = np.stack([xyz1[i, rng.permutation(n)[:m]] for i in range(b)])
    idx, weight, inverse = PointnetFPModule.geometry(torch.from_numpy(xyz1).cuda(), torch.from_numpy(xyz2).cuda())
    assert inverse is not None
    for c2, c1, widths in ((32, 32, (64, 64)), (32, 0, (64, 64)), (256, 1, (128,))):
        layers = shared_layers(52 + c2 + c1, widths, c2 + c1)
        p2 = rand(b, m, c2, seed=53, grad=True)
        p1 = rand(b, n, c1, seed=54, grad=True) if c1 else None
        tag = "c2_%d/c1_%d" % (c2, c1)
        record("shared_mlp_interp/train/" + tag, [mlp.shared_mlp_interp(layers, p2, p1, idx, weight, inverse)], [p2, p1], layers,
               took={"_InterpLinear": 1, "_SharedMLPChain": 1})
        mode(layers, False)
        with torch.no_grad():
            out = mlp.shared_mlp_interp(layers, p2.detach(), p1.detach() if c1 else None, idx, weight, None)
        record("shared_mlp_interp/eval/" + tag, [out], [], layers, took={"_InterpLinear": 1, "_SharedMLPChain": 0})


# ------------------------------------------------------------------------------------------------ bf16
def bf16_entries():
    mlp.BF16_MIN_ROWS, mlp.BF16_MIN_COUT = 1, 4                                              # as tests/test_bf16_inference.py lowers them
    mlp.BF16_TRAIN_MIN_ROWS, mlp.BF16_TRAIN_MIN_COUT, mlp.BF16_TRAIN_MIN_CIN = 1, 4, 32      # as tests/test_bf16_training.py
    w, x = rand(256, 256, seed=61, grad=True), rand(SHORT, 256, seed=62, grad=True)
    before = mlp.BF16_TRAIN_ROUTED_CALLS[0]
    with mlp.training_precision("bf16"):
        record("linear_nobias/bf16_training", [mlp.linear_nobias(x, w, allow_bf16=True)], [x], [], [w], took={"_LinearBf16Train": 1})
    assert mlp.BF16_TRAIN_ROUTED_CALLS[0] == before + 1
    torch.manual_seed(63)
    bn = mlp.BatchNormReLU(256).cuda().eval()
    randomise(bn, 64)
    bias = rand(256, seed=65)
    before = mlp.BF16_ROUTED_CALLS[0]
    with torch.no_grad():
        record("linear_bf16_eval/gemm_alone", [mlp.linear_bf16_eval(x.detach(), w.detach(), bias, None, 0)])
        record("linear_bf16_eval/batchnorm_epilogue", [mlp.linear_bf16_eval(x.detach(), w.detach(), bias, bn, 1)], [], [bn])
        layers = shared_layers(66, (256, 64), 256)
        mode(layers, False)
        with mlp.inference_precision("bf16"):
            record("shared_mlp/eval/bf16/pool8", [mlp.shared_mlp(layers, x.detach(), pool_k=8)], [], layers)
            d = pointcnn.Dense(256, 64).cuda().eval()
            randomise(d.post.bn, 67)
            record("Dense/eval/bf16", [d(x.detach())], [], [d])
    assert mlp.BF16_ROUTED_CALLS[0] == before + 5


# ------------------------------------------------------------------------------------------------ the lifting chain and the backbone
def dense_chain_entries():
    def pair(seed, cin):
        torch.manual_seed(seed)
        d0, d1 = pointcnn.Dense(cin, 32).cuda().train(), pointcnn.Dense(32, 64).cuda().train()
        randomise(d0.post.bn, seed + 1)
        randomise(d1.post.bn, seed + 2)
        return d0, d1
    d0, d1 = pair(71, 3)
    x = rand(2, 2048, 8, 3, seed=72)                                                         # 32768 rows of local coordinates
    record("dense_chain/lift_chain/train", [pointcnn.dense_chain(d0, d1, x)], [], [d0, d1], took={"_LiftChain": 1})
    d0.eval(), d1.eval()
    with torch.no_grad():
        record("dense_chain/lift_chain/eval", [pointcnn.dense_chain(d0, d1, x)], [], [d0, d1], took={"_lift_chain_eval": 1})
    d0, d1 = pair(73, 6)
    x = rand(TALL, 6, seed=74, grad=True)
    record("dense_chain/dense_chain_elu/train", [pointcnn.dense_chain(d0, d1, x)], [x], [d0, d1], took={"_DenseChainElu": 1})
    d0, d1 = pair(75, 3)
    x = rand(SHORT, 3, seed=76, grad=True)
    record("dense_chain/layer_by_layer/train", [pointcnn.dense_chain(d0, d1, x)], [x], [d0, d1],
           took={"_BNReLUTrain": 2, "_DenseChainElu": 0, "_LiftChain": 0})


def backbone_entries():
    before = collections.Counter(CALLS)
    small = pointcnn.PointCnnConfig(xconv=((8, 1, -1, 32), (8, 1, 512, 32), (8, 1, 128, 64), (8, 1, 32, 128), (8, 1, 16, 128)),
                                    fc=((32, 0.5), (32, 0.5)))
    for tag, cfg in (("with_x", small), ("without_x", dataclasses.replace(small, with_x=False))):
        torch.manual_seed(81)
        net = pointcnn.PointCnnBackbone(cfg).cuda().train()
        xyz = torch.from_numpy(np.random.default_rng(82).random((2, 1024, 3), dtype=np.float32)).cuda()
        fts = rand(2, 1024, 1, seed=83, grad=True)
        record("PointCnnBackbone/train/" + tag, [net(xyz, fts)], [fts], [net])
    nodes = ("_BNConcatGroup", "_BNConcatSkip", "_BNDropoutTrain", "_DenseChainElu", "_LiftChain")
    RESULTS["_nodes"] = {k: CALLS[k] - before[k] for k in nodes if CALLS[k] != before[k]}
    assert RESULTS["_nodes"].get("_BNConcatGroup") and RESULTS["_nodes"].get("_BNConcatSkip") and RESULTS["_nodes"].get("_BNDropoutTrain")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--values", default=None, help="also save the hashed tensors of every entry to this file (torch.save)")
    args = ap.parse_args()
    count_routes()
    for fn in (batchnorm_entries, single_layer_entries, shared_mlp_entries, grouped_entries, interp_entries, dense_chain_entries,
               backbone_entries, bf16_entries):
        fn()
    if args.values:
        torch.save(VALUES, args.values)
    print(json.dumps(RESULTS))


if __name__ == "__main__":
    main()
