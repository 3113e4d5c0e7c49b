"""Every dense and BatchNorm entry of the C ABI is launched from one place in the package, and that place is _dense_kernels.py: the
autograd nodes and eval routes of mlp.py and pointcnn.py call its functions, never lib().hf_* themselves.  Reads the sources only."""
import ast
import glob
import os

from heterofusionrcnn_amd import _lib

PKG = os.path.dirname(os.path.abspath(_lib.__file__))
FAMILIES = ("hf_bn_", "hf_linear_", "hf_lift_", "hf_f32_to_bf16")
ENTRIES = sorted(n for n in _lib.EXPORTED_SYMBOLS if n.startswith(FAMILIES) or n == "hf_narrow_linear_dx")
# Entries without a caller in the package.  The first two forward to their _ld forms with ld = c (csrc/mlp.hip), which bn_fwd_train and
# bn_bwd call.  hf_lift_elu_fwd_eval (the inference chain without the BatchNorm epilogue) never had one: hf_lift_elu_fwd_eval_bn serves
# the package, and tests/test_gemm_abi.py pins both through the C ABI.
MAY_HAVE_NONE = {"hf_bn_relu_fwd_train", "hf_bn_relu_bwd", "hf_lift_elu_fwd_eval"}


def _call_sites():
    """entry -> [(file, line)] of every call `<anything>.hf_entry(...)` in heterofusionrcnn_amd/*.py"""
    sites = {name: [] for name in ENTRIES}
    for path in sorted(glob.glob(os.path.join(PKG, "*.py"))):
        with open(path) as f:
            tree = ast.parse(f.read(), path)
        for node in ast.walk(tree):
            if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr in sites:
                sites[node.func.attr].append((os.path.basename(path), node.lineno))
    return sites


def test_the_families_are_the_ones_the_abi_exports():
    assert len(ENTRIES) == 36 and MAY_HAVE_NONE <= set(ENTRIES)


def test_each_entry_is_called_from_one_place_in_the_launch_module():
    sites = _call_sites()
    for name in ENTRIES:
        assert len(sites[name]) <= 1, (name, sites[name])
        assert all(f == "_dense_kernels.py" for f, _ in sites[name]), (name, sites[name])
        assert sites[name] or name in MAY_HAVE_NONE, name
    assert sum(len(s) for s in sites.values()) <= 35


def test_the_nodes_and_routes_launch_nothing_of_these_families_themselves():
    sites = _call_sites()
    for name in ENTRIES:
        assert not [s for s in sites[name] if s[0] in ("mlp.py", "pointcnn.py")], (name, sites[name])
    # ... and no entry is fetched by name either (getattr(lib(), "hf_bn_...")): the string would be the only trace
    for module in ("mlp.py", "pointcnn.py"):
        with open(os.path.join(PKG, module)) as f:
            tree = ast.parse(f.read())
        strings = [n.value for n in ast.walk(tree) if isinstance(n, ast.Constant) and isinstance(n.value, str)]
        assert not [s for s in strings if s in ENTRIES], module


def test_the_generation_counter_is_one_object():
    """mlp re-exports the counter and its bump under their old names: BatchNormReLU.eval_invstd and the bf16 weight cache key on the list
    that the launch functions advance"""
    import heterofusionrcnn_amd._dense_kernels as k
    import heterofusionrcnn_amd.mlp as mlp
    assert mlp._STATS_GENERATION is k._STATS_GENERATION and mlp.running_stats_written is k.running_stats_written
    before = k._STATS_GENERATION[0]
    mlp.running_stats_written()
    assert k._STATS_GENERATION[0] == before + 1
