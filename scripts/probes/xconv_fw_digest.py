"""Diagnostic: sha256 of every output of every case of the X-Conv backward ABI suites (tests/test_xconv_bwd_diet_abi.py,
tests/test_xconv_bwd_fw_abi.py and the folded cases of tests/test_xconv_bn_abi.py, whose runner also returns dgamma / dbeta), one line
per (suite, case, entry, output).  HFOPS_LIBRARY selects the build; run it once per library and compare the two files:

  HFOPS_LIBRARY=<parent>/libhfops.so python scripts/probes/xconv_fw_digest.py > parent.txt
  python scripts/probes/xconv_fw_digest.py > new.txt
  python scripts/probes/xconv_fw_digest.py --compare parent.txt new.txt

--compare prints equal / cases per entry and output and lists what differs.  grad_wd of the entries without a workspace is summed by
global atomics and does not repeat its own bits: it is hashed like the rest and reported on a line of its own."""
import collections
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def digest(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()[:24]


def emit(suite, case, entry, outs):
    for name in sorted(outs):
        print("%s|%s|%s|%s|%s" % (suite, case, entry, name, digest(outs[name])), flush=True)


def main():
    import xconv_cases as xc
    import test_xconv_abi as xa
    import test_xconv_bn_abi as xb
    import test_xconv_bwd_diet_abi as bd
    import test_xconv_bwd_fw_abi as fw
    for suite, mod, folded_of in (("diet", bd, bd), ("fw", fw, bd)):
        for c in mod.CASES:
            t = xc.make_inputs(c)
            if not c["gather"]:
                emit(suite, xc.case_id(c), "dense", xa.run_bwd(c, t)[0])
                continue
            for ws in (True, False):
                emit(suite, xc.case_id(c), "gather_ws" if ws else "gather_nows", xa.run_bwd(c, t, ws=ws)[0])
        for c in mod.FOLDED:
            emit(suite, xc.case_id(c), "folded", folded_of.run_folded(c, folded_of.folded_inputs(c))[0])
    for c in xb.CASES:
        outs = xb.run_new(xb.Device(c, xb.make_inputs(c)))
        emit("bn", xb.case_id(c), "folded", {k: v for k, v in outs.items() if k != "out"})


def compare(a, b):
    rd = lambda p: dict(l.rsplit("|", 1) for l in open(p).read().split("\n") if l.count("|") == 4)
    da, db = rd(a), rd(b)
    assert da.keys() == db.keys(), "the two files hold different cases"
    eq, tot, diff = collections.Counter(), collections.Counter(), []
    for key in da:
        suite, case, entry, name = key.split("|")
        k = (entry, name)
        tot[k] += 1
        if da[key] == db[key]:
            eq[k] += 1
        else:
            diff.append(key)
    for k in sorted(tot):
        print("%-12s %-7s %4d / %4d" % (k[0], k[1], eq[k], tot[k]))
    for key in diff:
        print("differs:", key)


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--compare":
        compare(sys.argv[2], sys.argv[3])
    else:
        main()
