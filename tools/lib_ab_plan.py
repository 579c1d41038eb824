"""Do two builds of the library PLAN their passes alike?  Runs the case table of tests/pass_plan_cases.py (every launch path of
csrc/pnn_passes.cpp, autotune off) in one subprocess per library under PNN_DEBUG=1 and compares, case by case, the output bits, the
[pnn] lines (which kernel ran which layer) and last_call_stats(): python tools/lib_ab_plan.py <libA.so> <libB.so>
(used when the pass layer is reshaped without a change of behaviour: any difference is a defect of the reshaping)"""
import os, subprocess, sys, tempfile
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, %r)
from tests import pass_plan_cases as C
out = {}
for case in C.CASES:
    sys.stderr.write("== %%s\n" %% case[0]); sys.stderr.flush()
    out[case[0]], out["stats " + case[0]] = C.run_case(case)
np.savez(sys.argv[1], **out)
''' % ROOT
res, plans = [], []
with tempfile.TemporaryDirectory() as d:
    for i, lib in enumerate(sys.argv[1:3]):
        f = os.path.join(d, "o%d.npz" % i)
        r = subprocess.run([sys.executable, "-c", CHILD, f], env=dict(os.environ, PNN_LIB_PATH=os.path.abspath(lib), PNN_DEBUG="1"),
                           stderr=subprocess.PIPE, universal_newlines=True)
        if r.returncode:
            sys.exit("%s: the cases failed\n%s" % (lib, r.stderr[-4000:]))
        res.append(dict(np.load(f)))
        plan, name = {}, None
        for line in r.stderr.splitlines():
            if line.startswith("== "): name = line[3:]; plan[name] = []
            elif line.startswith("[pnn]") and name: plan[name].append(line)
        plans.append(plan)
bad = 0
for k in sorted(k for k in res[0] if not k.startswith("stats ")):
    bits = np.array_equal(res[0][k].view(np.uint32), res[1][k].view(np.uint32))
    lines = plans[0][k] == plans[1][k]
    stats = res[0]["stats " + k].tolist() == res[1]["stats " + k].tolist()
    print("%-22s %s, %3d [pnn] lines %s, stats (%d, %d, %.17g) %s" % (
        k,"same bits" if bits else "DIFFERENT BITS", len(plans[0][k]), "same" if lines else "DIFFERENT", *res[0]["stats " + k], "same" if stats else "DIFFERENT"))
    if not lines:
        for a, b in zip(plans[0][k] + [""] * len(plans[1][k]), plans[1][k] + [""] * len(plans[0][k])):
            if a != b: print("    A: %s\n    B: %s" % (a, b))
    if not stats: print("    B: %s" % res[1]["stats " + k].tolist())
    bad += not (bits and lines and stats)
print("all equal" if not bad else "%d of %d cases differ" % (bad, len(plans[0])))
sys.exit(1 if bad else 0)
