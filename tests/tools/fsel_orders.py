"""A fresh process that asks the selector's launcher for its LDS sizes in the order a cached attribute would get wrong: the smallest setup
carve and kd-tree first, then the largest of both, the two-launch setup at both ends, then the smallest again (tests/test_fsel_launch.py).
usage: fsel_orders.py   - prints one line per step, exits 1 at the first mismatch with the FP64 oracle or HIP error"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]
PKG = "anticipated-vins-mono_amd"
synth, buffers, lib_m, fsel_m = (importlib.import_module(PKG + "." + m) for m in ("synth", "buffers", "lib", "feature_selector"))
import oracle_py  # noqa: E402

SMALL = dict(n_problems=1, horizon=2, n_cand=8, n_used=0, n_cloud=4, max_features=3)
STEPS = [  # (what it exercises, the frames, setup-only path too)
    ("smallest setup carve and kd-tree touch each kernel first", SMALL, False),
    ("largest setup carve (H = 13) and kd-tree (FS_MAX_CLOUD) after the smallest", dict(n_problems=1, horizon=13, n_cand=24, n_used=0, n_cloud=4096, max_features=6), True),
    ("two-launch setup (16 frames) at the largest H, one team per XCD", dict(n_problems=16, horizon=13, n_cand=20, n_used=2, n_cloud=12, max_features=4), False),
    ("two-launch setup at H = 2, two teams per XCD", dict(n_problems=16, horizon=2, n_cand=20, n_used=2, n_cloud=12, max_features=4), False),
    ("large, then small", SMALL, False),
]


def rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return float(np.abs(a - b).max() / max(1e-300, np.abs(b).max()))


def fail(step, what):
    print("step %d FAILED: %s" % (step, what), flush=True)
    raise SystemExit(1)


selector = fsel_m.FeatureSelector(ctx=lib_m.Context(0))
for step, (what, shape, info) in enumerate(STEPS, 1):
    pr = synth.make_fsel(**shape)
    P, mf = shape["n_problems"], shape["max_features"]
    oo = buffers.FselOutArrays.alloc(P, mf)
    oracle_py.fsel_select(pr, oo)
    try:
        if info:  # the setup-only path (run_rounds = false)
            om, dl, va = selector.information(pr)
            oom, odl, ova = oracle_py.fsel_information(pr)
            e_om, e_dl = rel(om, oom), rel(dl, odl)
            print("step %d information: Omega rel %.3g, Delta rel %.3g" % (step, e_om, e_dl), flush=True)
            if not (e_om < 1e-12 and np.array_equal(va, ova) and e_dl < 1e-10):
                fail(step, "information() against the oracle")
        out = selector.select_batch(pr).to_host()
    except lib_m.AvmError as e:
        fail(step, "HIP / library error: %s" % e)
    if not np.array_equal(out.a["n_selected"], oo.a["n_selected"]):
        fail(step, "n_selected %s, oracle %s" % (out.a["n_selected"].tolist(), oo.a["n_selected"].tolist()))
    if not np.array_equal(out.a["selected_ids"], oo.a["selected_ids"]):
        fail(step, "selected_ids differ from the oracle's")
    worst = 0.0
    for p in range(P):
        n = int(oo.a["n_selected"][p])
        if n == 0:
            fail(step, "frame %d is degenerate: the oracle selects nothing" % p)
        worst = max(worst, rel(out.a["fvalues"][p, :n], oo.a["fvalues"][p, :n]))
    print("step %d ok (%s): n_selected %s, fvalues rel %.3g" % (step, what, sorted(set(oo.a["n_selected"].tolist())), worst), flush=True)
    if not worst < 1e-9:
        fail(step, "fvalues rel %.3g" % worst)
print("all steps ok")
