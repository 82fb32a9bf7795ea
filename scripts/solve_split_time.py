#!/usr/bin/env python3
"""What a batch pays when SOME of its streams have a relocalization pending.

    python scripts/solve_split_time.py [--windows 4096] [--active 0,1,16,256,4096] [--calls 5] [--out profiles/solve_split.md]

Workload: --windows device-resident dense windows tiled from 32 (150 features, MARGIN_OLD: 2.22's workload) with relocalization data on
every window; k of them, spread evenly over the batch, are active.  For every k the median over the last calls - 1 of --calls calls of
avm_last_kernel_ms("window_solve") and of the synchronized wall time of the whole call, for

  (a)  the batch without the relocalization arrays                    avm_window_solve_batch_flags
  (b)  the batch with the arrays (every window: the extended kernel)  avm_window_solve_batch_flags
  (c)  the split call, relo_active marking the k windows              avm_window_solve_batch_relo
  (x)  the extended kernel alone on a batch of the k active windows: what k active windows must cost

Every call solves a fresh clone of the same tables.  Prints one JSON line; --out also writes the table as markdown.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PKG = "anticipated-vins-mono_amd"
RELO = ("relo_n", "relo_frame", "relo_feat", "relo_xy", "relo_pose")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--active", default="0,1,16,256,4096")
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch

    synth, est_m, abi, buffers = (importlib.import_module(PKG + "." + m) for m in ("synth", "estimator", "abi", "buffers"))
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_OLD
    E = est_m.Estimator(options=o)
    ctx, L = E.ctx, E.ctx._L
    W = args.windows
    master = synth.tile_windows(synth.make_windows(32, tracks="dense", n_feat=150, max_feat=150, relo=True), W).to_device("cuda:0")
    prior, summ = buffers.PriorOutArrays.alloc(W, 96, 16, "cuda:0"), buffers.summary_alloc(W, "cuda:0")

    def call(w, active=None, split=False):
        s, po = w.struct(), prior.struct()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if split:
            rc = L.avm_window_solve_batch_relo(ctx.h, C.byref(o), w.mem, C.byref(s), None, abi.iptr(active), C.byref(po), buffers.summary_ptr(summ))
        else:
            rc = L.avm_window_solve_batch_flags(ctx.h, C.byref(o), w.mem, C.byref(s), None, C.byref(po), buffers.summary_ptr(summ))
        t1 = time.perf_counter()
        ctx.check(rc, "the solve")
        return ctx.kernel_ms("window_solve"), (t1 - t0) * 1e3

    def measure(make, **kw):
        t = [call(make(), **kw) for _ in range(args.calls)][1:]
        ks, ws = [x[0] for x in t], [x[1] for x in t]
        return {"solve_ms": round(statistics.median(ks), 3), "solve_min": round(min(ks), 3), "solve_max": round(max(ks), 3),
                "call_ms": round(statistics.median(ws), 3), "forms": [ctx.last_solve_form(), ctx.last_marg_form()], "split": list(ctx.last_split())}

    def without(w):
        return buffers.WindowArrays(w.dims, {k: v for k, v in w.a.items() if k not in RELO})

    rows = []
    for k in [int(x) for x in args.active.split(",")]:
        idx = np.unique(np.linspace(0, W - 1, k).round().astype(np.int64)) if k else np.zeros(0, np.int64)
        assert len(idx) == k
        act = torch.zeros(W, dtype=torch.int32, device="cuda:0")
        act[torch.from_numpy(idx).to("cuda:0")] = 1
        row = {"k": k, "a": measure(lambda: without(master.copy())), "b": measure(master.copy), "c": measure(master.copy, active=act, split=True)}
        if k:
            sel = torch.from_numpy(idx).to("cuda:0")
            d = dict(master.dims)
            d["n_windows"] = k
            row["x"] = measure(lambda: buffers.WindowArrays(d, {kk: v[sel].contiguous() for kk, v in master.a.items()}))
        rows.append(row)
    out = {"windows": W, "calls": args.calls, "rows": rows}
    print(json.dumps(out))
    if args.out:
        with open(args.out, "w") as f:
            f.write("%d device-resident dense windows (150 features, MARGIN_OLD), k of them with a relocalization pending; median of the last %d of %d calls,\n"
                    "ms (`window_solve`: min - max in brackets; call: synchronized wall time of the whole call).  (x): the extended kernel alone on k windows.\n\n"
                    % (W, args.calls - 1, args.calls))
            f.write("| k | (a) no arrays: `window_solve` | call | (b) arrays, one call: `window_solve` | call | (c) split: `window_solve` | call | (c) - (a) | (x) `window_solve` | (c) split |\n")
            f.write("|---|---|---|---|---|---|---|---|---|---|\n")
            cell = lambda r: "%.2f [%.2f - %.2f]" % (r["solve_ms"], r["solve_min"], r["solve_max"])
            for r in rows:
                f.write("| %d | %s | %.2f | %s | %.2f | %s | %.2f | %.2f | %s | %s |\n" % (
                    r["k"], cell(r["a"]), r["a"]["call_ms"], cell(r["b"]), r["b"]["call_ms"], cell(r["c"]), r["c"]["call_ms"],
                    r["c"]["solve_ms"] - r["a"]["solve_ms"], cell(r["x"]) if "x" in r else "-", r["c"]["split"]))


if __name__ == "__main__":
    main()
