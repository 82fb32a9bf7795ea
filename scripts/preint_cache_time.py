#!/usr/bin/env python3
"""What the context's pre-integration cache costs and saves in the regimes bench.py does not show.

    python scripts/preint_cache_time.py [--windows 4096] [--cache 0|1] [--regimes all_hit,all_miss,stream] [--label TEXT]

avm_imu_preintegrate_batch on device-resident windows with all four outputs NULL, so that only the table check and
run_preint run; synchronized wall time per call, median of --reps after --warmup calls, one JSON line:

  all_hit      the same batch repeated
  all_miss     two distinct batches alternating on one context (every interval differs from its key: compare, store the
               key, integrate)
  stream       MARGIN_OLD: slide, refill interval 9 with new samples, pre-integrate; the slide call (wall), the roll of
               the cache inside it (device time, kernel_ms "preint_roll") and the pre-integration (wall) separately

--cache 0 sets AVM_PREINT_CACHE=0: every interval on every call, the path before the cache.  The script also runs on a
checkout without the cache (no counters, no roll time): that and --cache 0 are the yardsticks.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cache", type=int, default=1, choices=[0, 1])
    ap.add_argument("--label", default="")
    ap.add_argument("--regimes", default="all_hit,all_miss,stream", help="comma-separated subset (a run under a profiler takes one)")
    args = ap.parse_args()
    if not args.cache:
        os.environ["AVM_PREINT_CACHE"] = "0"
    import torch

    synth, est_m, abi = (importlib.import_module(PKG + "." + m) for m in ("synth", "estimator", "abi"))
    E = est_m.Estimator(options=abi.default_options())
    ctx, L = E.ctx, E.ctx._L
    has_counters = hasattr(ctx, "preint_cache")
    W = args.windows
    base = [synth.make_windows(32, first_id=k * 32, tracks="sparse", n_feat=20, max_feat=150) for k in range(2)]
    a, b = (synth.tile_windows(x, W).to_device("cuda:0") for x in base)

    def pre(w):
        s = w.struct()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rc = L.avm_imu_preintegrate_batch(ctx.h, C.byref(E.options), w.mem, C.byref(s), None, None, None, None)
        t1 = time.perf_counter()
        ctx.check(rc, "avm_imu_preintegrate_batch")
        return (t1 - t0) * 1e3

    def stats(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def recomputed():
        return ctx.preint_cache()["recomputed"] if has_counters else None

    out = {"windows": W, "reps": args.reps, "warmup": args.warmup, "cache": bool(args.cache) and has_counters, "label": args.label,
           "timing": "synchronized wall time of avm_imu_preintegrate_batch (table check + run_preint), outputs NULL"}
    regimes = args.regimes.split(",")
    if "all_hit" in regimes:
        t = [pre(a) for _ in range(args.warmup + args.reps)][args.warmup:]
        out["all_hit"] = dict(stats(t), recomputed=recomputed())
    if "all_miss" in regimes:
        t = [pre(a if k % 2 else b) for k in range(args.warmup + args.reps)][args.warmup:]
        out["all_miss"] = dict(stats(t), recomputed=recomputed())
    if "stream" not in regimes:
        print(json.dumps(out))
        return
    g = torch.Generator(device="cuda:0")
    g.manual_seed(1)
    pre(a)
    slide, roll, integ, rec = [], [], [], []
    for k in range(args.warmup + args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        E.slideWindow(a, abi.MARGIN_OLD)
        slide.append((time.perf_counter() - t0) * 1e3)
        try:
            roll.append(ctx.kernel_ms("preint_roll"))
        except Exception:
            roll.append(0.0)
        a.a["imu_n"][:, 9] = 20
        a.a["imu_dt"][:, 9, :20] = 0.005
        a.a["imu_acc"][:, 9, 1:21] = torch.randn((W, 20, 3), generator=g, device="cuda:0", dtype=torch.float64) + torch.tensor([0.0, 0.0, 9.8], device="cuda:0", dtype=torch.float64)
        a.a["imu_gyr"][:, 9, 1:21] = 0.1 * torch.randn((W, 20, 3), generator=g, device="cuda:0", dtype=torch.float64)
        integ.append(pre(a))
        rec.append(recomputed())
    n = args.warmup
    out["stream_margin_old"] = {"slide_call": stats(slide[n:]), "roll_kernel": stats(roll[n:]), "preintegrate": stats(integ[n:]), "recomputed": rec[-1],
                                "roll_plus_preintegrate_median_ms": round(statistics.median(r + p for r, p in zip(roll[n:], integ[n:])), 4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
