"""Generates tests/golden/preint_mp.npz: the independent numpy reading of IntegrationBase (gen_golden.preintegrate, written from the
reference sources) run in 50-digit arithmetic on sixteen intervals of the case sets of tests/preint_cases.py, followed by
sqrt_info = LLT(covariance^-1).matrixL()^T (imu_factor.h:64) in the same arithmetic.

The binary128 arbiter (oracle/avm_truth.cpp: avmt_imu_preintegrate) is oracle/'s reading of the same formulas with a wider scalar: it
removes rounding as an explanation for a difference, not a misreading that the FP64 oracle shares.  This fixture is the second reading.
Nothing of gen_golden.py is rewritten: its module-level `np` is replaced by gen_solve_trace_mp.NpProxy (object arrays of mpmath.mpf),
the FP64 inputs are converted exactly, and the noise variances are squared in mpmath.  tests/test_preint_truth.py compares the
arbiter's hi + lo pairs with the ones stored here.

Which intervals: sample counts 1, 2, 3, 5, 7 (= max_samp of its table), 13, 20 (= max_samp), 33 and 40 (= max_samp); intervals that turn
at 5 rad/s; three intervals under the non-default noise densities of set B.  The interval with one sample has a singular covariance
(rank 12: the p rows of V are 0.5 dt times its v rows) and no sqrt_info: NaN is stored there.

Run once (ten seconds):  python tests/golden/gen_preint_mp.py
"""
import os
import sys

import mpmath as mp
import numpy as real_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_solve_trace_mp import MPF, NpProxy, obj  # noqa: E402  (sets mp.dps = 50)

# (set, window, interval): the counts are asserted below
PICKS = [("A", 0, 0, 2), ("A", 0, 1, 5), ("A", 0, 2, 13), ("A", 0, 3, 20), ("A", 3, 0, 20), ("A", 9, 7, 20), ("A", 11, 2, 1), ("A", 11, 5, 7),
         ("B", 0, 0, 2), ("B", 1, 1, 20), ("B", 2, 2, 13),
         ("C7", 0, 2, 2), ("C7", 0, 3, 3), ("C7", 1, 7, 7),
         ("C40", 0, 0, 40), ("C40", 1, 2, 33)]
FIELDS = ("delta", "jacobian", "covariance", "sum_dt", "sqrt_info")


def split(vals):
    hi = real_np.array([float(v) for v in vals])
    lo = real_np.array([float(v - MPF(h)) if real_np.isfinite(h) else real_np.nan for v, h in zip(vals, hi)])
    return hi, lo


def main():
    import gen_golden as GG
    import preint_cases as PC

    assert mp.mp.dps == 50
    proxy = NpProxy()
    GG.np = proxy
    GG.float = lambda v: v  # (float(np.sum(dts)) would round to FP64)
    out = {k + s: [] for k in FIELDS for s in ("_hi", "_lo")}
    meta = dict(set=[], window=[], interval=[], ns=[], dt=[])
    cache = {}
    for name, b, j, want in PICKS:
        if name not in cache:
            cache[name] = PC.case(name)
        w, o = cache[name]
        a = w.a
        ns = int(a["imu_n"][b, j])
        assert ns == want, (name, b, j, ns)
        noise = tuple(MPF(float(getattr(o, k))) for k in ("acc_n", "gyr_n", "acc_w", "gyr_w"))  # FP64 densities; squared in 50 digits
        dp, dq, dv, J, P, sdt = GG.preintegrate(obj(a["imu_acc"][b, j, :ns + 1]), obj(a["imu_gyr"][b, j, :ns + 1]), obj(a["imu_dt"][b, j, :ns]),
                                                obj(a["imu_lin_ba"][b, j]), obj(a["imu_lin_bg"][b, j]), noise)
        if ns >= 2:
            U = proxy.linalg.cholesky(proxy.linalg.inv(P)).T
        else:
            U = real_np.full((15, 15), MPF("nan"), dtype=object)
        vals = dict(delta=list(dp) + [dq[1], dq[2], dq[3], dq[0]] + list(dv), jacobian=list(J.ravel()), covariance=list(P.ravel()),
                    sum_dt=[sdt], sqrt_info=list(U.ravel()))
        for k in FIELDS:
            hi, lo = split(vals[k])
            out[k + "_hi"].append(hi)
            out[k + "_lo"].append(lo)
        dt = real_np.full(40, real_np.nan)
        dt[:ns] = a["imu_dt"][b, j, :ns]
        for k, v in zip(("set", "window", "interval", "ns", "dt"), (name, b, j, ns, dt)):
            meta[k].append(v)
        print(f"{name} window {b} interval {j}: {ns} samples, fast turn {(b * 10 + j) % 5 == 0}, |sqrt_info| max {mp.nstr(max(abs(v) for v in vals['sqrt_info']) if ns >= 2 else MPF(0), 3)}", flush=True)
    res = {k: real_np.array(v) for k, v in out.items()}
    res.update(set=real_np.array(meta["set"]), window=real_np.array(meta["window"], real_np.int64), interval=real_np.array(meta["interval"], real_np.int64),
               ns=real_np.array(meta["ns"], real_np.int64), dt=real_np.array(meta["dt"]), dps=real_np.int64(mp.mp.dps))
    path = os.path.join(HERE, "preint_mp.npz")
    real_np.savez_compressed(path, **res)
    print("wrote preint_mp.npz with %d intervals, %d bytes" % (len(PICKS), os.path.getsize(path)))


if __name__ == "__main__":
    main()
