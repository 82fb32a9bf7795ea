"""Test infrastructure: the case sets of tests/test_preint_truth.py and tests/golden/gen_preint_mp.py, and the distance measure
the pre-integration is graded with.

Why sets of their own: synth.make_windows and helpers.blank_windows write dt = 0.005 into every sample of every interval, and the
same sample count into every interval.  preint_kernel packs four intervals into a wavefront, runs its scalar chain once per 16-lane
group and reads each group's dt back by readlane: whatever it mixes up between the groups of a wavefront is hidden when the groups
hold the same numbers.  Here no two intervals share anything.

Set A "lanes"    12 windows = 120 intervals = 30 wavefronts of four, max_samp 20.  Wavefronts 0-23 hold the sample counts
                 (2, 5, 13, 20) in their 24 orders; 24-27 hold 20 with a count of 0 at each of the four group positions; 28 and 29
                 are (1, 20, 1, 7) and (20, 1, 7, 1).
Set B            set A's first three windows, for noise densities that are all distinct and none the default (OPTIONS_B).
Set C "strides"  two windows at max_samp 7 with the counts 0 ... 7 in turn, and two at max_samp 40 with counts from
                 {40, 33, 21, 2} (what a MARGIN_SECOND_NEW slide leaves: an interval merged from two).
Every interval has a base rate of its own from [1/400, 1/100] s, every sample's dt is jittered by +-30 %, the linearization biases
are non-zero and differ per interval, every fifth interval turns at up to 5 rad/s, and everything beyond an interval's sample
count is the sentinel PAD (large and finite: a read past ns shows in the result).
"""
import itertools

import numpy as np

from helpers import abi, buffers, synth

PAD = 7.0
QUANTITIES = ("delta_p", "delta_q", "delta_v", "sum_dt", "jacobian", "covariance", "sqrt_info")
BLOCKS = ("p", "th", "v", "ba", "bg")  # the reference's order of the 15 error-state rows (parameters.h:58-65)
OPTIONS_B = dict(acc_n=0.2, gyr_n=0.05, acc_w=0.002, gyr_w=4e-5)


def counts_a():
    c = [list(p) for p in itertools.permutations((2, 5, 13, 20))]
    for g in range(4):
        c.append([0 if k == g else 20 for k in range(4)])
    c += [[1, 20, 1, 7], [20, 1, 7, 1]]
    return np.array(c, np.int32).reshape(12, 10)


def _windows(n_windows, max_samp, counts, seed):
    """make_windows with one feature and no prior; the IMU tables rewritten from Philox(seed)."""
    B, S = n_windows, max_samp
    w = synth.make_windows(B, tracks="sparse", n_feat=1, with_prior=False, max_feat=150, max_samp=max(S, 20))
    if S < 20:  # (make_windows writes its own 20 samples first: tables of a smaller stride are cut from it)
        a = dict(w.a)
        a.update(imu_dt=np.zeros((B, 10, S)), imu_acc=np.zeros((B, 10, S + 1, 3)), imu_gyr=np.zeros((B, 10, S + 1, 3)))
        w = buffers.WindowArrays(dict(w.dims, max_samp=S), a)
    rng = np.random.Generator(np.random.Philox(key=seed))
    a = w.a
    counts = np.asarray(counts, np.int32).reshape(B, 10)
    assert counts.min() >= 0 and counts.max() <= S
    base = rng.uniform(1.0 / 400, 1.0 / 100, (B, 10, 1))
    a["imu_n"][:] = counts
    a["imu_dt"][:] = base * (1.0 + rng.uniform(-0.3, 0.3, (B, 10, S)))
    a["imu_acc"][:] = rng.normal(0, 0.5, (B, 10, S + 1, 3)) + np.array([0, 0, 9.8])
    a["imu_gyr"][:] = rng.normal(0, 0.2, (B, 10, S + 1, 3))
    a["imu_lin_ba"][:] = rng.normal(0, 0.02, (B, 10, 3))
    a["imu_lin_bg"][:] = rng.normal(0, 0.002, (B, 10, 3))
    for i in range(0, B * 10, 5):  # every fifth interval: the fastest of its samples turns at 5 rad/s
        b, j = divmod(i, 10)
        g = a["imu_gyr"][b, j, :counts[b, j] + 1]
        g *= 5.0 / np.linalg.norm(g, axis=1).max()
    for b in range(B):
        for j in range(10):
            n = counts[b, j]
            a["imu_dt"][b, j, n:] = PAD
            a["imu_acc"][b, j, n + 1:] = PAD
            a["imu_gyr"][b, j, n + 1:] = PAD
    # no two intervals of a wavefront share a dt at any sample index (nor a sample count's worth of anything else)
    dt = a["imu_dt"].reshape(B * 10, S)
    for q in range(0, B * 10, 4):
        grp = dt[q:q + 4]
        for s in range(S):
            live = [grp[k, s] for k in range(len(grp)) if s < counts.reshape(-1)[q + k]]
            assert len(set(live)) == len(live)
    return w


def set_a():
    return _windows(12, 20, counts_a(), 0x9E170A)


def set_b():
    """Set A's first three windows, to be run with options_b()."""
    return set_a().slice(0, 3).copy()


def set_c7():
    return _windows(2, 7, [[j % 8 for j in range(10)]] * 2, 0x9E170C)


def set_c40():
    pick = (40, 33, 21, 2)
    counts = [[pick[(3 * b + j + j // 4) % 4] for j in range(10)] for b in range(2)]
    return _windows(2, 40, counts, 0x9E170D)


def options(**noise):
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    for k, v in noise.items():
        setattr(o, k, v)
    return o


def options_b():
    return options(**OPTIONS_B)


SETS = {"A": (set_a, options), "B": (set_b, options_b), "C7": (set_c7, options), "C40": (set_c40, options)}


def case(name):
    make, opt = SETS[name]
    return make(), opt()


def as_dict(d, j, cv, sd, sq):
    return dict(delta=np.asarray(d), jacobian=np.asarray(j), covariance=np.asarray(cv), sum_dt=np.asarray(sd), sqrt_info=np.asarray(sq))


def permuted(w, perm):
    """A copy of `w` whose interval perm[i] (flat index window * 10 + j) holds what interval i of `w` holds."""
    out = w.copy()
    for k in ("imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg"):
        src = w.a[k]
        flat = src.reshape((src.shape[0] * 10,) + src.shape[2:])
        dst = np.empty_like(flat)
        dst[perm] = flat
        out.a[k][:] = dst.reshape(src.shape)
    return out


def nan_padded(w):
    out = w.copy()
    a = out.a
    for b in range(w.n_windows):
        for j in range(10):
            n = a["imu_n"][b, j]
            a["imu_dt"][b, j, n:] = np.nan
            a["imu_acc"][b, j, n + 1:] = np.nan
            a["imu_gyr"][b, j, n + 1:] = np.nan
    return out


# ---- the distance measure -----------------------------------------------------------------------------------------------------------
def worse(a, b):
    """The larger of two distances; one that is not finite (a NaN or an infinity in what was compared) counts as infinite and stays."""
    a, b = (float(v) if np.isfinite(v) else np.inf for v in (a, b))
    return max(a, b)


def _rel_norm(x, t):
    return float(np.linalg.norm(x - t) / np.linalg.norm(t))


def distances(got, truth, counts):
    """Worst distance of `got` to `truth` (dicts of delta, jacobian, covariance, sum_dt, sqrt_info as the ABI lays them out) over the
    intervals, per interval and then:
      delta_p, delta_q, delta_v, sum_dt   |x - t| / |t|, each against its own norm
      jacobian, covariance                per 3 x 3 block (a, b) of BLOCKS: max |x - t| / max |t| over the block; a block that is
                                          exactly zero in the truth must be exactly zero in `got`
      sqrt_info                           per row, against the row's largest entry; intervals with at least two samples only
    A distance that is not finite - a NaN or an infinity anywhere in a compared slice - is reported as infinite.
    Intervals without samples are left to the caller.  Returns ({quantity or "quantity[a,b]" or "sqrt_info[row]": worst},
    [messages about blocks that should be zero and are not])."""
    worst, bad = {}, []

    def put(key, v):
        worst[key] = worse(worst.get(key, 0.0), v)

    n = np.asarray(counts).reshape(-1)
    G = {k: np.asarray(v).reshape((len(n),) + np.asarray(v).shape[2:]) for k, v in got.items()}
    T = {k: np.asarray(v).reshape((len(n),) + np.asarray(v).shape[2:]) for k, v in truth.items()}
    for i in range(len(n)):
        if n[i] < 1:
            continue
        put("delta_p", _rel_norm(G["delta"][i, 0:3], T["delta"][i, 0:3]))
        put("delta_q", _rel_norm(G["delta"][i, 3:7], T["delta"][i, 3:7]))
        put("delta_v", _rel_norm(G["delta"][i, 7:10], T["delta"][i, 7:10]))
        put("sum_dt", abs(G["sum_dt"][i] - T["sum_dt"][i]) / abs(T["sum_dt"][i]))
        for q in ("jacobian", "covariance"):
            for bi, bn in enumerate(BLOCKS):
                for ci, cn in enumerate(BLOCKS):
                    x, t = G[q][i, 3 * bi:3 * bi + 3, 3 * ci:3 * ci + 3], T[q][i, 3 * bi:3 * bi + 3, 3 * ci:3 * ci + 3]
                    key = "%s[%s,%s]" % (q, bn, cn)
                    if not t.any():
                        if x.any() or not np.isfinite(x).all():
                            bad.append("interval %d (%d samples): %s is zero in the truth, not here" % (i, n[i], key))
                        put(key, 0.0)
                    else:
                        put(key, float(np.abs(x - t).max() / np.abs(t).max()))
        if n[i] >= 2:
            for r in range(15):
                x, t = G["sqrt_info"][i, r], T["sqrt_info"][i, r]
                put("sqrt_info[%d]" % r, float(np.abs(x - t).max() / np.abs(t).max()))
    return worst, bad


def by_quantity(worst):
    """The worst of distances() per quantity (over its blocks / rows)."""
    out = {}
    for k, v in worst.items():
        q = k.split("[")[0]
        out[q] = worse(out.get(q, 0.0), v)
    return out


def report(title, worst):
    lines = [title]
    for q in ("delta_p", "delta_q", "delta_v", "sum_dt"):
        lines.append("  %-10s %.2e" % (q, worst[q]))
    for q in ("jacobian", "covariance"):
        lines.append("  %s, rows x columns %s (0: equal in every interval, as every structurally zero block is)" % (q, " ".join(BLOCKS)))
        for bn in BLOCKS:
            cells = [worst["%s[%s,%s]" % (q, bn, cn)] for cn in BLOCKS]
            lines.append("    %-3s " % bn + " ".join("   0    " if c == 0.0 else "%.2e" % c for c in cells))
    rows = [worst.get("sqrt_info[%d]" % r) for r in range(15)]
    if rows[0] is not None:
        lines.append("  sqrt_info rows 0..14: " + " ".join("%.1e" % r for r in rows))
    return "\n".join(lines)
