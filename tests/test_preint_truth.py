"""The pre-integration against the extended-precision arbiter (oracle/avm_truth.cpp: avmt_imu_preintegrate) and a 50-digit reading.

csrc/preint.hip runs in front of every solve, every marginalization and every stream step.  preint_kernel packs four intervals into
one wavefront, runs its scalar chain once per 16-lane group, holds the 15 x 15 state in the order theta | v | ba | bg | p with the
identity k-step folded into the accumulator and reads each group's dt back by readlane.  What the suite had for it: the FP64 oracle
(the same algorithm in the same order, for sqrt_info down to the LU inverse and the Cholesky columns), one golden interval, and windows
in which every sample of every interval has dt = 0.005 - compared through helpers.rel, one number per batch, which at 1e-12 holds the
bg block of a covariance whose entries span 1e-6 ... 1e-15 to about 1e-3.  A kernel that read group 0's dt for every group, or mixed
up anything else that equal inputs hide, passed.

Here (case sets and the distance measure: tests/preint_cases.py):
  * the truth is the oracle's pre-integration with binary128 as its scalar type, on the same FP64 tables, rounded once;
  * that arbiter is pinned to an independent reading - gen_golden.preintegrate in 50-digit arithmetic, tests/golden/preint_mp.npz - to
    1e-25, the repository's bound for arbiter <-> mpmath agreement: it removes misreading as what the two C++ builds could share;
  * distances are taken per interval: delta_p, delta_v, delta_q and sum_dt against their own norm, jacobian and covariance per 3 x 3
    block (a block that is exactly zero in the truth has to be exactly zero), sqrt_info per row against the row's largest entry (its
    (ba, bg) block is zero in exact arithmetic: a block measure has no scale there);
  * CPU tier: the FP64 oracle is within 1e-12 of the truth in every one of them (measured: ORACLE_TO_TRUTH);
  * GPU tier: the kernels are within ten times the oracle's own distance, per quantity, and within 1e-12; host and device mode give the
    same bits; an interval's five outputs do not depend on its position in the wavefront or on its three companions (to the bit); nor on
    what lies beyond its sample count (to the bit).

Intervals with 0 or 1 samples.  Without samples the outputs are the initial state (zero delta_p / delta_v, the identity quaternion
and jacobian, a zero covariance and sum_dt) and sqrt_info is NaN in every entry (csrc/preint.hip, sqrt_info_kernel).  With one sample
the p rows of V are exactly 0.5 dt times its v rows: the covariance has rank 12 and no inverse (cond 6e19 in FP64), so nothing defines
its sqrt_info - the other four outputs meet the bounds, sqrt_info is not compared.  Sets A - C hold 8 + 8 such intervals out of 160.
"""
import contextlib
import ctypes as C
import functools
import importlib
import os

import mpmath as mp
import numpy as np
import pytest

import preint_cases as PC
from helpers import abi

TOL = 1e-12  # the suite's tolerance for product <-> oracle, here per block and against the truth
# The FP64 oracle's worst distance to the binary128 arbiter over sets A, B, C7 and C40 (144 intervals with at least one sample),
# per quantity - for jacobian and covariance the worst 3 x 3 block, for sqrt_info the worst row.  Measured by
# test_fp64_oracle_is_within_tolerance_of_the_binary128_preintegration (x86-64, g++ -O3 -march=x86-64-v3 as oracle/Makefile builds it);
# three digits, rounded up; the per-block tables are in DESIGN.md 2.20.1.
ORACLE_TO_TRUTH = {
    "delta_p": 4.23e-16,     # set A
    "delta_q": 2.23e-16,     # A, C40
    "delta_v": 4.23e-16,     # A
    "sum_dt": 3.61e-16,      # C40 (forty additions)
    "jacobian": 8.89e-16,    # A, C40: the (theta, theta) block
    "covariance": 2.09e-15,  # C40: the (p, p) block
    "sqrt_info": 3.53e-15,   # C40: row 0
}
FIELDS = ("delta", "jacobian", "covariance", "sum_dt", "sqrt_info")
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preint_mp.npz"))
mp.mp.dps = 50


@functools.lru_cache(maxsize=None)
def _case(name):
    """(windows, options, the arbiter's hi, its lo) of a case set: computed once, read by every test, changed by none."""
    import oracle_py

    w, o = PC.case(name)
    hi, lo = oracle_py.truth_preintegrate(o, w)
    for d in (hi, lo):
        for v in d.values():
            v.setflags(write=False)
    return w, o, hi, lo


def _counts(w):
    return np.asarray(w.a["imu_n"]).reshape(-1)


def _assert_no_samples(got, hi, w, what):
    """An interval without samples: the initial state, exactly."""
    for i in np.where(_counts(w) == 0)[0]:
        b, j = divmod(int(i), 10)
        for k in ("delta", "jacobian", "covariance", "sum_dt"):
            assert np.array_equal(got[k][b, j], hi[k][b, j]), (what, i, k)
        assert np.array_equal(got["delta"][b, j], [0, 0, 0, 0, 0, 0, 1, 0, 0, 0]) and np.array_equal(got["jacobian"][b, j], np.eye(15))
        assert not got["covariance"][b, j].any() and got["sum_dt"][b, j] == 0.0


# ---- CPU tier -------------------------------------------------------------------------------------------------------------------------
def test_the_case_sets_hold_what_they_are_meant_to():
    import itertools

    n = _counts(_case("A")[0]).reshape(30, 4)
    assert [tuple(r) for r in n[:24]] == list(itertools.permutations((2, 5, 13, 20)))
    assert [tuple(r) for r in n[24:]] == [(0, 20, 20, 20), (20, 0, 20, 20), (20, 20, 0, 20), (20, 20, 20, 0), (1, 20, 1, 7), (20, 1, 7, 1)]
    assert sorted(set(_counts(_case("C7")[0]).tolist())) == list(range(8)) and set(_counts(_case("C40")[0]).tolist()) == {40, 33, 21, 2}
    assert [_case(k)[0].dims["max_samp"] for k in ("A", "B", "C7", "C40")] == [20, 20, 7, 40]
    for name in PC.SETS:
        w = _case(name)[0]
        a, S, cnt = w.a, w.dims["max_samp"], _counts(w)
        dt, gyr = a["imu_dt"].reshape(-1, S), a["imu_gyr"].reshape(-1, S + 1, 3)
        live = np.arange(S)[None, :] < cnt[:, None]
        assert (dt[~live] == PC.PAD).all() and dt[live].min() >= 0.7 / 400 and dt[live].max() <= 1.3 / 100
        for q in range(0, len(cnt), 4):  # no two intervals of a wavefront share a dt at any sample index
            for s in range(S):
                col = dt[q:q + 4, s][live[q:q + 4, s]]
                assert len(set(col.tolist())) == len(col)
        for k in ("imu_lin_ba", "imu_lin_bg"):
            assert a[k].all() and len(np.unique(a[k].reshape(-1, 3), axis=0)) == len(cnt)
        assert all(np.isclose(np.linalg.norm(gyr[i, :cnt[i] + 1], axis=1).max(), 5.0) for i in range(0, len(cnt), 5))
    # 0 or 1 samples: 8 + 8 of the 160 intervals of A, C7 and C40 (B is three windows of A again)
    assert [int((_counts(_case(k)[0]) <= 1).sum()) for k in ("A", "B", "C7", "C40")] == [8, 0, 8, 0]
    assert sum(len(_counts(_case(k)[0])) for k in ("A", "C7", "C40")) == 160
    o, d = _case("B")[1], abi.default_options()
    noise = [o.acc_n, o.gyr_n, o.acc_w, o.gyr_w]
    assert noise == [0.2, 0.05, 0.002, 4e-5] and all(x != y for x, y in zip(noise, [d.acc_n, d.gyr_n, d.acc_w, d.gyr_w]))
    for k in ("imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg"):
        assert np.array_equal(_case("B")[0].a[k], _case("A")[0].a[k][:3])


def test_the_arbiter_reads_nothing_but_the_imu_tables_and_any_output_may_be_left_out():
    """The golden interval of factors.npz in a window without features, every table but imu_* a null pointer, only three of the ten
    output pointers given: the arbiter against the FP64 numpy statement the fixture was written by."""
    import oracle_py
    from helpers import golden, imu_window_from_golden, rel

    g = golden()
    w = imu_window_from_golden(g)
    s = w.struct()
    for name, _ in s._fields_:
        if not name.startswith("imu_") and isinstance(getattr(s, name), (abi.c_dp, abi.c_ip)):
            setattr(s, name, None)
    assert not s.pose and not s.obs_xy and s.imu_dt
    J, P, P_lo = np.zeros((10, 15, 15)), np.zeros((10, 15, 15)), np.zeros((10, 15, 15))
    none = C.cast(None, abi.c_dp)
    rc = oracle_py.truth_lib().avmt_imu_preintegrate(C.byref(PC.options()), C.byref(s), 0, none, none, abi.dptr(J), none, abi.dptr(P), abi.dptr(P_lo),
                                                      none, none, none, none)
    assert rc == 0
    assert rel(J[0], g["pre_J"]) < 1e-14 and rel(P[0], g["pre_P"]) < 1e-14
    assert 0 < np.abs(P_lo[0]).max() <= 2.0 ** -53 * np.abs(P[0]).max()


@pytest.mark.parametrize("field", FIELDS)
def test_the_distance_measure_sees_a_nan_or_an_infinity(field):
    """The truth of set A with one interval of one output poisoned (an interval with 20 samples; for the jacobian a structurally zero
    entry as well): the measure reports an infinite distance, or the block in its list, never zero - max(0.0, nan) is 0.0."""
    w, _, hi, _ = _case("A")
    assert _counts(w)[3] == 20
    same, bad = PC.distances(hi, hi, w.a["imu_n"])
    assert not bad and set(same.values()) == {0.0}
    for poison in (np.nan, np.inf):
        got = {k: v.copy() for k, v in hi.items()}
        got[field].reshape(120, -1)[3, -1] = poison  # (interval 3: delta_v z, sum_dt, entry (14, 14) of a matrix)
        worst, bad = PC.distances(got, hi, w.a["imu_n"])
        q = PC.by_quantity(worst)
        hit = {"delta": "delta_v", "sum_dt": "sum_dt"}.get(field, field)
        assert not q[hit] < TOL and q[hit] == np.inf, (field, poison, q)
        assert [k for k, v in q.items() if v != 0.0] == [hit]
    got = {k: v.copy() for k, v in hi.items()}
    got["jacobian"][0, 3, 12, 0] = np.nan  # the (bg, p) block: zero in the truth
    assert PC.distances(got, hi, w.a["imu_n"])[1]
    got = {k: v.copy() for k, v in hi.items()}
    got["covariance"][:] = np.nan
    worst, _ = PC.distances(got, hi, w.a["imu_n"])
    assert all(v == np.inf for k, v in worst.items() if k.startswith("covariance") and k not in ("covariance[th,ba]", "covariance[ba,th]", "covariance[ba,bg]", "covariance[bg,ba]"))


def _mpv(hi, lo):
    hi, lo = np.asarray(hi, float), np.asarray(lo, float)
    out = np.empty(hi.shape, dtype=object)
    for idx in np.ndindex(hi.shape):
        out[idx] = mp.mpf(float(hi[idx])) + mp.mpf(float(lo[idx]))
    return out


def _mp_gap(a, t, norm):
    """|a - t| / |t| of two object arrays of mpf: Euclidean norms, or max norms."""
    a, t = a.ravel(), t.ravel()
    if norm == "l2":
        return mp.sqrt(sum(((x - y) ** 2 for x, y in zip(a, t)), mp.mpf(0))) / mp.sqrt(sum((y * y for y in t), mp.mpf(0)))
    return max(abs(x - y) for x, y in zip(a, t)) / max(abs(y) for y in t)


def test_binary128_arbiter_agrees_with_the_50_digit_reading_of_the_preintegration():
    """avmt_imu_preintegrate's hi + lo against tests/golden/preint_mp.npz (gen_golden.preintegrate and cholesky(inv(P)).T in 50 digits)
    on sixteen intervals of the sets - counts 1, 2, 3, 5, 7, 13, 20, 33, 40, fast turns, the noise of set B: every quantity in the
    measure of this file, to 1e-25."""
    worst = {}
    for e in range(len(GOLD["ns"])):
        name, b, j, ns = str(GOLD["set"][e]), int(GOLD["window"][e]), int(GOLD["interval"][e]), int(GOLD["ns"][e])
        w, o, hi, lo = _case(name)
        assert w.a["imu_n"][b, j] == ns and np.array_equal(w.a["imu_dt"][b, j, :ns], GOLD["dt"][e, :ns]), "the fixture is of other case sets: regenerate it"
        A = {k: _mpv(hi[k][b, j], lo[k][b, j]) for k in FIELDS}
        M = {k: _mpv(GOLD[k + "_hi"][e], GOLD[k + "_lo"][e]).reshape(A[k].shape) for k in FIELDS}
        gaps = {"delta_p": _mp_gap(A["delta"][0:3], M["delta"][0:3], "l2"), "delta_q": _mp_gap(A["delta"][3:7], M["delta"][3:7], "l2"),
                "delta_v": _mp_gap(A["delta"][7:10], M["delta"][7:10], "l2"), "sum_dt": _mp_gap(A["sum_dt"], M["sum_dt"], "max")}
        for q in ("jacobian", "covariance"):
            for bi in range(5):
                for ci in range(5):
                    x, t = A[q][3 * bi:3 * bi + 3, 3 * ci:3 * ci + 3], M[q][3 * bi:3 * bi + 3, 3 * ci:3 * ci + 3]
                    if all(v == 0 for v in t.ravel()):
                        assert all(v == 0 for v in x.ravel()), (e, q, bi, ci)
                    else:
                        gaps[q] = max(gaps.get(q, mp.mpf(0)), _mp_gap(x, t, "max"))
        if ns >= 2:
            gaps["sqrt_info"] = max(_mp_gap(A["sqrt_info"][r], M["sqrt_info"][r], "max") for r in range(15))
        else:
            assert np.isnan(GOLD["sqrt_info_hi"][e]).all()
        print("[mp pin] %-3s window %2d interval %d (%2d samples): " % (name, b, j, ns) + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in gaps.items()))
        for k, v in gaps.items():
            worst[k] = max(worst.get(k, mp.mpf(0)), v)
            assert v < mp.mpf("1e-25"), (e, k, v)
    print("[mp pin] worst: " + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in worst.items()))
    assert set(worst) == set(PC.QUANTITIES)


@pytest.mark.parametrize("name", list(PC.SETS))
def test_fp64_oracle_is_within_tolerance_of_the_binary128_preintegration(oracle, name):
    """The FP64 oracle against the arbiter on a case set: every quantity, every 3 x 3 block of jacobian and covariance and every row of
    sqrt_info within 1e-12 - and ORACLE_TO_TRUTH, which the GPU tier's bound is ten times of, still describes this oracle (within a
    factor of four: another compiler's choice of fused multiply-adds moves single roundings, not the size of the distance; beyond
    that the constants no longer belong to this oracle and are to be measured again)."""
    w, o, hi, _ = _case(name)
    got = PC.as_dict(*oracle.preintegrate(o, w))
    worst, bad = PC.distances(got, hi, w.a["imu_n"])
    print("\n" + PC.report("[preint truth] FP64 oracle -> binary128, set %s" % name, worst))
    q = PC.by_quantity(worst)
    print("[preint truth] set %s per quantity: %s" % (name, "  ".join("%s %.3e" % kv for kv in q.items())))
    assert not bad, bad
    for k, v in worst.items():
        assert v < TOL, (k, v)
    for k, v in q.items():
        assert v <= 4 * ORACLE_TO_TRUTH[k], "%s: %.3e, recorded %.3e - if the oracle or its compiler changed, measure ORACLE_TO_TRUTH again (printed above)" % (k, v, ORACLE_TO_TRUTH[k])
    _assert_no_samples(got, hi, w, name)


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------------
def _mod(name):
    return importlib.import_module("anticipated-vins-mono_amd." + name)


@contextlib.contextmanager
def _cache_off():
    old = os.environ.get("AVM_PREINT_CACHE")
    os.environ["AVM_PREINT_CACHE"] = "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["AVM_PREINT_CACHE"]
        else:
            os.environ["AVM_PREINT_CACHE"] = old


def _pre(E, w):
    """avm_imu_preintegrate_batch in the memory mode of `w`, and the sqrt_info it left: five host arrays."""
    B = w.n_windows
    if not w.on_device:
        d, j, cv, sd = E.preintegrate(w)
    else:
        import torch

        outs = [torch.zeros(s, dtype=torch.float64, device="cuda:0") for s in ((B, 10, 10), (B, 10, 15, 15), (B, 10, 15, 15), (B, 10))]
        s = w.struct()
        rc = E.ctx._L.avm_imu_preintegrate_batch(E.ctx.h, C.byref(E.options), w.mem, C.byref(s), *[abi.dptr(o) for o in outs])
        E.ctx.check(rc, "avm_imu_preintegrate_batch")
        d, j, cv, sd = [o.cpu().numpy() for o in outs]
    return PC.as_dict(d, j, cv, sd, E.sqrt_info(B))


def _assert_same_bits(got, want, what):
    for k in FIELDS:
        g, x = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == x.shape, (what, k)
        same = g.view(np.uint64) == x.view(np.uint64)
        assert same.all(), (what, k, "first difference at", tuple(int(v[0]) for v in np.nonzero(~same)))


@pytest.fixture()
def fresh():
    """Estimators on contexts of their own (the cache of the session's context is left alone), closed afterwards."""
    made = []

    def make(options):
        e = _mod("estimator").Estimator(ctx=_mod("lib").Context(0), options=options)
        made.append(e)
        return e

    yield make
    for e in made:
        e.ctx.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(PC.SETS))
def test_gpu_preintegration_is_as_close_to_the_binary128_one_as_the_fp64_oracle(fresh, name):
    """preint_kernel and sqrt_info_kernel against the arbiter on a case set: every distance within ten times the FP64 oracle's own (per
    quantity, the worst over all sets: ORACLE_TO_TRUTH) and within 1e-12 - the margin test_solve_truth.py gives the device over the
    oracle, for a different order of the sums (MFMA k-steps, the permuted state order), not for a different algorithm.  Host mode and
    device mode give the same bits."""
    w, o, hi, _ = _case(name)
    E = fresh(o)
    got = _pre(E, w)
    assert E.ctx.preint_cache()["recomputed"] == 10 * w.n_windows
    with _cache_off():  # (every interval integrated again, not handed out from the first call)
        dev = _pre(E, w.to_device("cuda:0"))
        assert E.ctx.preint_cache()["recomputed"] == 10 * w.n_windows
    worst, bad = PC.distances(got, hi, w.a["imu_n"])
    print("\n" + PC.report("[preint truth] GPU -> binary128, set %s" % name, worst))
    print("[preint truth] GPU set %s per quantity: %s" % (name, "  ".join("%s %.3e" % kv for kv in PC.by_quantity(worst).items())))
    _assert_same_bits(dev, got, "device mode against host mode")
    assert not bad, bad
    for k, v in worst.items():
        assert v <= 10 * ORACLE_TO_TRUTH[k.split("[")[0]] and v < TOL, (k, v, ORACLE_TO_TRUTH[k.split("[")[0]])
    _assert_no_samples(got, hi, w, name)
    for i in np.where(_counts(w) == 0)[0]:
        assert np.isnan(got["sqrt_info"][divmod(int(i), 10)]).all(), i


@pytest.mark.gpu
@pytest.mark.parametrize("cache", ["off", "default"])
def test_an_interval_does_not_depend_on_its_position_or_its_companions(fresh, cache):
    """Set A with its 120 intervals moved by i -> (7 i + 3) mod 120 - every interval in another 16-lane group with three other
    companions: all five outputs, moved back, are the unpermuted call's to the bit.  With the cache off every interval is item
    w * 10 + j of the launch; on a default context the second call integrates the intervals of the cache's list, in the order the
    wavefronts of the match kernel appended them."""
    w, o, _, _ = _case("A")
    perm = (7 * np.arange(120) + 3) % 120
    assert len(set(perm.tolist())) == 120 and ((perm % 4) != (np.arange(120) % 4)).all()
    for q in range(30):  # ... the four intervals of a wavefront go to four different ones
        assert len({int(perm[i]) // 4 for i in range(4 * q, 4 * q + 4)}) == 4
    wp = PC.permuted(w, perm)
    E = fresh(o)
    with _cache_off() if cache == "off" else contextlib.nullcontext():
        base = _pre(E, w)
        assert E.ctx.preint_cache()["recomputed"] == 120
        moved = _pre(E, wp)
        assert E.ctx.preint_cache()["recomputed"] == 120
    back = {k: v.reshape((120,) + v.shape[2:])[perm].reshape(v.shape) for k, v in moved.items()}
    _assert_same_bits(back, base, "permuted, cache %s" % cache)


@pytest.mark.gpu
def test_nothing_beyond_the_sample_count_reaches_the_result(fresh):
    """Set A with NaN in place of the sentinel in every entry of imu_dt / imu_acc / imu_gyr beyond an interval's sample count: the
    same bits (preint_kernel clamps the sample index of a group that has run out; what it loads there must not be used)."""
    w, o, _, _ = _case("A")
    E = fresh(o)
    with _cache_off():
        base = _pre(E, w)
        wn = PC.nan_padded(w)
        assert np.isnan(wn.a["imu_dt"]).sum() == (20 - _counts(w)).sum()
        got = _pre(E, wn)
    _assert_same_bits(got, base, "NaN beyond ns")
