"""GPU tier (-m gpu): the context's content-checked cache of the pre-integration (csrc/api/preint.hpp run_preint,
csrc/preint.hip preint_match_kernel / preint_roll_kernel).

A context remembers, per (window, interval), the IMU inputs its stored pre-integration was computed from.  A later
call integrates only the intervals whose inputs differ bitwise; avm_slide_window* moves the stored intervals with the
window.  Whatever the cache does, every result must be what a call without it gives, to the bit: "cold" below is the
same call with AVM_PREINT_CACHE=0 on a second context (every interval integrated, the parent's path), and "equal" is
byte equality of delta, jacobian, covariance, sum_dt and sqrt_info.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

from helpers import abi, buffers, synth

pytestmark = pytest.mark.gpu

FIELDS = ("delta", "jacobian", "covariance", "sum_dt", "sqrt_info")
IMU_KEYS = ("imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg")
PRIOR_FIELDS = ("n", "nblk", "blk_kind", "blk_frame", "J", "r", "x0")


def _mod(name):
    import importlib

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


def _estimator(**opts):
    o = abi.default_options()
    for k, v in opts.items():
        setattr(o, k, v)
    return _mod("estimator").Estimator(ctx=_mod("lib").Context(0), options=o)


@pytest.fixture()
def E():
    e = _estimator()
    yield e
    e.ctx.close()


@pytest.fixture(scope="module")
def cold_E():
    e = _estimator()
    yield e
    e.ctx.close()


def _pre(E, w):
    """avm_imu_preintegrate_batch in the memory mode of `w`, and sqrt_info: five host arrays."""
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
    return dict(delta=d, jacobian=j, covariance=cv, sum_dt=sd, sqrt_info=E.sqrt_info(B))


def _cold(cold_E, w, options=None):
    """The same call with the cache switched off (every interval integrated), on the module's second context."""
    if options is not None:
        cold_E.options = options
    try:
        with _cache_off():
            out = _pre(cold_E, w.to_host())
            assert cold_E.ctx.preint_cache()["recomputed"] == 10 * w.n_windows
    finally:
        cold_E.options = abi.default_options()
    return out


def _assert_equal(got, want, what):
    for k in FIELDS:
        g, x = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.shape == x.shape, (what, k)
        assert np.array_equal(g.view(np.uint64), x.view(np.uint64)), (what, k)


def _ragged(B, max_samp=20, seed=0):
    """B windows whose intervals hold 0, 1, max_samp and other sample counts (the samples of make_windows, cut short)."""
    w = synth.make_windows(B, tracks="sparse", n_feat=12, max_feat=150, max_samp=max_samp)
    rng = np.random.default_rng(100 + seed)
    n = rng.integers(2, 20, (B, 10)).astype(np.int32)
    n[0, 0], n[0, 1], n[0, 2] = 0, 1, 20
    n[B - 1, 9], n[B - 1, 8] = 0, 20
    n[1, 4] = 13  # the interval test 2 works on: samples and padding on both sides of ns
    w.a["imu_n"][:] = n
    return w


def _next(x):
    return np.nextafter(x, np.inf)


# ---- 1. hit ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["host", "device"])
def test_a_repeated_call_recomputes_nothing_and_equals_cold(E, cold_E, mode):
    w = _ragged(3)
    wm = w.to_device("cuda:0") if mode == "device" else w
    first = _pre(E, wm)
    c1 = E.ctx.preint_cache()
    second = _pre(E, wm)
    c2 = E.ctx.preint_cache()
    print("first call %s, second call %s" % (c1, c2))
    assert c1["examined"] == 30 and c1["recomputed"] == 30
    assert c2["examined"] == 30 and c2["recomputed"] == 0
    cold = _cold(cold_E, w)
    _assert_equal(first, cold, "first")
    _assert_equal(second, cold, "second")
    # ... and a fresh context gives the same as the switched-off one
    F = _estimator()
    try:
        _assert_equal(_pre(F, wm), cold, "fresh context")
    finally:
        F.ctx.close()


# ---- 2. every input is in the key ------------------------------------------------------------------------------------
def _mutations():
    b, j, ns = 1, 4, 13

    def n_plus(a):
        a["imu_n"][b, j] = ns + 1

    def dt(a):
        a["imu_dt"][b, j, 5] = _next(a["imu_dt"][b, j, 5])

    def row(key, r, c):
        def f(a):
            a[key][b, j, r, c] = _next(a[key][b, j, r, c])

        return f

    def bias(key, c):
        def f(a):
            a[key][b, j, c] = _next(a[key][b, j, c])

        return f

    changed = [("imu_n", n_plus), ("dt", dt), ("acc row 0", row("imu_acc", 0, 1)), ("acc row ns", row("imu_acc", ns, 2)),
               ("gyr row 0", row("imu_gyr", 0, 0)), ("gyr row ns", row("imu_gyr", ns, 1)), ("lin_ba", bias("imu_lin_ba", 2)),
               ("lin_bg", bias("imu_lin_bg", 0))]

    def pad_dt(a):
        a["imu_dt"][b, j, ns] = _next(a["imu_dt"][b, j, ns])
        a["imu_dt"][b, j, 19] = 7.0

    def pad_rows(a):
        a["imu_acc"][b, j, ns + 1, 0] = _next(a["imu_acc"][b, j, ns + 1, 0])
        a["imu_gyr"][b, j, ns + 1, 2] = _next(a["imu_gyr"][b, j, ns + 1, 2])
        a["imu_acc"][b, j, 20] = np.nan

    padding = [("dt beyond ns", pad_dt), ("rows beyond ns", pad_rows)]
    return changed, padding


def test_every_input_is_in_the_key_and_padding_is_not(E, cold_E):
    base = _ragged(3)
    assert base.a["imu_n"][1, 4] == 13
    changed, padding = _mutations()
    for name, f in changed:
        # the key is base's again before every mutation, so that nothing but the mutated entry differs from it: a key that
        # left this entry out would report 0
        _pre(E, base)
        _pre(E, base)
        assert E.ctx.preint_cache()["recomputed"] == 0, name
        w = base.copy()
        f(w.a)
        got = _pre(E, w)
        c = E.ctx.preint_cache()
        print("%-12s recomputed %d of %d" % (name, c["recomputed"], c["examined"]))
        assert c["recomputed"] == 1, name
        _assert_equal(got, _cold(cold_E, w), name)
    for name, f in padding:
        _pre(E, base)
        _pre(E, base)
        assert E.ctx.preint_cache()["recomputed"] == 0, name
        w = base.copy()
        f(w.a)
        got = _pre(E, w)
        c = E.ctx.preint_cache()
        print("%-14s recomputed %d of %d" % (name, c["recomputed"], c["examined"]))
        assert c["recomputed"] == 0, name
        _assert_equal(got, _cold(cold_E, w), name)


# ---- 3. options and shapes -------------------------------------------------------------------------------------------
def test_changed_noise_window_count_or_max_samp_recompute_everything(E, cold_E):
    w3, w5 = _ragged(3, seed=1), _ragged(5, seed=2)
    _pre(E, w3)
    _pre(E, w3)
    assert E.ctx.preint_cache()["recomputed"] == 0
    for field in ("acc_n", "gyr_n", "acc_w", "gyr_w"):
        setattr(E.options, field, _next(getattr(E.options, field)))
        got = _pre(E, w3)
        assert E.ctx.preint_cache()["recomputed"] == 30, field
        o = abi.default_options()
        for f in ("acc_n", "gyr_n", "acc_w", "gyr_w"):
            setattr(o, f, getattr(E.options, f))
        _assert_equal(got, _cold(cold_E, w3, o), field)
    E.options = abi.default_options()
    for w in (w3, w5, w3):
        got = _pre(E, w)
        assert E.ctx.preint_cache()["recomputed"] == 10 * w.n_windows
        _assert_equal(got, _cold(cold_E, w), "n_windows %d" % w.n_windows)
    w24 = synth.make_windows(3, tracks="sparse", n_feat=12, max_feat=150, max_samp=24)
    w24.a["imu_n"][:] = w3.a["imu_n"]
    w24.a["imu_n"][2, 3] = 24
    w24.a["imu_dt"][2, 3, 20:] = 0.005
    w24.a["imu_acc"][2, 3, 21:] = w24.a["imu_acc"][2, 3, 17:21]
    w24.a["imu_gyr"][2, 3, 21:] = w24.a["imu_gyr"][2, 3, 17:21]
    got = _pre(E, w24)
    assert E.ctx.preint_cache()["recomputed"] == 30
    _assert_equal(got, _cold(cold_E, w24), "max_samp 24")
    _pre(E, w24)
    assert E.ctx.preint_cache()["recomputed"] == 0


# ---- 4. companions: a listed interval's result does not depend on which others share its wavefront --------------------
def test_dirty_sets_of_5_7_and_49_intervals_equal_cold(E, cold_E):
    base = _ragged(5, seed=3)
    rng = np.random.default_rng(7)
    seven = sorted(rng.choice(50, 7, replace=False).tolist())
    sets = {"j = 9 of every window": [w * 10 + 9 for w in range(5)], "seven drawn": seven, "all but one": [i for i in range(50) if i != 23]}
    assert [len(v) for v in sets.values()] == [5, 7, 49]
    for name, ivs in sets.items():
        _pre(E, base)
        w = base.copy()
        for iv in ivs:
            b, j = divmod(iv, 10)
            w.a["imu_gyr"][b, j, 0, 1] = _next(w.a["imu_gyr"][b, j, 0, 1])  # row 0 is in every key (also of an empty interval)
        got = _pre(E, w)
        c = E.ctx.preint_cache()
        print("%-22s recomputed %d" % (name, c["recomputed"]))
        assert c["recomputed"] == len(ivs), name
        _assert_equal(got, _cold(cold_E, w), name)


# ---- 5. NaN and signed zero ------------------------------------------------------------------------------------------
def test_a_nan_sample_hits_and_a_signed_zero_misses(E, cold_E):
    w = _ragged(2, seed=4)
    w.a["imu_n"][1, 4] = 13
    w.a["imu_acc"][1, 4, 3, 1] = np.nan
    w.a["imu_gyr"][0, 5, 1, 0] = 0.0
    _pre(E, w)
    got = _pre(E, w)
    assert E.ctx.preint_cache()["recomputed"] == 0
    _assert_equal(got, _cold(cold_E, w), "NaN")
    z = w.copy()
    z.a["imu_gyr"][0, 5, 1, 0] = -0.0
    got = _pre(E, z)
    assert E.ctx.preint_cache()["recomputed"] == 1
    _assert_equal(got, _cold(cold_E, z), "-0.0")


# ---- 6. the cache follows the window ---------------------------------------------------------------------------------
def _refill_newest(w, seed, n):
    """New samples in interval 9 of every window (what processIMU pushes between two images)."""
    rng = np.random.default_rng(seed)
    B = w.n_windows
    w.a["imu_n"][:, 9] = n
    w.a["imu_dt"][:, 9, :n] = 0.005
    w.a["imu_acc"][:, 9, 1:n + 1] = rng.normal(0, 1, (B, n, 3)) + np.array([0, 0, 9.8])
    w.a["imu_gyr"][:, 9, 1:n + 1] = rng.normal(0, 0.1, (B, n, 3))


def test_margin_old_slide_recomputes_only_the_newest_interval(E, cold_E):
    B = 3
    w = _ragged(B, seed=5)
    _pre(E, w)
    E.slideWindow(w, abi.MARGIN_OLD)
    assert E.ctx.preint_cache()["rolled_windows"] == B
    _refill_newest(w, 11, 17)
    got = _pre(E, w)
    c = E.ctx.preint_cache()
    print("MARGIN_OLD: recomputed %d of %d, roll %.4f ms" % (c["recomputed"], c["examined"], E.ctx.kernel_ms("preint_roll")))
    assert c["recomputed"] == B
    _assert_equal(got, _cold(cold_E, w), "MARGIN_OLD")
    # a second image
    E.slideWindow(w, abi.MARGIN_OLD)
    _refill_newest(w, 12, 20)
    got = _pre(E, w)
    assert E.ctx.preint_cache()["recomputed"] == B
    _assert_equal(got, _cold(cold_E, w), "MARGIN_OLD twice")


def test_margin_second_new_and_mixed_flags_equal_cold(E, cold_E):
    B = 4
    w = synth.make_windows(B, tracks="sparse", n_feat=12, max_feat=150, max_samp=40)
    assert (w.a["imu_n"] == 20).all()
    _pre(E, w)
    E.slideWindow(w, abi.MARGIN_SECOND_NEW)
    assert E.ctx.preint_cache()["rolled_windows"] == B
    assert (w.a["imu_n"][:, 8] == 40).all()
    _refill_newest(w, 13, 20)
    got = _pre(E, w)
    c = E.ctx.preint_cache()
    print("MARGIN_SECOND_NEW: recomputed %d of %d" % (c["recomputed"], c["examined"]))
    assert c["recomputed"] <= 2 * B
    _assert_equal(got, _cold(cold_E, w), "MARGIN_SECOND_NEW")
    # mixed flags
    w = synth.make_windows(B, tracks="sparse", n_feat=12, max_feat=150, max_samp=40)
    _pre(E, w)
    flags = np.array([abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW, abi.MARGIN_SECOND_NEW, abi.MARGIN_OLD], np.int32)
    E.slideWindow(w, flags)
    assert E.ctx.preint_cache()["rolled_windows"] == B
    _refill_newest(w, 14, 20)
    got = _pre(E, w)
    c = E.ctx.preint_cache()
    print("mixed flags: recomputed %d of %d" % (c["recomputed"], c["examined"]))
    assert c["recomputed"] <= 6  # one interval per MARGIN_OLD window, two per MARGIN_SECOND_NEW window
    _assert_equal(got, _cold(cold_E, w), "mixed flags")


def test_a_slide_of_another_batch_leaves_the_cache_to_the_comparison(E, cold_E):
    w3, w2 = _ragged(3, seed=6), _ragged(2, seed=7)
    _pre(E, w3)
    E.slideWindow(w2, abi.MARGIN_OLD)
    assert E.ctx.preint_cache()["rolled_windows"] == 0
    got = _pre(E, w3)
    assert E.ctx.preint_cache()["recomputed"] == 0
    _assert_equal(got, _cold(cold_E, w3), "other n_windows")
    # ... and a batch of the same shape that was never pre-integrated here: the roll moves keys that are not its own, the comparison decides
    other = _ragged(3, seed=8)
    E.slideWindow(other, abi.MARGIN_OLD)
    assert E.ctx.preint_cache()["rolled_windows"] == 3
    got = _pre(E, w3)
    _assert_equal(got, _cold(cold_E, w3), "same shape, other batch")
    got = _pre(E, other)
    _assert_equal(got, _cold(cold_E, other), "the slid batch")


# ---- 7. the whole call -----------------------------------------------------------------------------------------------
def test_window_solve_with_a_warm_cache_equals_the_call_without(E, cold_E):
    w = synth.make_windows(2, tracks="sparse", n_feat=20, max_feat=150)
    assert E.options.marginalization_flag == abi.MARGIN_OLD

    def solve(est, win):
        s = buffers.summary_to_numpy(est.optimization(win)).copy()  # the whole avm_solve_summary records
        p = {k: np.array(est.last_marginalization_info.a[k]) for k in PRIOR_FIELDS}
        return win, s, p, est.ctx.kernel_ms("preint")

    with _cache_off():
        ref = solve(cold_E, w.copy())
    runs = [solve(E, w.copy()), solve(E, w.copy())]  # (the states restored in between: the second call finds every interval unchanged)
    assert E.ctx.preint_cache()["recomputed"] == 0
    print("kernel_ms preint: without the cache %.4f, first call %.4f, warm %.4f" % (ref[3], runs[0][3], runs[1][3]))
    assert not np.array_equal(ref[0].a["pose"], w.a["pose"])
    for n, (win, s, p, ms) in enumerate(runs):
        for k in ("pose", "speedbias", "ex_pose", "inv_depth"):
            assert np.array_equal(win.a[k].view(np.uint64), ref[0].a[k].view(np.uint64)), (n, k)
        assert s.dtype == abi.SUMMARY_DTYPE and s.shape == (2,)
        for k in abi.SUMMARY_DTYPE.names:  # (field by field for the message, then every byte of the records)
            assert np.ascontiguousarray(s[k]).tobytes() == np.ascontiguousarray(ref[1][k]).tobytes(), (n, k)
        assert s.tobytes() == ref[1].tobytes(), n
        for k in PRIOR_FIELDS:
            assert p[k].tobytes() == ref[2][k].tobytes(), (n, k)
        assert ms > 0.0
    assert ref[3] > 0.0
