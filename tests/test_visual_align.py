"""Estimator::visualInitialAlign on the device (avm_visual_initial_align_batch) against tests/golden/visual_align.npz: the
independent numpy statement of gen_visual_align.py and its 50-digit run.

Measured on an MI355X, over the fixture's cases: the largest relative distance of the device result from the 50-digit result | the
err_fp64 of that case (the FP64 numpy run's own distance):
  delta_bg 1.2e-13 | 8.7e-14   deltas 4.3e-16 | 3.7e-16   x 2.7e-13 | 1.2e-13   s 2.4e-13 | 1.1e-13   g_c0 7.4e-13 | 3.5e-13
  g_world 1.3e-15 | 3.6e-16    pos 5.3e-13 | 2.6e-13      quat 3.2e-13 | 1.4e-13 vel 6.5e-13 | 3.1e-13 inv_depth 2.4e-13 | 1.1e-13
No quantity of any case is further than 7 x its own err_fp64, and none uses more than 1 / 26 of the 100 x bound.
"""
import ctypes as C
import importlib
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_visual_align as GEN  # noqa: E402

PKG = "anticipated-vins-mono_amd"
abi = importlib.import_module(PKG + ".abi")
buffers = importlib.import_module(PKG + ".buffers")
synth = importlib.import_module(PKG + ".synth")

pytestmark = pytest.mark.gpu
NAMES = [c[0] for c in GEN.CASES]
WITH_WINDOWS = [i for i, c in enumerate(GEN.CASES) if c[3] is not None]
ALIGN_IN = ("n_frames", "frame_R", "frame_T", "tic", "imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "golden", "visual_align.npz"))


@pytest.fixture(scope="module")
def cases(gold):
    """[(AlignArrays, WindowArrays or None, g)] of the fixture's cases, regenerated and checked against the stored inputs."""
    out = []
    for ci, case in enumerate(GEN.CASES):
        inp, g_opt, al, win = GEN.case_inputs(case)
        for k, v in inp.items():
            np.testing.assert_array_equal(np.asarray(v), gold["c%d_in_%s" % (ci, k)], err_msg="%s %s" % (case[0], k))
        out.append((al, win, g_opt))
    return out


def estimator_for(ctx, g):
    opt = abi.default_options()
    opt.marginalization_flag = abi.MARGIN_NONE
    opt.g[0], opt.g[1], opt.g[2] = [float(v) for v in g]
    return importlib.import_module(PKG + ".estimator").Estimator(ctx=ctx, options=opt)


def run(ctx, al, win, g, device=False):
    """One call on copies; returns (outputs as host numpy dict, windows as host WindowArrays or None)."""
    al, win = al.copy(), (win.copy() if win is not None else None)
    if device:
        al, win = al.to_device(), (win.to_device() if win is not None else None)
    out = estimator_for(ctx, g).visualInitialAlign(al, win)
    return out.to_host().a, (win.to_host() if win is not None else None)


def pad_to(v, shape):
    out = np.zeros((v.shape[0],) + tuple(shape), v.dtype)
    out[tuple(slice(0, n) for n in v.shape)] = v
    return out


def stack(arrays_list, cls, dims_of):
    """Windows with different strides as one batch: every table zero-padded to the largest stride."""
    keys = arrays_list[0].a.keys()
    a = {}
    for k in keys:
        shape = np.max([v.a[k].shape[1:] for v in arrays_list], axis=0) if arrays_list[0].a[k].ndim > 1 else ()
        a[k] = np.concatenate([pad_to(v.a[k], shape) for v in arrays_list])
    return cls(dims_of(a), a)


def stack_align(als):
    # (frame_R of the padding frames stays zero: no kernel reads beyond n_frames)
    als = [buffers.AlignArrays(a.dims, dict(a.a, frame_R=a.a["frame_R"].reshape(a.n_windows, -1, 9))) for a in als]
    mf = max(a.dims["max_frames"] for a in als)
    ms = max(a.dims["max_samp"] for a in als)
    out = stack(als, buffers.AlignArrays, lambda a: dict(n_windows=a["n_frames"].shape[0], max_frames=mf, max_samp=ms))
    assert out.a["imu_acc"].shape[1:] == (mf - 1, ms + 1, 3) and out.a["frame_R"].shape[1:] == (mf, 9)
    return out


def stack_windows(wins):
    d0 = wins[0].dims
    ms = max(w.dims["max_samp"] for w in wins)
    return stack(wins, buffers.WindowArrays, lambda a: dict(d0, n_windows=a["n_feat"].shape[0], max_samp=ms))


def distance(q, got, want):
    """max |a - b| / max |b|, as gen_visual_align.py measures err_fp64 (a quaternion and its negative are one rotation)."""
    got, want = np.asarray(got, float), np.asarray(want, float)
    big = np.abs(want).max()
    if q == "quat":
        return float(np.minimum(np.abs(got - want).max(axis=1), np.abs(got + want).max(axis=1)).max() / big)
    return float(np.abs(got - want).max() / big)


def quantities(ci, out, win, F):
    """The output quantities of one case by the fixture's names."""
    r = {"delta_bg": out["delta_bg"][0], "deltas": out["deltas"][0, : F - 1], "x": out["x"][0, : 3 * F], "s": out["x"][0, -1:],
         "g_c0": out["g_c0"][0]}
    if win is not None:
        r.update(g_world=out["g_world"][0], pos=win.a["pose"][0, :, :3], quat=win.a["pose"][0, :, 3:], vel=win.a["speedbias"][0, :, :3],
                 inv_depth=win.a["inv_depth"][0, : int(win.a["n_feat"][0])])
    return r


def bound(gold, q, F):
    """100 x the FP64 numpy run's own distance from the 50-digit run, the maximum over the fixture's cases with F frames."""
    errs = [float(gold["c%d_err_fp64_%s" % (ci, q)]) for ci, c in enumerate(GEN.CASES) if c[2] == F and "c%d_err_fp64_%s" % (ci, q) in gold.files]
    return 100.0 * max(errs)


def test_ok_flags(ctx, gold, cases):
    for ci, (al, win, g) in enumerate(cases):
        out, _ = run(ctx, al, win, g)
        assert int(out["ok"][0]) == int(gold["c%d_ok" % ci]), NAMES[ci]


@pytest.mark.parametrize("ci", [i for i, c in enumerate(GEN.CASES) if c[6] is None and c[2] >= 4], ids=lambda i: NAMES[i])
def test_parity_with_50_digits(ctx, gold, cases, ci):
    al, win, g = cases[ci]
    F = GEN.CASES[ci][2]
    out, w = run(ctx, al, win, g)
    assert int(out["ok"][0]) == 1
    got = quantities(ci, out, w, F)
    report, bad = [], []
    for q, v in got.items():
        d, e = distance(q, v, gold["c%d_m_%s" % (ci, q)]), float(gold["c%d_err_fp64_%s" % (ci, q)])
        b = bound(gold, q, F)
        report.append("%s %.1e (fp64 %.1e, bound %.1e)" % (q, d, e, b))
        if not (d <= b and d <= 1e-6):
            bad.append(q)
    print(NAMES[ci], "; ".join(report))
    assert not bad, (bad, report)
    # the gyro biases of all eleven frames carry the increment (initial_aligment.cpp:29-30)
    if w is not None:
        np.testing.assert_array_equal(w.a["speedbias"][0, :, 6:9], win.a["speedbias"][0, :, 6:9] + out["delta_bg"][0])


def test_velocity_index_quirk(ctx, gold, cases):
    """Vs[kv] = R_key(kv) x.segment<3>(kv * 3): with non-key frames in between the literal velocities are far from the 'corrected' ones."""
    ci = NAMES.index("f33_stride2")
    al, win, g = cases[ci]
    out, w = run(ctx, al, win, g)
    b = bound(gold, "vel", 33)
    vel = w.a["speedbias"][0, :, :3]
    assert distance("vel", vel, gold["c%d_m_vel" % ci]) <= b
    assert distance("vel", vel, gold["c%d_m_vel_fixed" % ci]) > 100 * b
    assert distance("vel", gold["c%d_m_vel" % ci], gold["c%d_m_vel_fixed" % ci]) > 100 * b


def differ(a, b):
    """The keys at which two dicts of arrays are not bit-identical (empty: the same)."""
    return [k for k in a if not np.array_equal(a[k], b[k], equal_nan=True)]


def test_determinism(ctx, cases):
    """70 windows tiled from the cases with key frames: each bit-identical to the same window alone, to a second run, and in both memory modes."""
    base_ci = [ci for ci in WITH_WINDOWS if GEN.CASES[ci][6] != "g12"]  # (one value of opt->g per call)
    base = [cases[ci] for ci in base_ci]
    al1, win1 = stack_align([c[0] for c in base]), stack_windows([c[1] for c in base])
    n = len(base)
    idx = [i % n for i in range(70)]
    al = buffers.AlignArrays(dict(al1.dims, n_windows=70), {k: v[idx] for k, v in al1.a.items()})
    win = buffers.WindowArrays(dict(win1.dims, n_windows=70), {k: v[idx] for k, v in win1.a.items()})
    out, w = run(ctx, al, win, GEN.G_DEFAULT)
    out2, w2 = run(ctx, al, win, GEN.G_DEFAULT)
    assert not differ(out, out2) and not differ(w.a, w2.a)
    outd, wd = run(ctx, al, win, GEN.G_DEFAULT, device=True)
    assert not differ(out, outd) and not differ(w.a, wd.a)
    assert out["ok"].tolist() == [int(GEN.CASES[base_ci[i]][6] is None) for i in idx]
    for i in range(n):
        o1, w1 = run(ctx, al.slice(i, i + 1), win.slice(i, i + 1), GEN.G_DEFAULT)
        for j in range(i, 70, n):
            assert all(np.array_equal(o1[k][0], out[k][j], equal_nan=True) for k in o1), (i, j)
            assert all(np.array_equal(w1.a[k][0], w.a[k][j], equal_nan=True) for k in w1.a), (i, j)
    # alignment only, every case but the one with another G
    ab = [cases[ci][0] for ci in range(len(cases)) if GEN.CASES[ci][6] != "g12"]
    a1 = stack_align(ab)
    idx = [i % len(ab) for i in range(70)]
    a70 = buffers.AlignArrays(dict(a1.dims, n_windows=70), {k: v[idx] for k, v in a1.a.items()})
    o70, _ = run(ctx, a70, None, GEN.G_DEFAULT)
    o70d, _ = run(ctx, a70, None, GEN.G_DEFAULT, device=True)
    assert not differ(o70, o70d)
    for i in range(len(ab)):
        o1, _ = run(ctx, a1.slice(i, i + 1), None, GEN.G_DEFAULT)
        for j in range(i, 70, len(ab)):
            assert all(np.array_equal(o1[k][0], o70[k][j], equal_nan=True) for k in o1 if k != "g_world"), (i, j)


def test_failed_windows_are_isolated(ctx, cases):
    """Good, failing (s < 0), singular (no IMU samples: the 3 x 3 system of the gyro bias is zero) and NaN-input windows in one batch."""
    good = [cases[NAMES.index(n)] for n in ("f11", "f16_irregular", "f17_head")]
    neg = cases[NAMES.index("f11_neg_T")]
    sing = (cases[NAMES.index("f11_ragged_bg")][0].copy(), cases[NAMES.index("f11_ragged_bg")][1].copy())
    sing[0].a["imu_n"][:] = 0
    nan = (cases[NAMES.index("f16_tail")][0].copy(), cases[NAMES.index("f16_tail")][1].copy())
    nan[0].a["frame_T"][0, 2, 1] = np.nan
    order = [good[0], neg, good[1], sing, nan, good[2]]
    al, win = stack_align([c[0] for c in order]), stack_windows([c[1] for c in order])
    out, w = run(ctx, al, win, GEN.G_DEFAULT)
    assert out["ok"].tolist() == [1, 0, 1, 0, 0, 1]
    gi = [0, 2, 5]
    alg = buffers.AlignArrays(dict(al.dims, n_windows=3), {k: v[gi] for k, v in al.a.items()})
    wing = buffers.WindowArrays(dict(win.dims, n_windows=3), {k: v[gi] for k, v in win.a.items()})
    outg, wg = run(ctx, alg, wing, GEN.G_DEFAULT)
    assert all(np.array_equal(outg[k], out[k][gi]) for k in outg)
    assert all(np.array_equal(wg.a[k], w.a[k][gi]) for k in wg.a)
    for b in (1, 3, 4):  # failed: pose, velocity, accelerometer bias and depths as they came, the gyro biases incremented
        assert np.isfinite(out["delta_bg"][b]).all()
        np.testing.assert_array_equal(w.a["pose"][b], win.a["pose"][b])
        np.testing.assert_array_equal(w.a["inv_depth"][b], win.a["inv_depth"][b])
        np.testing.assert_array_equal(w.a["speedbias"][b, :, :6], win.a["speedbias"][b, :, :6])
        np.testing.assert_array_equal(w.a["speedbias"][b, :, 6:9], win.a["speedbias"][b, :, 6:9] + out["delta_bg"][b])
    assert np.abs(out["delta_bg"][1]).max() > 0 and np.abs(out["delta_bg"][3]).max() == 0
    # alignment only: the three-frame case (rank deficient by count) next to the others
    f3 = cases[NAMES.index("f3_singular")][0]
    al2 = stack_align([good[0][0], f3, nan[0], good[1][0]])
    o2, _ = run(ctx, al2, None, GEN.G_DEFAULT)
    assert o2["ok"].tolist() == [1, 0, 0, 1]
    al2g = buffers.AlignArrays(dict(al2.dims, n_windows=2), {k: v[[0, 3]] for k, v in al2.a.items()})
    o2g, _ = run(ctx, al2g, None, GEN.G_DEFAULT)
    assert all(np.array_equal(o2g[k], o2[k][[0, 3]]) for k in o2g if k != "g_world")


def test_chain_into_the_solve(ctx):
    """visualInitialAlign, the reset of the linearization biases, then optimization(): the solve starts from what the alignment leaves."""
    al, win = synth.make_align(2, 17, key_index=GEN.IRR17, scale=2.5, first_id=913, ragged=True, n_feat=40)
    est = estimator_for(ctx, GEN.G_DEFAULT)
    out = est.visualInitialAlign(al, win)
    assert out.a["ok"].tolist() == [1, 1]
    est.reset_linearization_biases(win)
    assert np.array_equal(win.a["imu_lin_bg"], win.a["speedbias"][:, :10, 6:9]) and not win.a["imu_lin_ba"].any()
    summ = buffers.summary_to_numpy(est.optimization(win))
    print("termination", summ["termination"], "cost", summ["initial_cost"], "->", summ["final_cost"])
    assert (summ["termination"] != abi.TERM_NAMES.index("FAILURE")).all()
    assert (summ["final_cost"] <= summ["initial_cost"]).all()


def test_statuses_and_timings(ctx, cases):
    L = ctx._L
    al, win, g = cases[NAMES.index("f11")]
    est = estimator_for(ctx, g)

    def call(al, win, device):
        al, win = al.copy(), win.copy() if win is not None else None
        if device:
            al, win = al.to_device(), win.to_device() if win is not None else None
        out = buffers.AlignOutArrays.alloc(al.n_windows, al.dims["max_frames"], "cuda:0" if device else None)
        sa, so = al.struct(), out.struct()
        sw = win.struct() if win is not None else None
        return L.avm_visual_initial_align_batch(ctx.h, C.byref(est.options), al.mem, C.byref(sa), C.byref(sw) if sw is not None else None, C.byref(so))

    for device in (False, True):
        assert call(al, win, device) == abi.AVM_OK
        for key in ("align_gyro_bias", "align_solve", "align_apply"):
            assert ctx.kernel_ms(key) >= 0.0
        bad = al.copy()
        bad.a["n_frames"][0] = 1
        assert call(bad, None, device) == abi.AVM_ERR_INVALID and b"n_frames" in L.avm_last_error(ctx.h)
        bad = al.copy()
        bad.a["n_frames"][0] = 12
        assert call(bad, None, device) == abi.AVM_ERR_INVALID
        bad = al.copy()
        bad.a["imu_n"][0, 3] = al.dims["max_samp"] + 1
        assert call(bad, win, device) == abi.AVM_ERR_INVALID and b"imu_n" in L.avm_last_error(ctx.h)
        bad = al.copy()
        bad.a["key_index"][0, 4] = bad.a["key_index"][0, 3]
        assert call(bad, win, device) == abi.AVM_ERR_INVALID and b"key_index" in L.avm_last_error(ctx.h)
        assert call(bad, None, device) == abi.AVM_OK  # (key_index is only read with windows)
        bad = al.copy()
        bad.a["key_index"][0, 10] = 11
        assert call(bad, win, device) == abi.AVM_ERR_INVALID
    big = stack_align([al, synth.make_align(1, 4, max_frames=65)[0]])
    assert call(big, None, False) == abi.AVM_ERR_CAPACITY and b"max_frames" in L.avm_last_error(ctx.h)
    # a batch above avm_config::max_windows
    cfg = abi.Config()
    cfg.device, cfg.abi_version, cfg.max_windows = 0, abi.AVM_ABI_VERSION, 1
    h = C.c_void_p()
    assert L.avm_create(C.byref(cfg), C.byref(h)) == abi.AVM_OK
    try:
        two = stack_align([al, al])
        out = buffers.AlignOutArrays.alloc(2, 11)
        sa, so = two.struct(), out.struct()
        assert L.avm_visual_initial_align_batch(h, C.byref(est.options), two.mem, C.byref(sa), None, C.byref(so)) == abi.AVM_ERR_CAPACITY
        one = al.copy()
        sa = one.struct()
        assert L.avm_visual_initial_align_batch(h, C.byref(est.options), one.mem, C.byref(sa), None, C.byref(so)) == abi.AVM_OK
    finally:
        L.avm_destroy(h)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    import align_host

    return align_host.build_shim(tmp_path_factory.mktemp("align_shim"))


@pytest.mark.parametrize("name", ["f17_irregular", "f33_stride2", "f33_irregular", "f11_neg_T"])  # (f33_irregular: non-zero incoming Bgs)
def test_cpp_host_visual_initial_align(ctx, cases, shim, name):
    """avm_host::Estimator::visualInitialAlign() leaves the states the Python mirror leaves, bit for bit, and flips solver_flag."""
    import align_host

    ci = NAMES.index(name)
    al, win, g = cases[ci]
    F, nf = GEN.CASES[ci][2], int(win.a["n_feat"][0])
    out, w = run(ctx, al, win, g)
    H = align_host.AlignHost(shim)
    assert H.load(al, win, 0) == 0, H.err()
    rc, res = H.align()
    assert rc == 0, H.err()
    st = H.state(F, nf)
    assert res == int(out["ok"][0]) == int(GEN.CASES[ci][6] is None) and st["solver_flag"] == res
    np.testing.assert_array_equal(st["pose"], w.a["pose"][0])
    np.testing.assert_array_equal(st["speedbias"], w.a["speedbias"][0])
    np.testing.assert_array_equal(st["inv_depth"][:nf], w.a["inv_depth"][0, :nf])
    np.testing.assert_array_equal(st["delta_bg"], out["delta_bg"][0])
    np.testing.assert_array_equal(st["x"], out["x"][0])
    bg = w.a["speedbias"][0, :, 6:9]
    np.testing.assert_array_equal(st["lin_all"], np.tile(np.concatenate([np.zeros(3), bg[0]]), (F - 1, 1)))  # repropagate(0, Bgs[0]), whatever the outcome
    if res:
        np.testing.assert_array_equal(st["g"], out["g_world"][0])
        np.testing.assert_array_equal(st["lin"], np.concatenate([np.zeros((10, 3)), bg[1:]], axis=1))  # pre_integrations[i]->repropagate(0, Bgs[i])
        assert st["is_key"].tolist() == [int(k in GEN.CASES[ci][3]) for k in range(F)]
    else:
        assert not st["g"].any() and not st["is_key"].any()
        np.testing.assert_array_equal(st["lin"][:, 3:], win.a["imu_lin_bg"][0])
