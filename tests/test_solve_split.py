"""GPU tier (-m gpu): the split solve, avm_window_solve_batch_relo - a batch of streams of which some have a relocalization pending.
The windows with relo_active == 0 take the kernel form the batch would get without the relocalization arrays, the others the extended
kernel; both through the list builds of the solve kernel (-DAVM_WIN_LIST), the marginalization once on the whole batch.

The yardstick is the one tests/test_mixed_batch.py relies on: results are bit-reproducible and independent of slot and batch
composition.  So every comparison is np.array_equal against the EXISTING entry point on the same batch:
  run P   the five relo_* arrays removed
  run X   the arrays present (every window through the extended kernel)
and window w of the split call equals P's window w where relo_active[w] == 0 and X's where it is not - states, every summary field and
the raw avm_prior_out rows.  The forms of all three runs are asserted, so that equal forms are compared.  Only the direct oracle check
has tolerances: those of tests/test_extended_solve.py for the same quantities.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import abi, buffers, synth
from test_extended_solve import _assert_parity, _opts
from test_mixed_batch import SIX_FLAGS, _concat, _host, _place, _six_windows, _solve_raw, _vec
from test_solve_split_cpu import partition_statement

pytestmark = pytest.mark.gpu

OLD, SECOND_NEW, NONE = abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW, abi.MARGIN_NONE
STATES = ("pose", "speedbias", "ex_pose", "inv_depth")
RELO = ("relo_n", "relo_frame", "relo_feat", "relo_xy", "relo_pose")
WHERE = pytest.mark.parametrize("where", ["host", "device"])


def _take(w, idx, drop=()):
    """the windows idx of w as a batch of its own (copies), without the arrays named in drop"""
    d = dict(w.dims)
    d["n_windows"] = len(idx)
    return buffers.WindowArrays(d, {k: np.ascontiguousarray(v[list(idx)]) for k, v in w.a.items() if k not in drop})


def _without_relo(w):
    return _take(w, range(w.n_windows), RELO)


def _solve_split(ctx, o, w, flags, active):
    """one call of avm_window_solve_batch_relo: the summaries and the raw avm_prior_out, on the host"""
    L, B = ctx._L, w.n_windows
    dev = "cuda:0" if w.on_device else None
    summ, prior = buffers.summary_alloc(B, dev), buffers.PriorOutArrays.alloc(B, 96, 16, dev)
    s, po = w.struct(), prior.struct()
    rc = L.avm_window_solve_batch_relo(ctx.h, C.byref(o), w.mem, C.byref(s), abi.iptr(flags), abi.iptr(active), C.byref(po), buffers.summary_ptr(summ))
    ctx.check(rc, "avm_window_solve_batch_relo")
    return buffers.summary_to_numpy(summ), (prior.to_host() if dev else prior)


def _run(ctx, o, w, where, flags=None, active=None):
    """w (host) through the existing entry point (active None) or the split one; returns (windows on the host, summaries, prior, forms, split)"""
    g = _place(w, where)
    f = None if flags is None else _vec(flags, where)
    if active is None:
        sm, pm = _solve_raw(ctx, o, g, f)
    else:
        sm, pm = _solve_split(ctx, o, g, f, _vec(active, where))
    gh = g.to_host() if where == "device" else g
    return gh, sm, pm, (ctx.last_solve_form(), ctx.last_marg_form()), ctx.last_split()


def _assert_window_equals(got, ref, b, states=STATES):
    gw, gs, gp = got[:3]
    rw, rs, rp = ref[:3]
    for k in states:
        assert np.array_equal(gw.a[k][b], rw.a[k][b]), (b, k)
    assert gs[b:b + 1].tobytes() == rs[b:b + 1].tobytes(), b
    for k in gp.a:
        assert gp.a[k][b].tobytes() == rp.a[k][b].tobytes(), (b, k)


def _assert_split_equals_P_and_X(w, split, P, X, active, states=STATES):
    for b, a in enumerate(np.asarray(active).tolist()):
        _assert_window_equals(split, X if a else P, b, states)
        if a:
            assert np.array_equal(split[0].a["relo_pose"][b], X[0].a["relo_pose"][b]), b
        else:                                                               # not written
            assert np.array_equal(split[0].a["relo_pose"][b], w.a["relo_pose"][b]), b


def _expected_split(active, plain_form, all_extended=False):
    plain, ext = partition_statement(active)
    if all_extended:
        return (0, len(active), -1, 1)
    return (len(plain), len(ext), -1 if not plain else plain_form, 1 if plain and ext else 0)


def _n_cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


# ---------------------------------------------------------------- 1: small windows, every pattern, around the ballot and chunk sizes
_SIX = {}


def _small_batch(B):
    """B windows tiled from _six_windows(relo=True): 12 / 33 / 60 features, dense and sparse, with and without a prior"""
    if "six" not in _SIX:
        _SIX["six"] = _six_windows(relo=True)
    return _take(_SIX["six"], [i % 6 for i in range(B)])


def _patterns(B):
    rng = np.random.default_rng(1000 + B)
    third = np.zeros(B, np.int32)
    third[rng.permutation(B)[:max(1, B // 3)]] = 1
    first, last = np.zeros(B, np.int32), np.zeros(B, np.int32)
    first[0], last[-1] = 1, 1
    return {"none": np.zeros(B, np.int32), "all": np.ones(B, np.int32), "first": first, "last": last,
            "alternating": (np.arange(B) % 2).astype(np.int32), "third": third}


@WHERE
@pytest.mark.parametrize("B", [1, 2, 63, 64, 65, 300])
def test_split_equals_the_existing_entry_point_small_windows(ctx, monkeypatch, where, B):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    monkeypatch.delenv("AVM_MARG_TP", raising=False)
    w = _small_batch(B)
    assert (w.a["relo_n"] >= 3).all()
    o = abi.default_options()
    o.marginalization_flag = OLD
    flags = [SIX_FLAGS[i % 6] for i in range(B)] if B == 65 else None       # (one case with the flag per window as well)
    P = _run(ctx, o, _without_relo(w), where, flags)
    X = _run(ctx, o, w, where, flags)
    # every form is the latency one while the batch gives no CU a second window; 300 windows on a device with fewer CUs take the forms of
    # the next test (P throughput / throughput, X latency / throughput, the split throughput / throughput): equal forms are compared either way
    big = B > _n_cus()
    assert B < 300 or big or _n_cus() >= 300
    tp = ("throughput", "throughput") if big else ("latency", "latency")
    assert P[3] == tp and X[3] == ("latency", tp[1])
    assert P[4] == (B, 0, int(big), 0) and X[4] == (0, B, -1, 0)
    assert not np.array_equal(P[0].a["pose"], X[0].a["pose"])               # (the relocalization factors do move the windows)
    for name, active in _patterns(B).items():
        S = _run(ctx, o, w, where, flags, active)
        plain = partition_statement(active)[0]
        assert S[3] == ((tp[0] if plain else "latency"), tp[1]) and S[4] == _expected_split(active, int(big)), (name, S[3], S[4])
        _assert_split_equals_P_and_X(w, S, P, X, active)
    assert ctx.kernel_ms("window_solve") > 0.0


# ---------------------------------------------------------------- 2: the throughput form, chosen from the size of the WHOLE batch
_TP = {}


def _tp_case(ctx, where):
    if where not in _TP:
        B = 2 * _n_cus() + 8
        six = _concat([synth.make_windows(1, first_id=140 + i, tracks="dense", n_feat=12, with_prior=i % 2 == 0, max_feat=150, relo=True) for i in range(6)])
        w = _take(six, [i % 6 for i in range(B)])
        o = abi.default_options()
        o.marginalization_flag = OLD
        _TP[where] = (w, o, _run(ctx, o, _without_relo(w), where), _run(ctx, o, w, where))
    return _TP[where]


@pytest.mark.parametrize("where,k", [("device", 1), ("device", 9), ("device", -1), ("host", 9)])
def test_plain_windows_take_the_throughput_form(ctx, monkeypatch, where, k):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    monkeypatch.delenv("AVM_MARG_TP", raising=False)
    w, o, P, X = _tp_case(ctx, where)
    B = w.n_windows
    assert P[3] == ("throughput", "throughput") and X[3] == ("latency", "throughput")   # (X: the extended batch beyond the CU count)
    k = B - 1 if k < 0 else k
    active = np.zeros(B, np.int32)
    active[np.random.default_rng(k).permutation(B)[:k]] = 1
    S = _run(ctx, o, w, where, None, active)
    assert S[3] == ("throughput", "throughput") and S[4] == (B - k, k, 1, 1)             # (B - 1 active: the one plain window all the same)
    _assert_split_equals_P_and_X(w, S, P, X, active)


def test_throughput_list_build_keeps_two_workgroups_per_cu(ctx):
    out, ref = (C.c_int * 2)(), (C.c_int * 2)()
    assert ctx._L.avm_debug_solve_tp_list_occupancy(out) == 1 and ctx._L.avm_debug_solve_tp_occupancy(ref) == 2
    assert out[0] == ref[0] == 2


# ---------------------------------------------------------------- 3: the rows of inactive windows
@WHERE
def test_rows_of_inactive_windows_are_neither_read_nor_written(ctx, monkeypatch, where):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    w = _small_batch(7)
    o = abi.default_options()
    o.marginalization_flag = OLD
    active = np.array([0, 1, 0, 0, 1, 1, 0], np.int32)
    clean = _run(ctx, o, w, where, None, active)
    g = w.copy()
    for b in np.flatnonzero(active == 0):
        g.a["relo_pose"][b], g.a["relo_xy"][b], g.a["relo_frame"][b] = -1234.5, 4321.0, 77
        g.a["relo_n"][b], g.a["relo_feat"][b] = (10 ** 9, 2 ** 30) if b % 2 else (-5, -99999)   # out of range either way
    S = _run(ctx, o, g, where, None, active)                               # not refused
    for b in range(7):
        _assert_window_equals(S, clean, b)
    for k in RELO:                                                          # the sentinels before the call and after it
        assert np.array_equal(S[0].a[k][active == 0], g.a[k][active == 0]), k
    assert np.array_equal(S[0].a["relo_pose"][active == 1], clean[0].a["relo_pose"][active == 1])
    assert not np.array_equal(S[0].a["relo_pose"][active == 1], w.a["relo_pose"][active == 1])


# ---------------------------------------------------------------- 4: estimate_td - every window through the extended list
@WHERE
def test_estimate_td_every_window_takes_the_extended_list(ctx, monkeypatch, where):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    w = synth.make_windows(6, first_id=90, tracks="sparse", n_feat=80, max_feat=150, td_true=0.01, relo=True)
    o = _opts(td=1, marg=OLD)
    states = STATES + ("td",)
    P = _run(ctx, o, _without_relo(w), where)
    X = _run(ctx, o, w, where)
    assert P[3] == X[3] == ("latency", "latency") and P[4] == X[4] == (0, 6, -1, 0)
    for active in (np.array([0, 1, 0, 1, 1, 0], np.int32), np.zeros(6, np.int32), np.ones(6, np.int32)):
        S = _run(ctx, o, w, where, None, active)
        assert S[3] == ("latency", "latency") and S[4] == _expected_split(active, 0, all_extended=True)
        _assert_split_equals_P_and_X(w, S, P, X, active, states)
    assert np.abs(S[0].a["td"]).min() > 1e-5                                # td was a variable


# ---------------------------------------------------------------- 5: refusals, and NULL
@WHERE
def test_refusals_write_nothing_and_name_the_rule(ctx, monkeypatch, where):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    w = _small_batch(6)
    o = abi.default_options()
    o.marginalization_flag = OLD
    dev = "cuda:0" if where == "device" else None

    def refused(batch, flags, active, match):
        g = _place(batch, where)
        prior, summ = buffers.PriorOutArrays.alloc(6, 96, 16, dev), buffers.summary_alloc(6, dev)
        for k in prior.a:
            prior.a[k][:] = 7
        s, po = g.struct(), prior.struct()
        f, act = None if flags is None else _vec(flags, where), _vec(active, where)      # (named: they live until the call returns)
        rc = ctx._L.avm_window_solve_batch_relo(ctx.h, C.byref(o), g.mem, C.byref(s), abi.iptr(f), abi.iptr(act), C.byref(po), buffers.summary_ptr(summ))
        assert rc == abi.AVM_ERR_INVALID and match in ctx._L.avm_last_error(ctx.h).decode(), ctx._L.avm_last_error(ctx.h)
        gh, ph = (g.to_host(), prior.to_host()) if dev else (g, prior)
        assert all(np.array_equal(gh.a[k], batch.a[k]) for k in batch.a) and all((ph.a[k] == 7).all() for k in ph.a)

    refused(_without_relo(w), None, [0, 1, 0, 0, 0, 0], "relo_active is given but relo_n")
    refused(_without_relo(w), None, [0, 0, 0, 0, 0, 0], "relo_active is given but relo_n")   # (whatever the values)
    refused(w, [OLD, NONE, 3, -1, OLD, OLD], [0, 1, 0, 1, 0, 0], "window 2: marginalization flag")


@pytest.mark.parametrize("flags", [None, SIX_FLAGS])
def test_null_relo_active_is_the_flags_entry_point(ctx, monkeypatch, flags):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    o = abi.default_options()
    o.marginalization_flag = SECOND_NEW
    w = _small_batch(6)
    a, b = w.copy(), w.copy()
    sa, pa = _solve_raw(ctx, o, a, None if flags is None else _vec(flags, "host"))
    split_a = ctx.last_split()
    sb, pb = _solve_split(ctx, o, b, None if flags is None else _vec(flags, "host"), None)
    assert split_a == ctx.last_split() == (0, 6, -1, 0)
    assert sa.tobytes() == sb.tobytes()
    for k in a.a:
        assert a.a[k].tobytes() == b.a[k].tobytes(), k
    for k in pa.a:
        assert pa.a[k].tobytes() == pb.a[k].tobytes(), k


# ---------------------------------------------------------------- 6: held against the oracle directly
def test_split_against_the_oracle(ctx, oracle, monkeypatch):
    """Active windows through the oracle with the relocalization arrays, inactive ones through it without; the tolerances are
    tests/test_extended_solve.py's (_assert_parity: 1e-6 relative on the states and the cost trace, the discrete fields exactly)."""
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    w = synth.make_windows(4, first_id=70, tracks="sparse", n_feat=90, max_feat=150, relo=True)
    o = _opts()
    active = np.array([0, 1, 1, 0], np.int32)
    S = _run(ctx, o, w, "device", None, active)
    assert S[4] == (2, 2, 0, 1)
    plain, ext = partition_statement(active)
    wa, wp = _take(w, ext), _take(w, plain, RELO)
    sa, sp = buffers.summary_alloc(2), buffers.summary_alloc(2)
    oracle.window_solve(o, wa, None, sa)
    oracle.window_solve(o, wp, None, sp)
    _assert_parity(_take(S[0], ext), wa, S[1][ext], sa, ["pose", "speedbias", "inv_depth", "ex_pose", "relo_pose"])
    _assert_parity(_take(S[0], plain), wp, S[1][plain], sp, ["pose", "speedbias", "inv_depth", "ex_pose"])
    assert np.array_equal(S[0].a["relo_pose"][plain], w.a["relo_pose"][plain])


# ---------------------------------------------------------------- 7: the stream loop
def test_streams_with_loop_closures_split(ctx, monkeypatch):
    """The four-stream, four-frame loop of tests/test_relo.py::test_streams_with_loop_closures on device tensors, with
    resolve_relo(split=True) and relo_active: after each solve every stream equals run P or run X of a clone of that frame's tables,
    according to its relocalization_info."""
    from test_relo import N_FRAMES, STREAM_MATCH, _E, _frame_messages, _stamp_of
    from test_tracks import SEQ_PTS, _frame_inputs, _lists, _min_parallax_between, _stream_start

    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    E = _E(ctx)
    o = E.options
    start, seqs = _stream_start(E)
    rng, rng_m = np.random.default_rng(21), np.random.default_rng(22)
    frames = [_frame_inputs(seqs, t, rng) for t in range(N_FRAMES)]
    Ta = start.to_device("cuda:0")
    SA = buffers.ReloState.alloc(4, STREAM_MATCH, "cuda:0")
    stamp = _vec(np.array([[_stamp_of(b, 1 + min(i, 9)) for i in range(11)] for b in range(4)]), "device", np.float64)
    n_active_seen, splits, spare = [], [], None
    for t, (images, dt, acc, gyr) in enumerate(frames):
        H = Ta.to_host()
        msgs = _frame_messages(t, _lists(H.full, H.feat_id), _host(stamp).tolist(), H.full.a["pose"], rng_m)
        if any(m is not None for m in msgs):
            E.setReloFrame(Ta.full, stamp, buffers.ReloMsgArrays.from_messages(msgs, STREAM_MATCH).to_device("cuda:0"), SA)
        E.headers_step(Ta.full, stamp, new_stamp=[_stamp_of(b, 11 + t) for b in range(4)])
        E.push_imu(Ta.full, _vec(np.full(4, 20), "device"), _vec(dt, "device", np.float64), _vec(acc, "device", np.float64), _vec(gyr, "device", np.float64))
        E.imu_propagate(Ta.full)
        image = buffers.ImageArrays.from_maps(images, SEQ_PTS).to_device("cuda:0")
        trial = Ta.copy()                                                   # the frame's parallax threshold: between the streams' means
        E.addFeatureCheckParallax(trial.full, trial.feat_id, image, 0.0)
        flags, _, _ = E.addFeatureCheckParallax(Ta.full, Ta.feat_id, image, _min_parallax_between(trial.full.to_host()))
        E.solve_view(Ta)
        n_active = E.resolve_relo(Ta, SA, split=True)
        n_active_seen.append(n_active)
        assert all(k in Ta.view.a for k in RELO)                            # attached whether or not a window is active
        E.triangulate(Ta.view)
        info = _host(SA.a["relocalization_info"]).copy()
        before = Ta.view.to_host()
        refs = {}
        for name, clone in (("P", _without_relo(before)), ("X", before.copy())):
            g = clone.to_device("cuda:0")
            sm, pm = _solve_raw(ctx, o, g, flags)
            refs[name] = (g.to_host(), sm, pm, (ctx.last_solve_form(), ctx.last_marg_form()))
        assert refs["P"][3] == refs["X"][3] == ("latency", "latency")
        E.optimization(Ta.view, marginalization_flags=flags, prior_out=spare, relo_active=True)
        splits.append(ctx.last_split())
        assert (ctx.last_solve_form(), ctx.last_marg_form()) == ("latency", "latency")
        after, sm = Ta.view.to_host(), buffers.summary_to_numpy(E.last_summary)
        for b in range(4):
            gw, gs = refs["X" if info[b] else "P"][:2]
            for k in STATES:
                assert np.array_equal(after.a[k][b], gw.a[k][b]), (t, b, k)
            assert sm[b:b + 1].tobytes() == gs[b:b + 1].tobytes(), (t, b)
            want = refs["X"][0].a["relo_pose"][b] if info[b] else before.a["relo_pose"][b]
            assert np.array_equal(after.a["relo_pose"][b], want), (t, b)
        prior = E.last_marginalization_info
        E.relo_finish(Ta.view, SA)                                          # every frame
        assert _host(SA.a["relocalization_info"]).tolist() == [0, 0, 0, 0]
        E.setDepth(Ta)
        E.slideWindow(Ta.full, flags, True, 5.0, remove_failures=True, feat_id=Ta.feat_id)
        Ta.swap_prior(prior)
        spare = prior
        E.headers_step(Ta.full, stamp, flags)
    assert n_active_seen == [0, 1, 1, 0]
    assert splits == [(4, 0, 0, 0), (3, 1, 0, 1), (3, 1, 0, 1), (4, 0, 0, 0)]
