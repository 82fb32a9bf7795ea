"""GPU tier (-m gpu): relocalization and the prior hand-over in the stream loop - avm_headers_step_batch, avm_set_relo_frame_batch,
avm_relo_resolve_batch, avm_relo_finish_batch, avm_prior_keep_batch - against the Python statements of tests/test_relo_cpu.py (checked
there on hand-computed cases) and, for the arithmetic of avm_relo_finish_batch, against the 50-digit values of tests/golden/relo.npz.

Everything but that arithmetic is integers and copied doubles: np.array_equal.  The outputs of avm_relo_finish_batch are held to
100 x err_fp64, the FP64 numpy statement's own distance from the 50-digit run (the maximum over the fixture's cases), in the fixture's
metric - the convention of tests/test_visual_align.py.  Measured on gfx950: 0.91 to 1.40 x err_fp64, the five
quantities, in both memory modes.
"""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import abi, blank_windows, buffers
from test_mixed_batch import _host, _place, _vec
from test_relo_cpu import (GEN, GOLD, headers_step_statement, prior_keep_statement, resolve_statement, set_relo_frame_statement)
from test_tracks_cpu import tables_from_features

pytestmark = pytest.mark.gpu

est_m = importlib.import_module("anticipated-vins-mono_amd.estimator")

OLD, SECOND_NEW, NONE = abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW, abi.MARGIN_NONE
INV, CAP = abi.AVM_ERR_INVALID, abi.AVM_ERR_CAPACITY
WHERE = pytest.mark.parametrize("where", ["host", "device"])
TRACKS = ("n_feat", "feat_start", "feat_nobs", "feat_obs_begin", "inv_depth", "obs_xy")
OUTPUTS = GEN.QUANTITIES


def _placed(x, where):
    """a *Arrays object where the test runs"""
    return x.to_device("cuda:0") if where == "device" else x.copy()


def _hosted(x):
    return x.to_host() if x.on_device else x


def _assert_same(got, want, what=""):
    """two *Arrays objects (host) hold the same bytes in every array"""
    assert set(got.a) == set(want.a)
    for k in want.a:
        assert got.a[k].tobytes() == want.a[k].tobytes(), (what, k)


def _E(ctx):
    return est_m.Estimator(ctx=ctx, options=abi.default_options())


# ---------------------------------------------------------------- 1: the frame stamps
@WHERE
@pytest.mark.parametrize("with_flags", [False, True])
@pytest.mark.parametrize("with_new", [False, True])
def test_headers_step_equals_the_statement(ctx, where, with_flags, with_new):
    rng = np.random.default_rng(5)
    w = _place(blank_windows(6), where)
    stamp = 1.4e9 + np.cumsum(rng.uniform(0.04, 0.06, (6, 11)), axis=1)
    flags, new = [OLD, SECOND_NEW] * 3, 1.4e9 + rng.uniform(1.0, 2.0, 6)
    g = _vec(stamp.copy(), where, np.float64)                               # (_vec hands a contiguous host array back as it is)
    _E(ctx).headers_step(w, g, _vec(flags, where) if with_flags else None, _vec(new, where, np.float64) if with_new else None)
    want = np.array([headers_step_statement(stamp[b].tolist(), flags[b] if with_flags else None, float(new[b]) if with_new else None) for b in range(6)])
    assert np.array_equal(_host(g), want)
    assert (with_flags or with_new) == (not np.array_equal(want, stamp))
    if with_flags or with_new:
        assert ctx.kernel_ms("headers_step") >= 0.0


# ---------------------------------------------------------------- 2: setReloFrame
MSG_MATCH, STATE_MATCH = 70, 80


def _state_dicts(S, b):
    a, n = S.a, int(S.a["n_match"][b])
    return dict(relocalization_info=int(a["relocalization_info"][b]), relo_frame=int(a["relo_frame"][b]), relo_stamp=float(a["relo_stamp"][b]),
                match_points=[(int(a["match_id"][b, k]),) + tuple(a["match_xy"][b, k]) for k in range(n)], prev_relo_t=a["prev_relo_t"][b].tolist(),
                prev_relo_q=a["prev_relo_q"][b].tolist(), relo_pose=a["relo_pose"][b].tolist())


def _store_state(S, b, d):
    a, n = S.a, len(d["match_points"])
    a["relocalization_info"][b], a["relo_frame"][b], a["relo_stamp"][b], a["n_match"][b] = d["relocalization_info"], d["relo_frame"], d["relo_stamp"], n
    for k, m in enumerate(d["match_points"]):
        a["match_id"][b, k], a["match_xy"][b, k] = m[0], m[1:3]
    a["prev_relo_t"][b], a["prev_relo_q"][b], a["relo_pose"][b] = d["prev_relo_t"], d["prev_relo_q"], d["relo_pose"]


def _seeded_state(B, max_match, rng):
    """a state whose every slot holds a value of its own: "untouched" can be seen"""
    S = buffers.ReloState.alloc(B, max_match)
    for k, v in S.a.items():
        S.a[k] = (rng.integers(1000, 2000, v.shape).astype(np.int32) if v.dtype == np.int32 else rng.uniform(50.0, 60.0, v.shape))
    S.a["relocalization_info"][:], S.a["relo_frame"][:] = 0, 3
    S.a["n_match"][:] = rng.integers(0, 5, B)
    return S


def _messages(stamp, rng):
    """eight windows: no message | frame 0, 0 matches | frame 9, 1 match | a stamp held by frames 3 and 6, 64 matches | no frame, 65 matches |
    frame 10 only, max_match matches | no message | frame 5, max_match matches"""
    plan = [None, (stamp[1, 0], 0), (stamp[2, 9], 1), (stamp[3, 3], 64), (123.0, 65), (stamp[5, 10], MSG_MATCH), None, (stamp[7, 5], MSG_MATCH)]
    out = []
    for p in plan:
        if p is None:
            out.append(None)
            continue
        ids = np.sort(rng.permutation(5000)[:p[1]])
        out.append(dict(frame_stamp=float(p[0]), matches=[(int(i),) + tuple(rng.uniform(-0.5, 0.5, 2)) for i in ids],
                        prev_relo_t=rng.uniform(-5, 5, 3).tolist(), prev_relo_q=rng.normal(size=4).tolist()))
    return out


@WHERE
def test_set_relo_frame_equals_the_statement(ctx, where):
    rng = np.random.default_rng(6)
    w = blank_windows(8)
    w.a["pose"] = rng.normal(size=(8, 11, 7))
    stamp = 100.0 + np.cumsum(rng.uniform(0.04, 0.06, (8, 11)), axis=1)
    stamp[3, 6] = stamp[3, 3]
    stamp[5, :10] -= 50.0                                                   # (window 5: only Headers[10] can equal its message's stamp)
    messages = _messages(stamp, rng)
    before = _seeded_state(8, STATE_MATCH, rng)
    want = before.copy()
    for b in range(8):
        _store_state(want, b, set_relo_frame_statement(_state_dicts(before, b), stamp[b].tolist(), w.a["pose"][b], messages[b]))
    assert want.a["relocalization_info"].tolist() == [0, 1, 1, 1, 0, 0, 0, 1] and want.a["relo_frame"].tolist() == [3, 0, 9, 6, 3, 3, 3, 5]
    assert want.a["n_match"].tolist()[1:6] == [0, 1, 64, 65, MSG_MATCH]
    g, S = _place(w, where), _placed(before, where)
    msg = _placed(buffers.ReloMsgArrays.from_messages(messages, MSG_MATCH), where)
    _E(ctx).setReloFrame(g, _vec(stamp, where, np.float64), msg, S)
    _assert_same(_hosted(S), want)
    for b in (0, 6):                                                        # no message: bit-identical to before
        for k in before.a:
            assert _hosted(S).a[k][b].tobytes() == before.a[k][b].tobytes(), (b, k)
    assert ctx.kernel_ms("set_relo") >= 0.0


# ---------------------------------------------------------------- 3: the match loop on the view
VIEW_LENGTHS, MATCH_COUNTS, RELO_FRAMES = (0, 1, 63, 64, 65, 150), (0, 1, 64, 65, 300), (0, 4, 9)
FULL_FEAT, FULL_OBS, MAX_MATCH = 160, 1200, 300


def _resolve_case(seed=7):
    """One window per (view length, match count), plus six inactive ones.  Full tables of strides 160 / 1200: beside the rows the solve
    takes, rows its filter drops (one observation, or a start in frames 8 .. 10); ids ascend along the list from 1000."""
    rng = np.random.default_rng(seed)
    combos = [(L, M) for L in VIEW_LENGTHS for M in MATCH_COUNTS] + [(L, 64) for L in VIEW_LENGTHS]
    B = len(combos)
    lists, matches, frames, active, kinds = [], [], [], [], []
    for b, (L, M) in enumerate(combos):
        rows = [(int(st), min(11 - int(st), int(rng.integers(2, 7 if L < 150 else 4)))) for st in rng.integers(0, 8, L)]
        rows += [(int(rng.integers(0, 8)), 1) for _ in range(min(6, FULL_FEAT - L - 4))] + [(8, 2), (9, 2), (10, 1)][:FULL_FEAT - L - 6]
        rows.sort(key=lambda r: r[0])
        ids = 1000 + np.cumsum(rng.integers(1, 9, len(rows)))
        feats = [dict(id=int(i), start=st, obs=[tuple(v) for v in rng.normal(scale=0.3, size=(no, 2))], inv_depth=0.5) for i, (st, no) in zip(ids, rows)]
        view_ids = [f["id"] for f in feats if len(f["obs"]) >= 2 and f["start"] < 8]
        assert len(view_ids) == L and len(feats) > L
        kind = b % 4                                                        # 0 below the list, 1 above, 2 interleaved, 3 identical
        if (L == M and L > 0) or (L, M) == (150, 300):
            kind = 3
        if kind == 0:
            mid = np.sort(rng.permutation(999)[:M])
        elif kind == 1:
            mid = int(ids[-1]) + 1 + np.sort(rng.permutation(4000)[:M])
        elif kind == 3 and M >= L:
            mid = np.array(sorted(view_ids + [int(ids[-1]) + 1 + k for k in range(M - L)]))   # every row of the view, then ids above
        else:                                                               # about half of them ids of the list (dropped rows' too)
            pool = [int(i) for i in ids]
            take = [int(x) for x in rng.permutation(pool)[:min(len(pool), (M + 1) // 2)]]
            rest = [int(x) for x in rng.permutation(np.setdiff1d(np.arange(900, 2600), pool))[:M - len(take)]]
            mid = np.array(sorted(take + rest))
        assert len(mid) == M and (np.diff(mid) > 0).all()
        lists.append(feats), kinds.append(kind)
        matches.append([(int(i),) + tuple(rng.uniform(-0.5, 0.5, 2)) for i in mid])
        frames.append(RELO_FRAMES[b % 3])
        active.append(b < len(VIEW_LENGTHS) * len(MATCH_COUNTS))
    full = blank_windows(B, max_feat=FULL_FEAT, max_obs=FULL_OBS)
    t = tables_from_features(lists, FULL_FEAT, FULL_OBS)
    for k in TRACKS:
        full.a[k] = t[k]
    S = buffers.ReloState.alloc(B, MAX_MATCH)
    for b in range(B):
        d = _state_dicts(S, b)
        d.update(relocalization_info=int(active[b]), relo_frame=frames[b], match_points=matches[b])
        _store_state(S, b, d)
    assert set(kinds) == {0, 1, 2, 3}
    return buffers.TrackTables(full, t["feat_id"]), S, lists, matches, frames, active


@WHERE
def test_resolve_equals_the_statement(ctx, where):
    E = _E(ctx)
    T, S, lists, matches, frames, active = _resolve_case()
    B = len(lists)
    T, S = (T.to_device("cuda:0"), S.to_device("cuda:0")) if where == "device" else (T, S)
    E.solve_view(T)
    assert _host(T.view.a["n_feat"]).tolist() == [L for L in VIEW_LENGTHS for _ in MATCH_COUNTS] + list(VIEW_LENGTHS)
    seed = {"relo_n": np.full(B, 77, np.int32), "relo_frame": np.full(B, 77, np.int32),
            "relo_feat": (5000 + np.arange(B * 150, dtype=np.int32)).reshape(B, 150), "relo_xy": 9.0 + np.arange(B * 300.0).reshape(B, 150, 2)}
    T._relo_out = {k: _vec(v.copy(), where, v.dtype) for k, v in seed.items()}
    S0 = _hosted(S).copy()
    n_active = E.resolve_relo(T, S)
    assert n_active == sum(active) == 30
    v = T.view.a
    assert v["relo_pose"] is S.a["relo_pose"] and all(v[k] is T._relo_out[k] for k in seed)
    got = {k: _host(v[k]) for k in seed}
    total = 0
    for b in range(B):
        if not active[b]:
            assert (got["relo_n"][b], got["relo_frame"][b]) == (0, 0), b
            n = 0
        else:
            feat, xy = resolve_statement(lists[b], frames[b], matches[b])
            n = len(feat)
            assert (got["relo_n"][b], got["relo_frame"][b]) == (n, frames[b]), b
            assert np.array_equal(got["relo_feat"][b, :n], np.array(feat, np.int32)), b
            assert np.array_equal(got["relo_xy"][b, :n], np.array(xy).reshape(-1, 2)), b
        assert np.array_equal(got["relo_feat"][b, n:], seed["relo_feat"][b, n:]) and np.array_equal(got["relo_xy"][b, n:], seed["relo_xy"][b, n:]), b
        total += n
    assert total > 300 and got["relo_n"].max() == 150
    _assert_same(_hosted(S), S0)                                            # the state is read only
    # no relocalization pending anywhere: the five arrays leave the view
    S.a["relocalization_info"][:] = 0
    assert E.resolve_relo(T, S) == 0 and not any(k.startswith("relo_") for k in T.view.a)
    assert ctx.kernel_ms("relo_resolve") >= 0.0


# ---------------------------------------------------------------- 4: the outputs of double2vector
def _finish_case():
    """the fixture's cases as windows 0 .. N - 1 (relo_frame = window % 10), with five windows in between and behind that have no
    relocalization pending"""
    gold = np.load(GOLD)
    N = gold["relo_pose"].shape[0]
    rng = np.random.default_rng(9)
    inactive = [3, 11, 20, N + 3, N + 4]
    B = N + len(inactive)
    case_of = [None if b in inactive else k for b, k in zip(range(B), np.cumsum([b not in inactive for b in range(B)]) - 1)]
    w = blank_windows(B)
    w.a["pose"] = rng.normal(size=(B, 11, 7))
    S = _seeded_state(B, 4, rng)
    for b, k in enumerate(case_of):
        if k is None:
            continue
        fr = b % 10
        S.a["relocalization_info"][b], S.a["relo_frame"][b] = 1, fr
        w.a["pose"][b, fr], S.a["relo_pose"][b] = gold["frame_pose"][k], gold["relo_pose"][k]
        S.a["prev_relo_t"][b], S.a["prev_relo_q"][b] = gold["prev_relo_t"][k], gold["prev_relo_q"][k]
    return gold, w, S, case_of


def _finish_bounds(gold):
    return {q: 100.0 * float(gold["err_fp64_" + q].max()) for q in OUTPUTS}


def _finish_distances(gold, S, case_of):
    """per quantity the largest distance from the 50-digit values over the active windows, in the fixture's metric"""
    worst = dict.fromkeys(OUTPUTS, 0.0)
    for b, k in enumerate(case_of):
        if k is None:
            continue
        scale = max(1.0, max(np.abs(gold[key][k]).max() for key in ("relo_pose", "frame_pose", "prev_relo_t", "prev_relo_q")))
        for q in OUTPUTS:
            worst[q] = max(worst[q], GEN.distance(q, np.atleast_1d(S.a[q][b]).tolist(), gold["m_" + q][k].tolist(), scale))
    return worst


@WHERE
def test_finish_against_the_50_digit_values(ctx, where):
    gold, w, S0, case_of = _finish_case()
    g, S = _place(w, where), _placed(S0, where)
    _E(ctx).relo_finish(g, S)
    H = _hosted(S)
    bounds, worst = _finish_bounds(gold), _finish_distances(gold, H, case_of)
    print("\n[relo_finish, %s] distance / err_fp64:" % where, {q: round(100.0 * worst[q] / bounds[q], 2) for q in OUTPUTS})
    for q in OUTPUTS:
        assert worst[q] <= bounds[q], (q, worst[q], bounds[q])
    active = np.array([k is not None for k in case_of])
    assert np.array_equal(H.a["relocalization_info"], np.zeros(len(case_of), np.int32)) and S0.a["relocalization_info"].tolist() == active.astype(int).tolist()
    for k in S0.a:                                                          # inactive windows: bit for bit; active ones: only the outputs and the flag
        assert H.a[k][~active].tobytes() == S0.a[k][~active].tobytes(), k
        if k not in OUTPUTS + ("relocalization_info",):
            assert H.a[k].tobytes() == S0.a[k].tobytes(), k
    assert ctx.kernel_ms("relo_finish") >= 0.0


# ---------------------------------------------------------------- 5: streams with loop closures, on the device
# (tests/test_tracks.py's _stream_start builds four streams: streams 0 .. 2 get the messages, stream 3 never does)
N_FRAMES, STREAM_MATCH = 4, 160


def _stamp_of(b, F):
    return 1000.0 * (b + 1) + 0.05 * F


def _frame_messages(t, lists, stamps, poses, rng):
    """The loop-closure messages that arrive before image t: stream 0 at t = 1 for the stamp of window frame 9, stream 1 at t = 1 for a
    stamp no frame has, stream 2 at t = 2 for window frame 0.  Matches: every other track that is observed in the matched frame and that
    the solve takes (its observation there plus 1e-3 noise), up to five tracks that start later, three ids the list does not hold."""
    plan = {1: {0: 9, 1: None}, 2: {2: 0}}.get(t, {})
    out = [None] * 4
    for b, i in plan.items():
        solved = [f for f in lists[b] if len(f["obs"]) >= 2 and f["start"] < abi.WINDOW_SIZE - 2]
        seen = [f for f in solved if i is not None and f["start"] <= i < f["start"] + len(f["obs"])][::2]
        later = [f for f in solved if i is not None and f["start"] > i][:5]
        assert i is None or len(seen) >= 5
        m = [(f["id"],) + tuple(np.array(f["obs"][i - f["start"]]) + 1e-3 * rng.normal(size=2)) for f in seen]
        m += [(f["id"],) + tuple(np.array(f["obs"][0]) + 1e-3 * rng.normal(size=2)) for f in later]
        m += [(50000 + 7 * k + b,) + tuple(rng.uniform(-0.5, 0.5, 2)) for k in range(3)]
        q = poses[b, i if i is not None else 0, 3:7] + 0.02 * rng.normal(size=4)
        out[b] = dict(frame_stamp=stamps[b][i] if i is not None else 9999.0, matches=sorted(m), prev_relo_q=(q / np.linalg.norm(q)).tolist(),
                      prev_relo_t=(poses[b, i if i is not None else 0, :3] + [0.3, -0.2, 0.1]).tolist())
    return out


def _used_prior(a, prefix=""):
    """the used parts of prior tables (host), window by window"""
    out = []
    for b in range(len(a[prefix + "n"])):
        n, nb = int(a[prefix + "n"][b]), int(a[prefix + "nblk"][b])
        out.append((n, nb, a[prefix + "blk_kind"][b, :nb].tolist(), a[prefix + "blk_frame"][b, :nb].tolist(), a[prefix + "J"][b, :n, :n].tobytes(),
                    a[prefix + "r"][b, :n].tobytes(), a[prefix + "x0"][b, :nb].tobytes()))
    return out


def test_streams_with_loop_closures(ctx, monkeypatch):
    from test_mixed_batch import _hand_prior_over
    from test_tracks import SEQ_PTS, _frame_inputs, _lists, _min_parallax_between, _set_tracks, _stream_start
    from test_tracks_cpu import add_image_statement, roll_tracks_statement, store_depths_statement, view_statement
    from test_relo_cpu import _blank_state

    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    E = _E(ctx)
    start, seqs = _stream_start(E)
    rng, rng_m = np.random.default_rng(21), np.random.default_rng(22)
    frames = [_frame_inputs(seqs, t, rng) for t in range(N_FRAMES)]
    stamps0 = [[_stamp_of(b, 1 + min(i, 9)) for i in range(11)] for b in range(4)]     # (the first roll, MARGIN_OLD, left Headers[10] = Headers[9])
    RELO = ("relo_n", "relo_frame", "relo_feat", "relo_xy", "relo_pose")

    # ---- chain B: the bookkeeping by the host - statements on the tables, numpy arithmetic of double2vector, copies of the prior
    Tb = start.copy()
    lists, stamps, states = _lists(Tb.full, Tb.feat_id), copy.deepcopy(stamps0), [_blank_state() for _ in range(4)]
    outputs = buffers.ReloState.alloc(4, STREAM_MATCH)                                 # (only its five outputs are used)
    messages, min_parallax, snaps_b, n_active_b, moved = [], [], [], [], []
    for t, (images, dt, acc, gyr) in enumerate(frames):
        a = Tb.full.a
        messages.append(_frame_messages(t, lists, stamps, a["pose"], rng_m))
        for b in range(4):
            set_relo_frame_statement(states[b], stamps[b], a["pose"][b], messages[t][b])
            stamps[b] = headers_step_statement(stamps[b], None, _stamp_of(b, 11 + t))
        set_pose = [list(s["relo_pose"]) for s in states]
        for b in range(4):                                                  # processIMU's buffers
            n9 = int(a["imu_n"][b, 9])
            a["imu_dt"][b, 9, n9:n9 + 20], a["imu_acc"][b, 9, n9 + 1:n9 + 21], a["imu_gyr"][b, 9, n9 + 1:n9 + 21] = dt[b], acc[b], gyr[b]
            a["imu_n"][b, 9] = n9 + 20
        E.imu_propagate(Tb.full)
        last_P = a["pose"][:, 10, :3].copy()
        lists = [add_image_statement(feats, images[b]) for b, feats in enumerate(lists)]
        Tb.feat_id = _set_tracks(Tb.full, lists, False)
        min_parallax.append(_min_parallax_between(Tb.full))
        flags, ltn, par = E.keyframe_decision(Tb.full, min_parallax[-1])
        views = [view_statement(feats) for feats in lists]
        _set_tracks(Tb.view, [v for v, _ in views], False)
        act = [s["relocalization_info"] != 0 for s in states]
        n_active_b.append(sum(act))
        for k in RELO:
            Tb.view.a.pop(k, None)
        if any(act):                                                        # the relo_* arrays, written by the test
            r = dict(relo_n=np.zeros(4, np.int32), relo_frame=np.zeros(4, np.int32), relo_feat=np.zeros((4, 150), np.int32),
                     relo_xy=np.zeros((4, 150, 2)), relo_pose=np.array([s["relo_pose"] for s in states]))
            for b in range(4):
                if act[b]:
                    feat, xy = resolve_statement(lists[b], states[b]["relo_frame"], states[b]["match_points"])
                    r["relo_n"][b], r["relo_frame"][b], r["relo_feat"][b, :len(feat)] = len(feat), states[b]["relo_frame"], feat
                    r["relo_xy"][b, :len(feat)] = np.array(xy).reshape(-1, 2)
                    assert len(feat) >= 5
            Tb.view.a.update(r)
        E.triangulate(Tb.view)
        E.optimization(Tb.view, marginalization_flags=flags)
        prior = E.last_marginalization_info
        if any(act):
            for b in range(4):
                states[b]["relo_pose"] = Tb.view.a["relo_pose"][b].tolist()
                if act[b]:
                    s = states[b]
                    f = GEN.finish_statement(s["relo_pose"], a["pose"][b, s["relo_frame"]], s["prev_relo_t"], s["prev_relo_q"])
                    for q in OUTPUTS:
                        outputs.a[q][b] = [float(v) for v in f[q]] if len(f[q]) > 1 else float(f[q][0])
                    s["relocalization_info"] = 0
                    moved.append(float(np.abs(np.array(s["relo_pose"]) - np.array(set_pose[b])).max()))
        for b, (v, rows) in enumerate(views):
            store_depths_statement(lists[b], rows, Tb.view.a["inv_depth"][b, :len(rows)])
        _set_tracks(Tb.full, lists, False)
        E.failureDetection(Tb.full, last_P)
        pose_before = a["pose"].copy()
        E.slideWindow(Tb.full, flags, True, 5.0, remove_failures=True)
        for b in range(4):
            lists[b] = roll_tracks_statement(lists[b], int(flags[b]), True, True, pose_before[b], a["ex_pose"][b])
            for e, f in enumerate(lists[b]):
                f["inv_depth"] = float(a["inv_depth"][b, e])
            stamps[b] = headers_step_statement(stamps[b], int(flags[b]))
        _hand_prior_over(Tb.full, prior)
        snaps_b.append(dict(pose=a["pose"].copy(), speedbias=a["speedbias"].copy(), n_feat=a["n_feat"].copy(),
                            inv_depth=[a["inv_depth"][b, :a["n_feat"][b]].copy() for b in range(4)], stamp=np.array(stamps),
                            relo_pose=np.array([s["relo_pose"] for s in states]), prior=_used_prior(a, "prior_"),
                            info=[s["relocalization_info"] for s in states], outputs={q: outputs.a[q].copy() for q in OUTPUTS}))
    assert n_active_b == [0, 1, 1, 0] and len(moved) == 2 and min(moved) > 1e-6, (n_active_b, moved)

    # ---- chain A: the same frames on device tensors, everything through the new calls; nothing goes to the host inside a frame
    Ta = start.to_device("cuda:0")
    SA = buffers.ReloState.alloc(4, STREAM_MATCH, "cuda:0")
    stamp = _vec(np.array(stamps0), "device", np.float64)
    gold = np.load(GOLD)
    bounds = _finish_bounds(gold)
    spare = None
    for t, (images, dt, acc, gyr) in enumerate(frames):
        if any(m is not None for m in messages[t]):
            E.setReloFrame(Ta.full, stamp, buffers.ReloMsgArrays.from_messages(messages[t], STREAM_MATCH).to_device("cuda:0"), SA)
        E.headers_step(Ta.full, stamp, new_stamp=[_stamp_of(b, 11 + t) for b in range(4)])
        E.push_imu(Ta.full, _vec(np.full(4, 20), "device"), _vec(dt, "device", np.float64), _vec(acc, "device", np.float64), _vec(gyr, "device", np.float64))
        E.imu_propagate(Ta.full)
        last_P = Ta.full.a["pose"][:, 10, :3].clone()
        flags, ltn, par = E.addFeatureCheckParallax(Ta.full, Ta.feat_id, buffers.ImageArrays.from_maps(images, SEQ_PTS).to_device("cuda:0"), min_parallax[t])
        for k in TRACKS:
            Ta.view.a[k].zero_()
        E.solve_view(Ta)
        n_active = E.resolve_relo(Ta, SA)
        assert n_active == n_active_b[t], t
        E.triangulate(Ta.view)
        E.optimization(Ta.view, marginalization_flags=flags, prior_out=spare)
        prior = E.last_marginalization_info
        if n_active:
            E.relo_finish(Ta.view, SA)
        E.setDepth(Ta)
        E.failureDetection(Ta.full, last_P)
        E.slideWindow(Ta.full, flags, True, 5.0, remove_failures=True, feat_id=Ta.feat_id)
        Ta.swap_prior(prior)                                                # the hand-over: an exchange of pointers
        spare = prior
        E.headers_step(Ta.full, stamp, flags)
        H, HS, sb = Ta.full.to_host(), SA.to_host(), snaps_b[t]
        for k in ("pose", "speedbias", "n_feat"):
            assert np.array_equal(H.a[k], sb[k]), (t, k)
        for b in range(4):
            assert np.array_equal(H.a["inv_depth"][b, :sb["n_feat"][b]], sb["inv_depth"][b]), (t, b)
        assert np.array_equal(_host(stamp), sb["stamp"]) and np.array_equal(HS.a["relo_pose"], sb["relo_pose"]), t
        assert _used_prior(H.a, "prior_") == sb["prior"], t
        assert HS.a["relocalization_info"].tolist() == sb["info"] == [0, 0, 0, 0], t
        for b in range(4):
            scale = max(1.0, float(np.abs(H.a["pose"][b, :, :3]).max()), float(np.abs(HS.a["prev_relo_t"][b]).max()))
            for q in OUTPUTS:
                d = GEN.distance(q, np.atleast_1d(HS.a[q][b]).tolist(), np.atleast_1d(sb["outputs"][q][b]).tolist(), scale)
                assert d <= bounds[q], (t, b, q, d, bounds[q])
    assert not np.array_equal(HS.a["drift_correct_t"][0], np.zeros(3)) and not np.array_equal(HS.a["relo_relative_t"][2], np.zeros(3))
    assert np.array_equal(HS.a["drift_correct_t"][[1, 3]], np.zeros((2, 3)))           # streams 1 and 3 never had a relocalization pending


# ---------------------------------------------------------------- 6: the prior hand-over
def _blocks(n):
    """block kinds / frames of a prior of n rows"""
    kinds = {0: [], 1: [abi.BLK_TD], 75: [abi.BLK_POSE] * 10 + [abi.BLK_SPEEDBIAS, abi.BLK_EXPOSE], 96: [abi.BLK_POSE] * 10 + [abi.BLK_SPEEDBIAS] * 4}[n]
    return kinds, [k % 10 for k in range(len(kinds))]


def _keep_case(slot_prior=104, slot_pblk=18):
    rng = np.random.default_rng(12)
    w = blank_windows(6)
    for b, n in enumerate([75, 96, 1, 75, 96, 0]):
        kinds, frames = _blocks(n)
        w.a["prior_n"][b], w.a["prior_nblk"][b] = n, len(kinds)
        w.a["prior_blk_kind"][b, :len(kinds)], w.a["prior_blk_frame"][b, :len(kinds)] = kinds, frames
    for k in ("prior_J", "prior_r", "prior_x0"):
        w.a[k] = rng.normal(size=w.a[k].shape)
    P = buffers.PriorOutArrays.alloc(6, slot_prior, slot_pblk)
    for k, v in P.a.items():
        P.a[k] = (rng.integers(0, 3, v.shape).astype(np.int32) if v.dtype == np.int32 else rng.uniform(50.0, 60.0, v.shape))
    P.a["n"][:] = [-1, 0, -1, 75, -1, -1]
    P.a["nblk"][:] = [5, 0, 5, 12, 5, 5]
    return w, P


def _prior_dict(a, b, prefix=""):
    return {k: (int(a[prefix + k][b]) if k in ("n", "nblk") else a[prefix + k][b]) for k in buffers.PRIOR_KEYS}


@WHERE
def test_prior_keep_equals_the_statement(ctx, where):
    w, P0 = _keep_case()
    want = P0.copy()
    for b in range(6):
        d = prior_keep_statement(_prior_dict(want.a, b), _prior_dict(w.a, b, "prior_"))
        want.a["n"][b], want.a["nblk"][b] = d["n"], d["nblk"]
    assert want.a["n"].tolist() == [75, 0, 1, 75, 96, 0] and want.a["nblk"].tolist() == [12, 0, 1, 12, 14, 0]
    g, P = _place(w, where), _placed(P0, where)
    _E(ctx).keep_prior(g, P)
    _assert_same(_hosted(P), want)
    for k in P0.a:                                                          # windows 1 and 3 reported n >= 0: untouched
        assert _hosted(P).a[k][[1, 3]].tobytes() == P0.a[k][[1, 3]].tobytes(), k
    assert not np.array_equal(want.a["J"], P0.a["J"]) and np.array_equal(want.a["J"][0, 75:], P0.a["J"][0, 75:])
    _assert_same(g.to_host() if where == "device" else g, w)
    assert ctx.kernel_ms("prior_keep") >= 0.0


def test_swap_prior_is_the_hand_over():
    w, P = _keep_case(96, 16)
    T = buffers.TrackTables(w, np.zeros((6, 8), np.int32))
    mine, theirs = {k: T.full.a["prior_" + k] for k in buffers.PRIOR_KEYS}, dict(P.a)
    T.swap_prior(P)
    for k in buffers.PRIOR_KEYS:
        assert T.full.a["prior_" + k] is theirs[k] and T.view.a["prior_" + k] is theirs[k] and P.a[k] is mine[k]
    with pytest.raises(ValueError):
        T.swap_prior(_keep_case()[1])


# ---------------------------------------------------------------- 7: refusals
def _refused(ctx, call, status, window, arrays):
    """`call()` returns `status`, avm_last_error names `window` (None: an argument check, no window to name), and every object of
    `arrays` (pairs: placed, host original - *Arrays objects or plain arrays) is untouched"""
    rc = call()
    msg = ctx._L.avm_last_error(ctx.h).decode()
    assert rc == status, (rc, msg)
    assert window is None or msg.startswith("window %d:" % window), msg
    for got, orig in arrays:
        if isinstance(orig, np.ndarray):
            assert _host(got).tobytes() == orig.tobytes()
        else:
            _assert_same(_hosted(got), orig, msg)


@WHERE
def test_headers_and_set_relo_refusals(ctx, where):
    L = ctx._L
    stamp = np.arange(66.0).reshape(6, 11)
    g = _vec(stamp.copy(), where, np.float64)
    flags = _vec([OLD, SECOND_NEW, OLD, NONE, 5, OLD], where)
    _refused(ctx, lambda: L.avm_headers_step_batch(ctx.h, int(where == "device"), 6, abi.dptr(g), abi.iptr(flags), None), INV, 3, [(g, stamp)])
    # setReloFrame
    rng = np.random.default_rng(13)
    w = blank_windows(8)
    stamp = 100.0 + np.cumsum(rng.uniform(0.04, 0.06, (8, 11)), axis=1)
    good = buffers.ReloMsgArrays.from_messages(_messages(stamp, rng), MSG_MATCH)
    S0 = _seeded_state(8, STATE_MATCH, rng)

    def attempt(status, window, msg, state=S0, windows=w):
        gw, gm, gs, gst = _place(windows, where), _placed(msg, where), _placed(state, where), _vec(stamp, where, np.float64)
        s, sm, ss = gw.struct(), gm.struct(), gs.struct()
        _refused(ctx, lambda: L.avm_set_relo_frame_batch(ctx.h, gw.mem, C.byref(s), abi.dptr(gst), C.byref(sm), C.byref(ss)), status, window,
                 [(gs, state), (gw, windows)])

    for n in (-1, MSG_MATCH + 1):
        bad = good.copy()
        bad.a["n_match"][3] = n
        attempt(INV, 3, bad)
    bad = good.copy()
    bad.a["match_id"][5, 40] = bad.a["match_id"][5, 39]                     # not strictly ascending
    attempt(INV, 5, bad)
    bad.a["n_match"][2] = -4                                                # ... and the first offending window is named
    attempt(INV, 2, bad)
    bad = good.copy()
    bad.a["n_match"][0], bad.a["match_id"][0, :2] = 2, [9, 3]               # a row without a message is not read
    gw, gm, gs = _place(w, where), _placed(bad, where), _placed(S0, where)
    _E(ctx).setReloFrame(gw, _vec(stamp, where, np.float64), gm, gs)
    attempt(CAP, None, good, _seeded_state(8, MSG_MATCH - 1, rng))          # state->max_match < msg->max_match
    attempt(INV, None, good, _seeded_state(7, STATE_MATCH, rng), blank_windows(7))   # msg->n_windows != windows->n_windows


@WHERE
def test_resolve_finish_and_keep_refusals(ctx, where):
    L, E = ctx._L, _E(ctx)
    T0, S0, lists, matches, frames, active = _resolve_case()
    B = len(lists)
    E0 = _E(ctx)
    Th = T0.copy()
    E0.solve_view(Th)                                                       # (host tables; the view the attempts start from)

    def attempt(status, window, change, max_feat=None):
        T, S = Th.copy(), S0.copy()
        change(T, S)
        T, S = (T.to_device("cuda:0"), S.to_device("cuda:0")) if where == "device" else (T, S)
        T1, S1 = T.to_host(), _hosted(S).copy()
        outs = [np.full(B, 77, np.int32), np.full(B, 77, np.int32), np.full((B, 150), 77, np.int32), np.full((B, 150, 2), 7.0)]
        gouts = [_vec(o.copy(), where, o.dtype) for o in outs]
        s, ss, n_active = T.view.struct(), S.struct(), C.c_int32(-9)
        if max_feat:
            s.max_feat = max_feat
        call = lambda: L.avm_relo_resolve_batch(ctx.h, T.view.mem, C.byref(s), abi.iptr(T.feat_id), FULL_FEAT, abi.iptr(T.view_row), C.byref(ss),
                                                abi.iptr(gouts[0]), abi.iptr(gouts[1]), abi.iptr(gouts[2]), abi.dptr(gouts[3]), C.byref(n_active))
        _refused(ctx, call, status, window, list(zip(gouts, outs)) + [(S, S1), (T.view, T1.view), (T.view_row, T1.view_row), (T.feat_id, T1.feat_id)])
        assert n_active.value == -9

    def set_item(name, idx, value, state=False):
        def f(T, S):
            (S.a[name] if state else (getattr(T, name) if hasattr(T, name) else T.full.a[name]))[idx] = value
        return f

    b = 13                                                                  # 63 rows, 65 matches, active
    assert active[b] and Th.view.a["n_feat"][b] == 63
    attempt(INV, b, set_item("view_row", (b, 5), int(Th.view_row[b, 4])))                    # view_row not strictly increasing
    attempt(INV, b, set_item("view_row", (b, 62), FULL_FEAT))                                # ... outside the full list
    attempt(INV, 31, set_item("view_row", (31, 0), -1))                                      # ... checked on an inactive window too
    r = int(Th.view_row[b, 7])
    attempt(INV, b, set_item("feat_id", (b, r), int(Th.feat_id[b, int(Th.view_row[b, 6])])))  # the view rows' ids not strictly ascending
    attempt(INV, b, set_item("match_id", (b, 64), int(S0.a["match_id"][b, 63]), state=True))  # the match ids
    attempt(INV, b, set_item("relo_frame", b, 10, state=True))
    attempt(INV, b, set_item("relo_frame", b, -1, state=True))
    attempt(INV, b, set_item("n_match", b, MAX_MATCH + 1, state=True))
    attempt(INV, b, set_item("n_match", b, -1, state=True))
    attempt(INV, 2, lambda T, S: (S.a["n_match"].__setitem__(b, -1), S.a["relo_frame"].__setitem__(2, 11)))   # the first offending window
    # an inactive window's state is not looked at
    T, S = Th.copy(), S0.copy()
    S.a["n_match"][32], S.a["relo_frame"][32], S.a["match_id"][33, :2] = -1, 55, [9, 3]
    T, S = (T.to_device("cuda:0"), S.to_device("cuda:0")) if where == "device" else (T, S)
    assert E.resolve_relo(T, S) == 30
    attempt(CAP, None, lambda T, S: None, max_feat=151)                                       # view->max_feat > AVM_MAX_FEAT
    # avm_relo_finish_batch: relo_frame outside [0, WINDOW_SIZE) on a window with a relocalization pending
    gold, w, F0, case_of = _finish_case()
    for window, value in ((6, 10), (2, -1)):
        F = F0.copy()
        F.a["relo_frame"][window] = value
        F.a["relo_frame"][3] = 99                                           # (window 3 has none pending: not looked at)
        g, gF = _place(w, where), _placed(F, where)
        s, ss = g.struct(), gF.struct()
        _refused(ctx, lambda: L.avm_relo_finish_batch(ctx.h, g.mem, C.byref(s), C.byref(ss)), INV, window, [(gF, F), (g, w)])
    # avm_prior_keep_batch: a kept prior that does not fit the slots (window 0 keeps 75 rows / 12 blocks; window 4 96 / 14)
    for window, strides in ((0, (74, 18)), (0, (104, 11)), (4, (80, 13))):
        w, P0 = _keep_case(*strides)
        g, P = _place(w, where), _placed(P0, where)
        s, po = g.struct(), P.struct()
        _refused(ctx, lambda: L.avm_prior_keep_batch(ctx.h, g.mem, C.byref(s), C.byref(po)), CAP, window, [(P, P0), (g, w)])
    w, P0 = _keep_case()
    w.a["prior_nblk"][5] = 17                                               # the window's own table: prior_n == 0 with a block count outside the table
    g, P = _place(w, where), _placed(P0, where)
    s, po = g.struct(), P.struct()
    _refused(ctx, lambda: L.avm_prior_keep_batch(ctx.h, g.mem, C.byref(s), C.byref(po)), INV, 5, [(P, P0), (g, w)])
