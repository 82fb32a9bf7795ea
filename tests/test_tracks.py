"""GPU tier (-m gpu): the feature manager on device-resident tables - avm_add_image_batch, avm_imu_push_batch, avm_solve_view_batch,
avm_solve_view_store_depths, avm_slide_window_tracks - against the Python statements of tests/test_tracks_cpu.py (checked there on
hand-computed cases).  Everything compared is integers and copied doubles: every comparison is np.array_equal.

Test 1 runs on full tables of strides 160 / 1200: a 130-point image leaves at least 130 rows in its window, which the 96 rows first
planned for these tables cannot hold; the list lengths (0, 1, 63, 64, 65, 90) and image sizes (0, 1, 64, 65, 130, 70) are as planned.
"""
import copy
import ctypes as C
import importlib

import numpy as np
import pytest

from helpers import abi, blank_windows, buffers, synth
from test_mixed_batch import MIN_PARALLAX, ROLLED, _hand_prior_over, _host, _place, _vec
from test_mixed_batch_cpu import decision_statement
from test_tracks_cpu import (add_image_statement, features_with_ids, roll_tracks_statement, store_depths_statement, tables_from_features,
                             view_statement)

pytestmark = pytest.mark.gpu

est_m = importlib.import_module("anticipated-vins-mono_amd.estimator")
lib_m = importlib.import_module("anticipated-vins-mono_amd.lib")

OLD, SECOND_NEW = abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW
TRACKS = ("n_feat", "feat_start", "feat_nobs", "feat_obs_begin", "inv_depth", "obs_xy")
WHERE = pytest.mark.parametrize("where", ["host", "device"])


def _set_tracks(w, lists, with_td):
    """the lists as the track tables of `w` (dense); returns feat_id [B, max_feat]"""
    t = tables_from_features(lists, w.dims["max_feat"], w.dims["max_obs"], with_td)
    for k in TRACKS + (("obs_vel_td",) if with_td else ()):
        w.a[k] = t[k]
    return t["feat_id"]


def _lists(w, fid):
    return [features_with_ids(w.a, fid, b) for b in range(w.n_windows)]


def _assert_tables_equal_lists(w, fid, lists, with_td, before=None, before_fid=None):
    """w / fid (host) hold exactly `lists`, dense in list order; with `before`: every slot beyond is what it was"""
    t = tables_from_features(lists, w.dims["max_feat"], w.dims["max_obs"], with_td)
    assert np.array_equal(w.a["n_feat"], t["n_feat"])
    for b in range(w.n_windows):
        n = int(t["n_feat"][b])
        total = int(t["feat_nobs"][b, :n].sum())
        assert np.array_equal(fid[b, :n], t["feat_id"][b, :n]), b
        for k in ("feat_start", "feat_nobs", "feat_obs_begin", "inv_depth"):
            assert np.array_equal(w.a[k][b, :n], t[k][b, :n]), (b, k)
        for k in ("obs_xy",) + (("obs_vel_td",) if with_td else ()):
            assert np.array_equal(w.a[k][b, :total], t[k][b, :total]), (b, k)
            if before is not None:
                assert np.array_equal(w.a[k][b, total:], before.a[k][b, total:]), (b, k)
        if before is not None:
            assert np.array_equal(fid[b, n:], before_fid[b, n:]), b
            for k in ("feat_start", "feat_nobs", "feat_obs_begin", "inv_depth"):
                assert np.array_equal(w.a[k][b, n:], before.a[k][b, n:]), (b, k)


# ---------------------------------------------------------------- the tables of tests 1 and 3
LIST_LENGTHS, IMAGE_SIZES, MATCHED = (0, 1, 63, 64, 65, 90), (0, 1, 64, 65, 130, 70), (0, 1, 40, 44, 45, 64)
ROLL_FLAGS = [OLD, SECOND_NEW, OLD, SECOND_NEW, OLD, SECOND_NEW]
MAX_FEAT, MAX_OBS, MAX_PTS = 160, 1200, 160


def _pre_roll_tables(with_td, seed=3):
    """Six windows whose lists no roll shortens (start-0 tracks have >= 3 observations, no one-observation track in frame 9): ids in no
    order, most tracks reach frame 10."""
    rng = np.random.default_rng(seed)
    w = blank_windows(6, max_feat=MAX_FEAT, max_obs=MAX_OBS)
    w.a["imu_n"][:] = 8                                                     # (MARGIN_SECOND_NEW appends interval 9 to interval 8: 16 of 20)
    lists = []
    for b, n in enumerate(LIST_LENGTHS):
        ids = rng.permutation(3 * n + 5)[:n] * 2 + 1                       # odd ids: the image's new ids are even
        starts = np.sort(np.r_[rng.integers(0, 9, max(0, n - 4)), [9, 9, 10, 10][:min(n, 4)]])[:n]
        feats = []
        for i, st in enumerate(starts):
            st = int(st)
            if st >= 9 or rng.uniform() < 0.8:
                no = 11 - st                                                # tracked up to frame 10
            else:
                no = int(rng.integers(3 if st == 0 else 1, 10 - st + 1))   # lost in frame 9 or before
            # (image motion: large in the odd windows, a tenth of MIN_PARALLAX in the even ones - the windows do not all decide alike)
            xy = rng.normal(scale=0.3, size=2) + rng.normal(scale=0.3 if b % 2 else 0.002, size=(no, 2))
            f = dict(id=int(ids[i]), start=st, obs=[tuple(v) for v in xy], inv_depth=float(rng.uniform(0.1, 0.5)))
            if with_td:
                f["td"] = [tuple(v) for v in rng.normal(size=(no, 4))]
            feats.append(f)
        lists.append(feats)
    if with_td:
        w.a["obs_vel_td"] = np.zeros((6, MAX_OBS, 4))
    fid = _set_tracks(w, lists, with_td)
    # (slots no list uses hold values of their own: "left as they were" can be seen)
    for b in range(6):
        n, total = int(w.a["n_feat"][b]), int(w.a["feat_nobs"][b].sum())
        w.a["obs_xy"][b, total:] = 7.0 + np.arange(MAX_OBS - total)[:, None]
        w.a["inv_depth"][b, n:], fid[b, n:] = 9.0, -5
    return w, fid


def _rolled(E, with_td, where):
    """the tables after a roll of each kind through avm_slide_window_tracks, placed `where`, and their host copies"""
    w, fid = _pre_roll_tables(with_td)
    g, gfid = _place(w, where), _vec(fid, where)
    E.slideWindow(g, _vec(ROLL_FLAGS, where), True, 5.0, feat_id=gfid)
    h, hfid = (g.to_host(), _host(gfid)) if where == "device" else (g.copy(), gfid.copy())
    assert h.a["n_feat"].tolist() == list(LIST_LENGTHS)
    # holes and rows shifted both ways: the tables are not dense any more
    dense = tables_from_features(_lists(h, hfid), MAX_FEAT, MAX_OBS, with_td)
    assert not np.array_equal(dense["feat_obs_begin"], h.a["feat_obs_begin"])
    return g, gfid, h, hfid


def _images(h, hfid, with_td, seed=8):
    """per window MATCHED ids of tracks that end in frame 9 plus new (even) ids, below, between and above the matched ones"""
    rng = np.random.default_rng(seed)
    images = []
    for b in range(6):
        n = int(h.a["n_feat"][b])
        ends9 = [e for e in range(n) if h.a["feat_start"][b, e] + h.a["feat_nobs"][b, e] == 10]
        assert len(ends9) >= MATCHED[b], (b, len(ends9))
        rows = rng.permutation(ends9)[:MATCHED[b]]
        ids = [int(hfid[b, e]) for e in rows] + [int(x) * 2 for x in rng.permutation(400)[:IMAGE_SIZES[b] - MATCHED[b]]]
        assert len(set(ids)) == IMAGE_SIZES[b]
        images.append({i: tuple(rng.normal(scale=0.3, size=6 if with_td else 2)) for i in ids})
        if n > 64:
            assert min(rows) < 64 <= max(rows)                              # matched rows on both sides of the list's 64 boundary
    return images


# ---------------------------------------------------------------- 1: the append
@WHERE
@pytest.mark.parametrize("with_td", [False, True])
def test_append_equals_the_statement(ctx, where, with_td):
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    g, gfid, h, hfid = _rolled(E, with_td, where)
    images = _images(h, hfid, with_td)
    img = buffers.ImageArrays.from_maps(images, MAX_PTS, with_td)
    flags, ltn, par = (_host(x) for x in E.addFeatureCheckParallax(g, gfid, img.to_device("cuda:0") if where == "device" else img, MIN_PARALLAX))
    r, rfid = (g.to_host(), _host(gfid)) if where == "device" else (g, gfid)
    want = [add_image_statement(feats, images[b]) for b, feats in enumerate(_lists(h, hfid))]
    assert [len(x) for x in want] == [l + p - m for l, p, m in zip(LIST_LENGTHS, IMAGE_SIZES, MATCHED)]
    _assert_tables_equal_lists(r, rfid, want, with_td, before=h, before_fid=hfid)
    for k in ("pose", "speedbias", "imu_n", "imu_dt"):
        assert np.array_equal(r.a[k], h.a[k]), k
    # the decision: the statement's and avm_keyframe_decision_batch's on the result
    stated = [decision_statement(r.a, b, MIN_PARALLAX) for b in range(6)]
    f2, l2, p2 = (_host(x) for x in E.keyframe_decision(g, MIN_PARALLAX))
    print("\n[append] flag, last_track_num, sum, num:", list(zip(flags.tolist(), ltn.tolist(), par[:, 0].tolist(), par[:, 1].tolist())))
    assert np.array_equal(flags, np.array([x[0] for x in stated], np.int32)) and np.array_equal(flags, f2)
    assert np.array_equal(ltn, np.array([x[1] for x in stated], np.int32)) and np.array_equal(ltn, l2)
    assert np.array_equal(par, np.array([[x[2], x[3]] for x in stated])) and np.array_equal(par, p2)
    assert ltn.tolist() == list(MATCHED) and {OLD, SECOND_NEW} == set(flags.tolist())
    assert ctx.kernel_ms("add_image") >= 0.0


# ---------------------------------------------------------------- 2: the view and the depths
def _full_from_solve_windows(n_feat=22, seed=4):
    """Three solvable windows (every row passes the filter) with rows between them that do not: tracks that start in frames 8, 9, 10 and
    one-observation tracks, some depths not triangulated yet.  Full strides 96 / 640."""
    rng = np.random.default_rng(seed)
    s = synth.make_windows(3, first_id=20, tracks="sparse", n_feat=n_feat, max_feat=150)
    d = dict(s.dims)
    d["max_feat"], d["max_obs"] = 96, 640
    full = buffers.WindowArrays(d, {k: v.copy() for k, v in s.a.items() if k not in TRACKS})
    lists = []
    for b in range(3):
        feats = features_with_ids(s.a, np.tile(np.arange(150, dtype=np.int32), (3, 1)), b)
        for f in feats[1::5]:
            f["inv_depth"] = -1.0                                           # "no depth yet": triangulate has work
        extra = [(8, 2), (8, 3), (9, 2), (10, 1), (3, 1), (0, 1), (9, 1), (5, 1), (8, 1)][: 9 - 2 * b]
        feats += [dict(id=0, start=st, obs=[tuple(v) for v in rng.normal(scale=0.3, size=(no, 2))], inv_depth=-1.0) for st, no in extra]
        feats.sort(key=lambda f: f["start"])                                # std::list order (stable)
        for f, i in zip(feats, rng.permutation(500)):
            f["id"] = int(i)
        lists.append(feats)
    fid = _set_tracks(full, lists, False)
    return full, fid, lists


@WHERE
@pytest.mark.parametrize("strides", [(150, 1650), (64, 256)])
def test_view_and_depths(ctx, where, strides):
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    E = est_m.Estimator(ctx=ctx, options=o)
    full, fid, lists = _full_from_solve_windows()
    mf, mo = strides
    T = buffers.TrackTables(full.copy(), fid.copy(), mf, mo)
    T = T.to_device("cuda:0") if where == "device" else T
    assert T.view.a["pose"] is T.full.a["pose"] and T.view.a["obs_xy"] is not T.full.a["obs_xy"]
    E.solve_view(T)
    views = [view_statement(feats) for feats in lists]
    want = tables_from_features([v for v, _ in views], mf, mo)
    H = T.to_host()
    for k in TRACKS:
        assert np.array_equal(H.view.a[k], want[k]), k                     # (the view's tables started as zeros: equal in every slot)
    for b, (v, rows) in enumerate(views):
        assert len(rows) >= 20 and np.array_equal(H.view_row[b, :len(rows)], np.array(rows, np.int32)) and (np.diff(rows) > 0).all()
    for k in full.a:
        assert np.array_equal(H.full.a[k], full.a[k]), k                    # the full tables are read only
    # triangulate + optimization on the view == the same calls on host-marshalled filtered tables of the same strides
    m = buffers.WindowArrays(dict(T.view.dims), {**{k: v.copy() for k, v in full.a.items() if k not in TRACKS}, **{k: want[k] for k in TRACKS}})
    m = _place(m, where)
    E.triangulate(T.view)
    E.optimization(T.view)
    E.triangulate(m)
    E.optimization(m)
    H, mh = T.to_host(), (m.to_host() if where == "device" else m)
    for k in ("pose", "speedbias", "ex_pose", "inv_depth"):
        assert np.array_equal(H.view.a[k], mh.a[k]), k
    assert not np.array_equal(H.view.a["pose"], full.a["pose"]) and np.array_equal(H.full.a["pose"], H.view.a["pose"])
    # setDepth: distinct values into the view, exactly those rows of the full tables change
    before = H.full.a["inv_depth"].copy()
    vd = 100.0 + np.arange(3)[:, None] * 7.0 + 0.5 * np.arange(mf)[None, :]
    T.view.a["inv_depth"][:] = _vec(vd, where, np.float64)
    E.setDepth(T)
    after = _host(T.full.a["inv_depth"])
    for b, (v, rows) in enumerate(views):
        expect = [f["inv_depth"] for f in store_depths_statement(features_with_ids(dict(H.full.a, inv_depth=before), fid, b), rows, vd[b])]
        assert np.array_equal(after[b, :len(expect)], np.array(expect)) and np.array_equal(after[b, len(expect):], before[b, len(expect):])
        assert (after[b, rows] == vd[b, :len(rows)]).all() and (np.delete(after[b], rows) == np.delete(before[b], rows)).all()
    assert ctx.kernel_ms("solve_view") >= 0.0 and ctx.kernel_ms("store_depths") >= 0.0


# ---------------------------------------------------------------- 3: the roll with ids
@WHERE
def test_roll_with_ids_and_td_rows(ctx, where):
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    w, fid = _pre_roll_tables(True)
    for b in range(6):                                                      # removeFailures has work: negative depths on rows the solve took
        take = [e for e in range(int(w.a["n_feat"][b])) if w.a["feat_nobs"][b, e] >= 2 and w.a["feat_start"][b, e] < 8][::7]
        w.a["inv_depth"][b, take] = -0.3
    g, gfid, old = _place(w, where), _vec(fid.copy(), where), _place(w, where)
    flags = _vec(ROLL_FLAGS, where)
    E.slideWindow(g, flags, True, 5.0, remove_failures=True, feat_id=gfid)
    E.slideWindow(old, flags, True, 5.0, remove_failures=True)              # avm_slide_window_flags
    g, gfid, old = (g.to_host(), _host(gfid), old.to_host()) if where == "device" else (g, gfid, old)
    for k in ROLLED:
        assert np.array_equal(g.a[k], old.a[k]), k                          # every array the older call writes
    assert np.array_equal(old.a["obs_vel_td"], w.a["obs_vel_td"])           # ... which still leaves obs_vel_td alone
    assert not np.array_equal(g.a["obs_vel_td"], w.a["obs_vel_td"])
    erased = 0
    for b in range(6):
        want = roll_tracks_statement(features_with_ids(w.a, fid, b), ROLL_FLAGS[b], True, True, w.a["pose"][b], w.a["ex_pose"][b])
        n = len(want)
        erased += int(w.a["n_feat"][b]) - n
        assert g.a["n_feat"][b] == n and np.array_equal(gfid[b, :n], np.array([f["id"] for f in want], np.int32)), b
        for e, f in enumerate(want):                                        # the td rows are with their observations
            ob, no = int(g.a["feat_obs_begin"][b, e]), int(g.a["feat_nobs"][b, e])
            assert no == len(f["obs"]) and g.a["feat_start"][b, e] == f["start"], (b, e)
            assert np.array_equal(g.a["obs_xy"][b, ob:ob + no], np.array(f["obs"]).reshape(-1, 2)), (b, e)
            assert np.array_equal(g.a["obs_vel_td"][b, ob:ob + no], np.array(f["td"]).reshape(-1, 4)), (b, e)
    assert erased > 6


# ---------------------------------------------------------------- 4: four streams, five frames
N_FRAMES, FULL_FEAT, FULL_OBS, SEQ_PTS = 5, 256, 2816, 160


def _stream_start(E):
    """Four synth.Sequence streams after their first roll (MARGIN_OLD): tables that hold frames up to 9, the state a frame's loop starts
    from.  Returns host TrackTables (full strides FULL_FEAT / FULL_OBS, view 150 / 1650) and the sequences."""
    seqs = [synth.Sequence(70 + b, n_frames=24, n_landmarks=140, max_feat=150, max_samp=160) for b in range(4)]
    firsts = [s.first_window() for s in seqs]
    w0 = firsts[0][0]
    d = dict(w0.dims)
    d["n_windows"], d["max_feat"], d["max_obs"] = 4, FULL_FEAT, FULL_OBS
    full = buffers.WindowArrays(d, {k: np.concatenate([f[0].a[k] for f in firsts]) for k in w0.a if k not in TRACKS})
    lists = []
    for w, ids in firsts:
        lists.append(features_with_ids(w.a, np.array([ids + [0] * (150 - len(ids))], np.int32), 0))
    fid = _set_tracks(full, lists, False)
    E.slideWindow(full, OLD, True, 5.0, feat_id=fid)
    return buffers.TrackTables(full, fid), seqs


def _frame_inputs(seqs, t, rng):
    """frame t of the run: the image {landmark id: observation} of absolute frame 11 + t plus three ids seen once, and the IMU samples"""
    F = 11 + t
    images, dt, acc, gyr = [], np.zeros((4, 20)), np.zeros((4, 20, 3)), np.zeros((4, 20, 3))
    for b, s in enumerate(seqs):
        im = {li: tuple(obs[F]) for li, (_, obs, _) in enumerate(s.tracks) if F in obs}
        for k in range(3):
            im[100000 + 10 * t + k] = tuple(rng.uniform(-0.5, 0.5, 2))
        images.append(im)
        d, a, g = s.imu_interval(F - 1)
        dt[b], acc[b], gyr[b] = d, a[1:], g[1:]
    return images, dt, acc, gyr


def _min_parallax_between(full, B=4):
    means = sorted(x[2] / x[3] for x in (decision_statement(full.a, b, 0.0) for b in range(B)) if x[3] > 0)
    assert len(means) == B
    return 0.5 * (means[1] + means[2])


def test_four_streams_five_frames(ctx, monkeypatch):
    monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    start, seqs = _stream_start(E)
    rng = np.random.default_rng(21)
    frames = [_frame_inputs(seqs, t, rng) for t in range(N_FRAMES)]

    # ---- run B: the list as Python dicts (the statements), the existing calls on marshalled tables of the same strides
    Tb = start.copy()
    lists = _lists(Tb.full, Tb.feat_id)
    decisions_b, min_parallax = [], []
    for images, dt, acc, gyr in frames:
        a = Tb.full.a
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
        assert sorted(set(flags.tolist())) == [OLD, SECOND_NEW]             # the four streams do not all decide alike
        views = [view_statement(feats) for feats in lists]
        _set_tracks(Tb.view, [v for v, _ in views], False)
        E.triangulate(Tb.view)
        E.optimization(Tb.view, marginalization_flags=flags)
        prior = E.last_marginalization_info
        for b, (v, rows) in enumerate(views):
            store_depths_statement(lists[b], rows, Tb.view.a["inv_depth"][b, :len(rows)])
        _set_tracks(Tb.full, lists, False)
        failed = E.failureDetection(Tb.full, last_P)
        pose_before = a["pose"].copy()
        E.slideWindow(Tb.full, flags, True, 5.0, remove_failures=True)      # avm_slide_window_flags on the marshalled list
        for b in range(4):                                                  # the list follows by the statement; the depths are the roll's
            lists[b] = roll_tracks_statement(lists[b], int(flags[b]), True, True, pose_before[b], a["ex_pose"][b])
            assert a["n_feat"][b] == len(lists[b])
            for e, f in enumerate(lists[b]):
                assert (a["feat_start"][b, e], a["feat_nobs"][b, e]) == (f["start"], len(f["obs"]))
                f["inv_depth"] = float(a["inv_depth"][b, e])
        _hand_prior_over(Tb.full, prior)
        decisions_b.append((flags.copy(), ltn.copy(), par.copy(), failed.copy()))

    # ---- run A: the same frames on device tensors, the loop of INTEGRATION.md section 1; nothing goes to the host inside the loop
    Ta = start.to_device("cuda:0")
    dev = [(buffers.ImageArrays.from_maps(images, SEQ_PTS).to_device("cuda:0"), _vec(np.full(4, 20), "device"), _vec(dt, "device", np.float64),
            _vec(acc, "device", np.float64), _vec(gyr, "device", np.float64)) for images, dt, acc, gyr in frames]
    decisions_a = []
    for t, (img, n, dt, acc, gyr) in enumerate(dev):
        E.push_imu(Ta.full, n, dt, acc, gyr)
        E.imu_propagate(Ta.full)
        last_P = Ta.full.a["pose"][:, 10, :3].clone()
        flags, ltn, par = E.addFeatureCheckParallax(Ta.full, Ta.feat_id, img, min_parallax[t])
        for k in TRACKS:
            Ta.view.a[k].zero_()                                            # (run B marshals into zeroed tables)
        E.solve_view(Ta)
        E.triangulate(Ta.view)
        E.optimization(Ta.view, marginalization_flags=flags)
        prior = E.last_marginalization_info
        E.setDepth(Ta)
        failed = E.failureDetection(Ta.full, last_P)
        E.slideWindow(Ta.full, flags, True, 5.0, remove_failures=True, feat_id=Ta.feat_id)
        _hand_prior_over(Ta.full, prior)
        decisions_a.append((flags, ltn, par, failed))

    Ha = Ta.to_host()
    for t in range(N_FRAMES):
        for x, y in zip(decisions_a[t], decisions_b[t]):
            assert np.array_equal(_host(x), y), t
    print("\n[four streams, five frames] decisions:", [d[0].tolist() for d in decisions_b], "rows:", Ha.full.a["n_feat"].tolist())
    for k in ("pose", "speedbias", "ex_pose", "imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg", "prior_n", "prior_nblk", "prior_blk_kind",
              "prior_blk_frame", "prior_J", "prior_r", "prior_x0"):
        assert np.array_equal(Ha.full.a[k], Tb.full.a[k]), k
    assert (Ha.full.a["prior_n"] > 0).any()
    for b in range(4):
        n = len(lists[b])
        assert Ha.full.a["n_feat"][b] == n and n > 0
        assert np.array_equal(Ha.feat_id[b, :n], np.array([f["id"] for f in lists[b]], np.int32)), b
        assert np.array_equal(Ha.full.a["inv_depth"][b, :n], np.array([f["inv_depth"] for f in lists[b]])), b
        got = features_with_ids(Ha.full.a, Ha.feat_id, b)
        assert [(f["start"], f["obs"]) for f in got] == [(f["start"], [tuple(map(float, p)) for p in f["obs"]]) for f in lists[b]], b


# ---------------------------------------------------------------- 5: refusals
def _small(with_td=False):
    """three windows of five rows (max_feat 8, max_obs 32): ids 10, 4, 8, 6, 2; tracks 0 .. 3 end in frame 9, track 4 was lost in frame 5"""
    w = blank_windows(3, max_feat=8, max_obs=32, max_samp=8)
    feats = [dict(id=i, start=st, obs=[(0.1 * i, 0.01 * k) for k in range(no)], inv_depth=0.5)
             for i, st, no in ((10, 0, 10), (4, 2, 8), (8, 7, 3), (6, 9, 1), (2, 3, 3))]
    feats.sort(key=lambda f: f["start"])
    fid = _set_tracks(w, [copy.deepcopy(feats) for _ in range(3)], False)
    w.a["imu_n"][:] = 4
    return w, fid


def _image(points, max_pts=8, n_windows=3, bad_window=None, bad=None):
    """every window gets `points` ([(id, x, y)], in the order given); window `bad_window` gets `bad`"""
    a = {"n_pts": np.zeros(n_windows, np.int32), "feature_id": np.zeros((n_windows, max_pts), np.int32), "xy": np.zeros((n_windows, max_pts, 2))}
    for b in range(n_windows):
        pts = bad if b == bad_window else points
        a["n_pts"][b] = len(pts)
        for i, (fid, x, y) in enumerate(pts):
            a["feature_id"][b, i], a["xy"][b, i] = fid, (x, y)
    return buffers.ImageArrays({"n_windows": n_windows, "max_pts": max_pts}, a)


GOOD = [(4, 0.4, 0.4), (5, 0.5, 0.5), (10, 1.0, 1.0)]


def _refused(ctx, call, status, window, arrays, where):
    """`call()` returns `status`, avm_last_error names `window`, and every array of `arrays` (pairs: placed, host original) is untouched"""
    rc = call()
    msg = ctx._L.avm_last_error(ctx.h).decode()
    assert rc == status, (rc, msg)
    assert msg.startswith("window %d:" % window), msg
    for got, orig in arrays:
        if isinstance(orig, np.ndarray):
            assert _host(got).tobytes() == orig.tobytes()
        else:
            h = got.to_host() if where == "device" else got
            for k in orig.a:
                assert h.a[k].tobytes() == orig.a[k].tobytes(), k


@WHERE
def test_add_image_refusals(ctx, where):
    L = ctx._L

    def attempt(status, window, w, fid, img):
        g, gfid = _place(w, where), _vec(fid.copy(), where)
        gi = img.to_device("cuda:0") if where == "device" else img.copy()
        flags = _vec(np.full(3, 77), where)
        s, si = g.struct(), gi.struct()
        call = lambda: L.avm_add_image_batch(ctx.h, g.mem, C.byref(s), abi.iptr(gfid), C.byref(si), MIN_PARALLAX, abi.iptr(flags), None, None)
        _refused(ctx, call, status, window, [(g, w), (gfid, fid), (flags, np.full(3, 77, np.int32))], where)

    w, fid = _small()
    INV, CAP = abi.AVM_ERR_INVALID, abi.AVM_ERR_CAPACITY
    attempt(INV, 1, w, fid, _image(GOOD, bad_window=1, bad=[(4, 0.4, 0.4), (10, 1.0, 1.0), (5, 0.5, 0.5)]))      # ids not ascending
    attempt(INV, 2, w, fid, _image(GOOD, bad_window=2, bad=[(4, 0.4, 0.4), (4, 0.5, 0.5)]))                        # ... not strictly
    img = _image(GOOD)
    img.a["n_pts"][1] = 9
    attempt(INV, 1, w, fid, img)                                                                                     # n_pts > max_pts
    img.a["n_pts"][1] = -1
    attempt(INV, 1, w, fid, img)
    attempt(INV, 0, w, fid, _image(GOOD, bad_window=0, bad=[(2, 0.2, 0.2)]))                                         # a lost id comes back
    w2, fid2 = _small()
    w2.a["feat_nobs"][2, 0] = 11                                                                                     # a row that already has frame 10
    attempt(INV, 2, w2, fid2, _image(GOOD))
    fid3 = fid.copy()
    fid3[1, 4] = fid3[1, 1]                                                                                          # a duplicate in the id table
    attempt(INV, 1, w, fid3, _image([(5, 0.5, 0.5)]))
    attempt(CAP, 2, w, fid, _image(GOOD, bad_window=2, bad=[(4, 0.4, 0.4), (5, 0.5, 0.5), (7, 0.7, 0.7), (9, 0.9, 0.9), (11, 1.1, 1.1)]))   # 5 + 4 rows > 8
    w4, fid4 = _small()
    w4.dims["max_obs"] = 27                                                                                          # 25 observations + 3 > 27
    for k in ("obs_xy",):
        w4.a[k] = np.ascontiguousarray(w4.a[k][:, :27])
    attempt(CAP, 0, w4, fid4, _image(GOOD))
    # and the same tables take a good image
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    g, gfid = _place(w, where), _vec(fid.copy(), where)
    img = _image(GOOD)
    E.addFeatureCheckParallax(g, gfid, img.to_device("cuda:0") if where == "device" else img, MIN_PARALLAX)
    assert _host(g.a["n_feat"]).tolist() == [6, 6, 6] and _host(gfid)[0, :6].tolist() == [10, 4, 2, 8, 6, 5]


def test_a_refused_call_raises_with_the_entry_points_name_and_the_ctx_stays_usable(ctx):
    """The call path of the Python layer (Context.call) on a refusal: an image batch of three windows for tables of two."""
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    w = blank_windows(2)
    fid, before = np.zeros((2, w.dims["max_feat"]), np.int32), w.copy()
    three = buffers.ImageArrays.from_maps([{1: (0.1, 0.1)}] * 3, 4)
    assert three.n_windows != w.n_windows
    with pytest.raises(lib_m.AvmError) as e:
        E.addFeatureCheckParallax(w, fid, three, MIN_PARALLAX)
    assert str(e.value).startswith("avm_add_image_batch failed: status %d: " % abi.AVM_ERR_INVALID)
    assert "image->n_windows differs from windows->n_windows" in str(e.value)
    assert all(np.array_equal(w.a[k], before.a[k]) for k in w.a) and not fid.any()
    # ... and the same ctx takes the valid call
    two = buffers.ImageArrays.from_maps([{1: (0.1, 0.1)}, {2: (0.2, 0.2), 5: (0.5, 0.5)}], 4)
    flags, ltn, _ = E.addFeatureCheckParallax(w, fid, two, MIN_PARALLAX)
    assert w.a["n_feat"].tolist() == [1, 2] and fid[0, :1].tolist() == [1] and fid[1, :2].tolist() == [2, 5]
    assert flags.tolist() == [OLD, OLD] and ltn.tolist() == [0, 0]          # nothing tracked: a keyframe


@WHERE
def test_view_depths_and_imu_refusals(ctx, where):
    L = ctx._L
    INV, CAP = abi.AVM_ERR_INVALID, abi.AVM_ERR_CAPACITY
    # nine passing rows into view.max_feat = 8 (window 1)
    w = blank_windows(3, max_feat=12, max_obs=64, max_samp=8)
    nine = [dict(id=i, start=0, obs=[(0.0, 0.0)] * 3, inv_depth=0.5) for i in range(9)]
    fid = _set_tracks(w, [nine[:8], nine, nine[:2]], False)
    T = buffers.TrackTables(w.copy(), fid.copy(), 8, 88)
    T = T.to_device("cuda:0") if where == "device" else T
    T0 = T.to_host()
    sf, sv = T.full.struct(), T.view.struct()
    _refused(ctx, lambda: L.avm_solve_view_batch(ctx.h, T.full.mem, C.byref(sf), C.byref(sv), abi.iptr(T.view_row)), CAP, 1,
             [(T.full, T0.full), (T.view, T0.view), (T.view_row, T0.view_row)], where)
    T = buffers.TrackTables(w.copy(), fid.copy(), 12, 26)                  # 27 observations into view.max_obs = 26
    T = T.to_device("cuda:0") if where == "device" else T
    T0 = T.to_host()
    sf, sv = T.full.struct(), T.view.struct()
    _refused(ctx, lambda: L.avm_solve_view_batch(ctx.h, T.full.mem, C.byref(sf), C.byref(sv), abi.iptr(T.view_row)), CAP, 1,
             [(T.full, T0.full), (T.view, T0.view), (T.view_row, T0.view_row)], where)
    # setDepth: a view_row out of range (window 2), and one that does not increase (window 0)
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    for window, k, value in ((2, 1, 2), (2, 0, -1), (0, 3, 2)):
        T = buffers.TrackTables(w.copy(), fid.copy(), 12, 64)
        T = T.to_device("cuda:0") if where == "device" else T
        E.solve_view(T)
        T.view_row[window, k] = value
        T0 = T.to_host()
        sf, sv = T.full.struct(), T.view.struct()
        _refused(ctx, lambda: L.avm_solve_view_store_depths(ctx.h, T.full.mem, C.byref(sf), C.byref(sv), abi.iptr(T.view_row)), INV, window,
                 [(T.full, T0.full)], where)
    # avm_imu_push_batch: n out of range (window 1), too many samples for max_samp = 8 (window 2: 4 + 5)
    for status, window, n in ((INV, 1, [2, 6, 2]), (INV, 1, [2, -1, 2]), (CAP, 2, [4, 4, 5])):
        g = _place(w, where)
        g.a["imu_n"][:, 9] = 4
        g0 = g.to_host() if where == "device" else g.copy()
        s = g.struct()
        nn, dt, acc = _vec(n, where), _vec(np.full((3, 5), 0.005), where, np.float64), _vec(np.ones((3, 5, 3)), where, np.float64)
        _refused(ctx, lambda: L.avm_imu_push_batch(ctx.h, g.mem, C.byref(s), abi.iptr(nn), 5, abi.dptr(dt), abi.dptr(acc), abi.dptr(acc)), status, window,
                 [(g, g0)], where)
    # ... and a push that fits: the samples land behind the four that are there
    g = _place(w, where)
    g.a["imu_n"][:, 9] = 4
    dt, acc, gyr = np.arange(15.0).reshape(3, 5), np.arange(45.0).reshape(3, 5, 3), -np.arange(45.0).reshape(3, 5, 3)
    E.push_imu(g, _vec([4, 0, 3], where), _vec(dt, where, np.float64), _vec(acc, where, np.float64), _vec(gyr, where, np.float64))
    h = g.to_host() if where == "device" else g
    assert h.a["imu_n"][:, 9].tolist() == [8, 4, 7] and np.array_equal(h.a["imu_n"][:, :9], w.a["imu_n"][:, :9])
    assert np.array_equal(h.a["imu_dt"][0, 9, 4:8], dt[0, :4]) and np.array_equal(h.a["imu_acc"][2, 9, 5:8], acc[2, :3])
    assert np.array_equal(h.a["imu_gyr"][0, 9, 5:9], gyr[0, :4]) and np.array_equal(h.a["imu_dt"][:, :9], w.a["imu_dt"][:, :9])
    assert np.array_equal(h.a["imu_dt"][1], w.a["imu_dt"][1]) and np.array_equal(h.a["imu_acc"][:, 9, :5], w.a["imu_acc"][:, 9, :5])
    assert ctx.kernel_ms("imu_push") >= 0.0
