"""CPU tier of the relocalization and the prior hand-over in the stream loop (avm_headers_step_batch, avm_set_relo_frame_batch,
avm_relo_resolve_batch, avm_relo_finish_batch, avm_prior_keep_batch): the header and the ctypes prototypes, the Python statements of the
reference that tests/test_relo.py holds the kernels against - checked here on hand-computed cases, without a GPU - and the fixture
tests/golden/relo.npz against the FP64 statement it was generated with.

  headers_step_statement    Headers[] through slideWindow (estimator.cpp:1015,1021,1064) and processImage (:126)
  set_relo_frame_statement  Estimator::setReloFrame (:1109-1127); relo_pose from the pose of frame i (the deviation avm.h documents)
  resolve_statement         the two-pointer loop of optimization() (:765-790) over f_manager.feature as a list of dicts (the form of
                            tests/test_tracks_cpu.py), with the bound on retrive_feature_index the reference lacks
  prior_keep_statement      estimator.cpp:926-927 on one slot: the used part of the prior the window was solved with
"""
import ctypes as C
import importlib
import os
import re
import sys

import numpy as np

from helpers import abi
from helpers import header_arg_count as _header_arg_count, header_text as _header

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import gen_relo as GEN  # noqa: E402

WINDOW_SIZE = abi.WINDOW_SIZE
OLD, SECOND_NEW = abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW
RELO_ENTRY_POINTS = ("avm_headers_step_batch", "avm_set_relo_frame_batch", "avm_relo_resolve_batch", "avm_relo_finish_batch", "avm_prior_keep_batch")
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "relo.npz")


# ---------------------------------------------------------------- the statements
def headers_step_statement(stamps, flag=None, new_stamp=None):
    """stamps: the 11 Headers[i].stamp.toSec() of one window; returns the new list"""
    h = list(stamps)
    if flag == OLD:
        for i in range(WINDOW_SIZE):
            h[i] = h[i + 1]
        h[WINDOW_SIZE] = h[WINDOW_SIZE - 1]
    elif flag == SECOND_NEW:
        h[WINDOW_SIZE - 1] = h[WINDOW_SIZE]
    else:
        assert flag is None
    if new_stamp is not None:
        h[WINDOW_SIZE] = new_stamp
    return h


def set_relo_frame_statement(state, stamps, poses, msg):
    """state: dict(relocalization_info, relo_frame, relo_stamp, match_points [(id, x, y)], prev_relo_t, prev_relo_q, relo_pose) of one
    window, changed in place; msg: None or dict(frame_stamp, matches, prev_relo_t, prev_relo_q); poses [11][7]."""
    if msg is None:
        return state
    state["relo_stamp"] = msg["frame_stamp"]
    state["match_points"] = [tuple(m) for m in msg["matches"]]
    state["prev_relo_t"], state["prev_relo_q"] = list(msg["prev_relo_t"]), list(msg["prev_relo_q"])
    for i in range(WINDOW_SIZE):
        if state["relo_stamp"] == stamps[i]:
            state["relo_frame"], state["relocalization_info"] = i, 1
            state["relo_pose"] = [float(x) for x in poses[i]]
    return state


def resolve_statement(feats, relo_frame, match_points):
    """feats: the whole f_manager.feature list (dicts with id, start, obs).  Returns (relo_feat, relo_xy): the feature_index - the
    position among the rows the solve takes - and match point of every factor, in order."""
    relo_feat, relo_xy = [], []
    retrive_feature_index, feature_index = 0, -1
    for f in feats:
        if not (len(f["obs"]) >= 2 and f["start"] < WINDOW_SIZE - 2):
            continue
        feature_index += 1
        if f["start"] <= relo_frame:
            while retrive_feature_index < len(match_points) and int(match_points[retrive_feature_index][0]) < f["id"]:
                retrive_feature_index += 1
            if retrive_feature_index < len(match_points) and int(match_points[retrive_feature_index][0]) == f["id"]:
                relo_feat.append(feature_index)
                relo_xy.append(tuple(match_points[retrive_feature_index][1:3]))
                retrive_feature_index += 1
    return relo_feat, relo_xy


def prior_keep_statement(slot, prior):
    """slot / prior: dicts n, nblk, blk_kind [max_pblk], blk_frame, J [max_prior, max_prior], r, x0 [max_pblk, 9] of one window, each
    with strides of its own; the slot is changed in place when its n < 0."""
    if slot["n"] >= 0:
        return slot
    n, nb = int(prior["n"]), int(prior["nblk"])
    slot["n"], slot["nblk"] = n, nb
    for k in ("blk_kind", "blk_frame", "x0"):
        slot[k][:nb] = prior[k][:nb]
    slot["J"][:n, :n] = prior["J"][:n, :n]
    slot["r"][:n] = prior["r"][:n]
    return slot


# ---------------------------------------------------------------- header and prototypes
def test_header_declares_the_five_entry_points_and_keeps_the_abi():
    for name in RELO_ENTRY_POINTS:
        assert _header_arg_count(name) > 0
    h = _header()
    assert "#define AVM_ABI_VERSION 6 " in h and abi.AVM_ABI_VERSION == 6
    assert "typedef struct avm_relo_msg_batch {" in h and "typedef struct avm_relo_state {" in h


def test_relo_prototypes_match_the_headers_argument_counts():
    for name in RELO_ENTRY_POINTS:
        assert len(abi.PROTOTYPES[name][1]) == _header_arg_count(name), name
        assert re.fullmatch(r"avm_[a-z_]+", name)
    lib_m = importlib.import_module("anticipated-vins-mono_amd.lib")
    assert set(RELO_ENTRY_POINTS) <= set(lib_m.EXPORTS)
    L = lib_m.lib()                                                       # (loads without a GPU)
    out = (C.c_int * 8)()
    n = L.avm_debug_relo_struct_sizes(out)
    M, S = abi.ReloMsgBatch, abi.ReloState
    assert [out[i] for i in range(n)] == [C.sizeof(M), C.sizeof(S), M.has_msg.offset, M.prev_relo_q.offset, S.relocalization_info.offset,
                                          S.relo_relative_yaw.offset]
    out16 = (C.c_int * 16)()
    assert L.avm_debug_struct_sizes(out16) == 7 and L.avm_debug_track_struct_sizes(out16) == 8   # the older hooks keep their entries


# ---------------------------------------------------------------- the statements on hand-computed cases
STAMPS = [float(10 + i) for i in range(11)]


def test_headers_step_statement():
    assert headers_step_statement(STAMPS, OLD) == [11.0, 12.0, 13.0, 14.0, 15.0, 16.0, 17.0, 18.0, 19.0, 20.0, 20.0]
    assert headers_step_statement(STAMPS, SECOND_NEW) == STAMPS[:9] + [20.0, 20.0]
    assert headers_step_statement(STAMPS, None, 33.0) == STAMPS[:10] + [33.0]
    assert headers_step_statement(STAMPS, OLD, 33.0) == [float(11 + i) for i in range(10)] + [33.0]
    assert headers_step_statement(STAMPS) == STAMPS


def _blank_state():
    return dict(relocalization_info=0, relo_frame=0, relo_stamp=0.0, match_points=[], prev_relo_t=[0.0] * 3, prev_relo_q=[0.0, 0.0, 0.0, 1.0],
                relo_pose=[0.0] * 6 + [1.0])


def test_set_relo_frame_statement():
    poses = [[float(i)] * 3 + [0.0, 0.0, 0.0, 1.0] for i in range(11)]
    msg = dict(frame_stamp=14.0, matches=[(3, 0.1, 0.2), (9, 0.3, 0.4)], prev_relo_t=[1.0, 2.0, 3.0], prev_relo_q=[0.0, 0.0, 1.0, 0.0])
    s = set_relo_frame_statement(_blank_state(), STAMPS, poses, msg)
    assert (s["relocalization_info"], s["relo_frame"], s["relo_stamp"]) == (1, 4, 14.0) and s["relo_pose"] == poses[4]
    assert s["match_points"] == msg["matches"] and s["prev_relo_t"] == [1.0, 2.0, 3.0] and s["prev_relo_q"] == [0.0, 0.0, 1.0, 0.0]
    # a stamp occurring at two indices takes the later one (MARGIN_SECOND_NEW leaves Headers[9] == Headers[10]; here frames 2 and 7)
    twice = list(STAMPS)
    twice[7] = twice[2]
    s = set_relo_frame_statement(_blank_state(), twice, poses, dict(msg, frame_stamp=12.0))
    assert (s["relocalization_info"], s["relo_frame"]) == (1, 7) and s["relo_pose"] == poses[7]
    # a stamp equal to Headers[10] alone yields no match; the message is stored all the same
    s = set_relo_frame_statement(_blank_state(), STAMPS, poses, dict(msg, frame_stamp=20.0))
    assert (s["relocalization_info"], s["relo_frame"], s["relo_stamp"]) == (0, 0, 20.0) and s["relo_pose"] == [0.0] * 6 + [1.0]
    assert s["match_points"] == msg["matches"]
    # no message: untouched
    assert set_relo_frame_statement(_blank_state(), STAMPS, poses, None) == _blank_state()


def _feat(fid, start, nobs):
    return dict(id=fid, start=start, obs=[(0.0, 0.0)] * nobs, inv_depth=0.5)


def test_resolve_statement():
    # list positions:     0            1            2 (one obs)  3            4 (start 8)  5            6
    feats = [_feat(5, 0, 4), _feat(8, 0, 9), _feat(9, 1, 1), _feat(12, 2, 5), _feat(13, 8, 3), _feat(20, 6, 4), _feat(31, 7, 3)]
    # the solve's rows: ids 5, 8, 12, 20, 31 -> feature_index 0 .. 4 (ids 9 and 13 are dropped by the view's filter)
    m = [(2, 0.2, 0.2), (8, 0.8, 0.8), (9, 0.9, 0.9), (12, 1.2, 1.2), (20, 2.0, 2.0), (25, 2.5, 2.5)]
    assert resolve_statement(feats, 9, m) == ([1, 2, 3], [(0.8, 0.8), (1.2, 1.2), (2.0, 2.0)])
    # a matched id whose track starts after relo_frame yields no factor (id 20 starts in frame 6)
    assert resolve_statement(feats, 5, m) == ([1, 2], [(0.8, 0.8), (1.2, 1.2)])
    assert resolve_statement(feats, 0, m) == ([1], [(0.8, 0.8)])
    # an id dropped by the view's filter is no factor although it is among the matches (id 9), nor does it take a feature_index
    assert resolve_statement(feats, 9, [(9, 0.9, 0.9), (13, 1.3, 1.3)]) == ([], [])
    # a list id above every match id: the matches simply end (the reference would read past match_points)
    assert resolve_statement(feats, 9, [(5, 0.5, 0.5)]) == ([0], [(0.5, 0.5)])
    assert resolve_statement(feats, 9, [(1, 0.1, 0.1), (2, 0.2, 0.2)]) == ([], [])
    # zero matches; an empty list
    assert resolve_statement(feats, 9, []) == ([], []) and resolve_statement([], 3, m) == ([], [])
    # identical to the list
    assert resolve_statement(feats, 9, [(f["id"], 0.0, 1.0) for f in feats])[0] == [0, 1, 2, 3, 4]


def _prior(n, nblk, max_prior, max_pblk, base):
    return dict(n=n, nblk=nblk, blk_kind=np.arange(max_pblk, dtype=np.int32) + base, blk_frame=np.arange(max_pblk, dtype=np.int32) + 2 * base,
                J=np.arange(max_prior * max_prior, dtype=float).reshape(max_prior, max_prior) + base, r=np.arange(max_prior, dtype=float) - base,
                x0=np.arange(max_pblk * 9, dtype=float).reshape(max_pblk, 9) * base)


def test_prior_keep_statement():
    prior = _prior(3, 2, 5, 4, 100)
    slot = prior_keep_statement(_prior(-1, 7, 4, 3, 1), prior)
    assert (slot["n"], slot["nblk"]) == (3, 2)
    assert slot["blk_kind"].tolist() == [100, 101, 3] and slot["blk_frame"].tolist() == [200, 201, 4]
    assert slot["J"].tolist() == [[100, 101, 102, 4], [105, 106, 107, 8], [110, 111, 112, 12], [13, 14, 15, 16]]
    assert slot["r"].tolist() == [-100, -99, -98, 2] and np.array_equal(slot["x0"][:2], prior["x0"][:2]) and slot["x0"][2].tolist() == list(range(18, 27))
    kept = prior_keep_statement(_prior(0, 7, 4, 3, 1), prior)              # n >= 0: the marginalization's own result stays
    assert kept["n"] == 0 and np.array_equal(kept["J"], _prior(0, 7, 4, 3, 1)["J"])
    none = prior_keep_statement(_prior(-1, 7, 4, 3, 1), _prior(0, 0, 5, 4, 100))   # kept "no prior": counts only
    assert (none["n"], none["nblk"]) == (0, 0) and np.array_equal(none["J"], _prior(0, 7, 4, 3, 1)["J"])


# ---------------------------------------------------------------- the fixture of avm_relo_finish_batch
def test_golden_fixture_against_its_fp64_statement():
    gold = np.load(GOLD)
    N = gold["relo_pose"].shape[0]
    assert N >= 24
    wraps = 0
    for k in range(N):
        args = [gold[key][k] for key in ("relo_pose", "frame_pose", "prev_relo_t", "prev_relo_q")]
        f = GEN.finish_statement(*args)
        assert all(abs(abs(float(v)) - 180) >= 1 for v in f["_yaws"] + [f["drift_correct_yaw"][0], f["_rel_yaw_raw"]]), k
        assert all(abs(float(v)) <= 80 for v in f["_pitches"]), k
        wraps += abs(float(f["_rel_yaw_raw"])) > 180
        scale = max(1.0, max(np.abs(a).max() for a in args))
        for q in GEN.QUANTITIES:
            d, e = GEN.distance(q, [float(v) for v in f[q]], gold["m_" + q][k], scale), float(gold["err_fp64_" + q][k])
            assert d <= e + 4e-16, (k, q, d, e)                            # (the stored 50-digit values are rounded to double: half an ulp of 360 deg / 180)
    assert wraps >= 2
    for q in GEN.QUANTITIES:
        assert 0 < gold["err_fp64_" + q].max() < 1e-14, q
    assert np.abs(gold["relo_pose"][:, :3]).max() > 5.0                     # positions up to about 10 m
