"""TEST INFRASTRUCTURE shared by the tests of avm_global_sfm_batch: the fixture tests/golden/global_sfm.npz as batches of the ABI's
tables, the generator's own distance, and the bound the issue sets - 100 x the largest err_fp64_<quantity> over the fixture's cases."""
import os
import sys

import numpy as np

from conftest import mod

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_global_sfm as GEN  # noqa: E402

NAMES = [c[0] for c in GEN.CASES]
SENTINEL = -7.25  # what the tests put into every output row: a row the call must not write still holds it
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(os.path.join(HERE, "golden", "global_sfm.npz")))
    return _gold


def case_input(ci):
    g = gold()
    p = "c%d_in_" % ci
    return {k[len(p):]: g[k] for k in g if k.startswith(p)}


def bounds():
    """per quantity: 100 x the FP64 numpy run's own worst distance from the 50-digit run over the fixture's cases"""
    g = gold()
    return {q: 100 * max(float(g[k]) for k in g if k.endswith("_err_fp64_" + q)) for q in GEN.QUANTITIES}


def distance(q, a, b):
    """the generator's: max |a - b| / max |b|, q and -q one rotation"""
    a, b = np.asarray(a, float), np.asarray(b, float)
    big = np.abs(b).max()
    if q in ("q", "pnp_q"):
        a, b = a.reshape(-1, 4), b.reshape(-1, 4)
        return float(np.minimum(np.abs(a - b).max(axis=1), np.abs(a + b).max(axis=1)).max() / big)
    return float(np.abs(a - b).max() / big)


def batch(inputs, max_frames=None, max_feat=None, max_obs=None, max_pts=None, max_it=None):
    """Stacks run() inputs (dicts as case_input gives them) to common strides: (SfmBatchArrays, WindowArrays, feat_id [B, max_feat]).
    max_it: the batch's ba_max_num_iterations (None: the inputs' own, which must then agree)."""
    ib, buffers = mod("init_buffers"), mod("buffers")
    B = len(inputs)
    MF = max_frames or max(i["frame_n_pts"].shape[0] for i in inputs)
    MP = max_pts or max(i["frame_pt_id"].shape[1] for i in inputs)
    MFE = max_feat or max(i["feat_start"].shape[0] for i in inputs)
    MO = max_obs or max(i["obs_xy"].shape[0] for i in inputs)
    s = {"l": np.zeros(B, np.int32), "relative_R": np.zeros((B, 9)), "relative_T": np.zeros((B, 3)), "n_frames": np.zeros(B, np.int32),
         "key_index": np.zeros((B, 11), np.int32), "frame_n_pts": np.zeros((B, MF), np.int32), "frame_pt_id": np.zeros((B, MF, MP), np.int32),
         "frame_pt_xy": np.zeros((B, MF, MP, 2))}
    w = {"n_feat": np.zeros(B, np.int32), "feat_start": np.zeros((B, MFE), np.int32), "feat_nobs": np.zeros((B, MFE), np.int32),
         "feat_obs_begin": np.zeros((B, MFE), np.int32), "obs_xy": np.zeros((B, MO, 2)), "ex_pose": np.zeros((B, 7))}
    fid = np.zeros((B, MFE), np.int32)
    its = {max_it} if max_it else {int(i["ba_max_num_iterations"]) for i in inputs}
    for b, i in enumerate(inputs):
        for k in ("l", "n_frames", "relative_R", "relative_T", "key_index"):
            s[k][b] = i[k]
        F, P = i["frame_pt_id"].shape
        s["frame_n_pts"][b, :F] = i["frame_n_pts"]
        s["frame_pt_id"][b, :F, :P] = i["frame_pt_id"]
        s["frame_pt_xy"][b, :F, :P] = i["frame_pt_xy"]
        n = i["feat_start"].shape[0]
        w["n_feat"][b], w["ex_pose"][b] = i["n_feat"], i["ex_pose"]
        for k in ("feat_start", "feat_nobs", "feat_obs_begin"):
            w[k][b, :n] = i[k]
        w["obs_xy"][b, : i["obs_xy"].shape[0]] = i["obs_xy"]
        fid[b, :n] = i["feat_id"]
    assert len(its) == 1, "one ba_max_num_iterations per batch"
    sfm = ib.SfmBatchArrays(dict(n_windows=B, max_frames=MF, max_pts=MP, ba_max_num_iterations=its.pop(), ba_max_solver_time_s=0.0), s)
    win = buffers.WindowArrays(dict(n_windows=B, max_feat=MFE, max_obs=MO, max_samp=0, max_prior=0, max_pblk=0), w)
    return sfm, win, fid


def out_alloc(sfm, win, device=None):
    o = mod("init_buffers").SfmOutArrays.alloc(sfm.n_windows, sfm.dims["max_frames"], win.dims["max_feat"], fill=SENTINEL)
    o.a["ok"][:], o.a["point_state"][:], o.a["ba_counts"][:] = -7, -7, -7
    return o.to_device(device) if device else o


def expected_written(ok):
    """which outputs a stream with this ok writes (include/avm_init.h)"""
    w = {"ok"}
    if ok != 4 and ok != 1:
        w |= {"pnp_q", "pnp_t", "ba_counts", "ba_cost"}
    if ok in (0, 3):
        w |= {"q", "T", "point", "point_state"}
    if ok == 0:
        w |= {"frame_R", "frame_T"}
    return w


def check_stream(o, b, inp, ref, ref_prefix, bound, measured=None):
    """Output row b of the host arrays `o` against a reference dict: ok, point_state, ba_counts exactly; every stored quantity within
    `bound` (every figure is printed before anything is asserted); every row the contract leaves unwritten still the sentinel.  With a key
    "ba_cost0" in `bound` the initial cost is held to that and the final cost to bound["ba_cost"], else the pair to bound["ba_cost"].  ref_prefix: 'm_' (the fixture's 50-digit run) or '' (a live
    FP64 run's result dict).  measured: dict quantity -> largest distance seen, updated."""
    ok = int(ref["ok"])
    assert int(o["ok"][b]) == ok, (int(o["ok"][b]), ok)
    wr = expected_written(ok)
    nf, F = int(inp["n_feat"]), int(inp["n_frames"])
    rows = {"point": nf, "point_state": nf, "frame_R": F, "frame_T": F}
    missed = []
    for k, v in o.items():
        if k == "ok":
            continue
        sent = -7 if v.dtype == np.int32 else SENTINEL
        if k not in wr:
            assert (v[b] == sent).all(), (k, "written though ok = %d" % ok)
            continue
        n = rows.get(k, v[b].shape[0])
        assert (v[b][n:] == sent).all(), (k, "rows beyond the stream's own were written")
        got = v[b][:n]
        if k in ("point_state", "ba_counts"):
            np.testing.assert_array_equal(got, np.asarray(ref[k])[:n], err_msg=k)
            continue
        want = np.asarray(ref[ref_prefix + k], float)
        want = want.reshape((-1,) + got.shape[1:])[:n] if got.ndim > 1 else want
        parts = [(k, got, want, bound[k])]
        if k == "ba_cost" and "ba_cost0" in bound:
            parts = [("ba_cost0", got[:1], want[:1], bound["ba_cost0"]), ("ba_cost", got[1:], want[1:], bound["ba_cost"])]
        for name, a, r, bd in parts:
            d = distance(k, a, r)
            if measured is not None:
                measured[name] = max(measured.get(name, 0.0), d)
            print("%-8s distance %.2e  bound %.2e" % (name, d, bd))
            if not d <= bd:
                missed.append((name, d, bd))
    assert not missed, missed
