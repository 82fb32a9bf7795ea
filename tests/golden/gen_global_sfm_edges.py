"""TEST INFRASTRUCTURE.  Generates tests/golden/global_sfm_edges.npz: a second case list for gen_global_sfm.py's statement (imported,
both backends, every assertion of that generator; the same keys per case), at the shapes where what only the device has goes wrong:

  name        tracks (start, length, count)                     nf   l  frames      what it reaches
  e_l9_nf33   (0,11,33)                                          33   9  11          tail of 1; nine backward PnPs; constant frame next to 10
  e_l5_nf47   (0,11,25) (2,7,11) (5,6,11)                        47   5  11          tail of 15; both chains non-trivial
  e_nf257     (0,11,40) (0,5,100) (4,7,117)                     257   2  16 IRR16    one row past the 256-thread stride; 17 chunks, the last
                                                                                     with one point; frames listing more than 64 points
  e_holes64   (0,11,30) (2,1,5) (4,6,14) (7,1,3) (8,3,12)        64   0  11          state == 0 rows inside chunks 1, 2 and 3; full last chunk
  e_cnt10     (0,11,10) (1,10,20)                                30   0  11          frame 1's chain PnP on exactly 10 points
  e_frame6    T64                                                64   0  16 IRR16    hook "frame6": fail_frame5's frame keeps 6 known points
  e_lanes     T64F                                               64   0  16 IRR16    hook "npts64_65": frames 2 and 5 list 64 and 65 points
  e_f64       T64                                                64   4  64 KEY64    the largest n_frames: 53 frame PnPs; two adjacent keys,
                                                                                     a gap of 21 frames

Noise 0.5 px, ba_max_num_iterations 50, ok = 0 everywhere.  No count was changed.  first_id is the case's position in the
list, except where an assertion forced another:
  e_f64     7: an accept test of a frame's PnP has a margin of 4e-13 on a step of 1.3e-7 |param| > FLT_EPSILON |param| (check_trace refuses);
            8: err_fp64 of ba_cost 9.6e-10 against the cap of 1.2e-12 below; 9 is e_cnt10's; 10 passes
  e_cnt10   4: err_fp64 of ba_cost 3.5e-10 against the cap; 9 passes
  e_frame6  5: err_fp64 of ba_cost 8.3e-10 against the cap; 9 is e_cnt10's, 10 misses too (1.9e-10); 11 passes
(where the FP64 run takes an accept test inside rounding noise the other way than the 50-digit run, its chain is off by 1e-10 and the
BA's initial cost with it: DESIGN.md 2.24.)
e_cnt10 has 10 pairs between frames l and 10, as fail_pnp9 has 9: with l = 0 every point of frame 1's PnP is such a pair, so the
generator's "more than 20" (a condition of relativePose, which is not part of this entry point) is waived for it here as the generator
waives it for fail_pnp9: check_trace() sees e_cnt10's trace without that one count, after it was asserted to be 10.

gen_global_sfm.py is used as it stands: its run(), Trace, fp64_part() and main() with all their assertions work on this module's CASES,
OUT, case_inputs() and check_trace() (the four names are set in that module before main() is called), so the comparison of the two runs is
written once.  The two hooks live here, next to the copy of what "frame5" does: "frame6" and "npts64_65".

Two conditions beyond the generator's own, on the inputs: every case ends with ok = 0 and the same ba_counts in both runs (main()
asserts the equality), and its err_fp64 is, per quantity, at most 10 x the largest err_fp64 of that quantity in global_sfm.npz - a case
that misses it gets another first_id.

    python tests/golden/gen_global_sfm_edges.py          (FP64 and 50 digits: 122 s of wall time)
    GEN_SFM_PROBE=1 python tests/golden/gen_global_sfm_edges.py     (the FP64 run alone, with its margins and counts)
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_global_sfm as GEN  # noqa: E402

OUT = os.path.join(HERE, "global_sfm_edges.npz")
KEY64 = [0, 1, 5, 9, 14, 18, 39, 44, 50, 57, 63]
# name, first_id, tracks, n_frames, key_index, l, noise_px, ba_max_num_iterations, hook, the ok it must end with
CASES = [
    ("e_l9_nf33", 0, [(0, 11, 33)], 11, None, 9, 0.5, 50, None, 0),
    ("e_l5_nf47", 1, [(0, 11, 25), (2, 7, 11), (5, 6, 11)], 11, None, 5, 0.5, 50, None, 0),
    ("e_nf257", 2, [(0, 11, 40), (0, 5, 100), (4, 7, 117)], 16, GEN.IRR16, 2, 0.5, 50, None, 0),
    ("e_holes64", 3, [(0, 11, 30), (2, 1, 5), (4, 6, 14), (7, 1, 3), (8, 3, 12)], 11, None, 0, 0.5, 50, None, 0),
    ("e_cnt10", 9, [(0, 11, 10), (1, 10, 20)], 11, None, 0, 0.5, 50, None, 0),
    ("e_frame6", 11, GEN.T64, 16, GEN.IRR16, 0, 0.5, 50, "frame6", 0),
    ("e_lanes", 6, GEN.T64F, 16, GEN.IRR16, 0, 0.5, 50, "npts64_65", 0),
    ("e_f64", 10, GEN.T64, 64, KEY64, 4, 0.5, 50, None, 0),
]
FACTOR = 10  # a case's err_fp64 against the largest of global_sfm.npz
_statement_inputs, _statement_check = GEN.case_inputs, GEN.check_trace


def set_frame(sf, k, ids, xy):
    sf.a["frame_n_pts"][0, k] = len(ids)
    sf.a["frame_pt_id"][0, k], sf.a["frame_pt_xy"][0, k] = 0, 0
    sf.a["frame_pt_id"][0, k, : len(ids)], sf.a["frame_pt_xy"][0, k, : len(ids)] = ids, xy


def hook_frame6(sf, known_ids):
    """what "frame5" does, with 6: the first non-key frame keeps 6 ids the SfM knows and the ids it does not"""
    k = int(np.flatnonzero(sf.a["frame_n_pts"][0])[0])
    n = int(sf.a["frame_n_pts"][0, k])
    ids, xy = sf.a["frame_pt_id"][0, k, :n].copy(), sf.a["frame_pt_xy"][0, k, :n].copy()
    kn = np.isin(ids, known_ids)
    keep = sorted(list(np.flatnonzero(kn)[:6]) + list(np.flatnonzero(~kn)))
    set_frame(sf, k, ids[keep], xy[keep])


def hook_npts64_65(sf, known_ids):
    """the first two non-key frames list exactly 64 and 65 points: ids no track has (1, 2, ... < 7, the smallest track id) in front, then
    the LAST 63 (64) of the frame's ids the SfM knows - so that the last listed point, n = 63 (64), counts"""
    for k, total in zip(np.flatnonzero(sf.a["frame_n_pts"][0])[:2], (64, 65)):
        n = int(sf.a["frame_n_pts"][0, k])
        ids, xy = sf.a["frame_pt_id"][0, k, :n].copy(), sf.a["frame_pt_xy"][0, k, :n].copy()
        kn = np.flatnonzero(np.isin(ids, known_ids))[-(total - 1):]
        pad = total - len(kn)
        assert 1 <= pad <= 6 and total <= sf.a["frame_pt_id"].shape[2] and known_ids.min() == 7, (k, total, len(kn))
        set_frame(sf, k, np.concatenate([np.arange(1, pad + 1), ids[kn]]), np.concatenate([xy[n - pad :], xy[kn]]))


HOOKS = {"frame6": hook_frame6, "npts64_65": hook_npts64_65}


def case_inputs(case):
    """the statement's case_inputs (which knows none of the hooks here and leaves the tables as make_sfm made them), then the hook"""
    inp, objs = _statement_inputs(case)
    if case[8]:
        sf, win, feat_id = objs[:3]
        HOOKS[case[8]](sf, feat_id[0, : win.a["n_feat"][0]])
        for k in ("frame_n_pts", "frame_pt_id", "frame_pt_xy"):
            inp[k] = sf.a[k][0]
    return inp, objs


def check_trace(name, tr):
    if name == "e_cnt10":
        assert ("corres_l_10", 10) in tr.counts
        seen, tr = tr, GEN.Trace()
        tr.dec, tr.f32, tr.counts = seen.dec, seen.f32, [c for c in seen.counts if c[0] != "corres_l_10"]
    return _statement_check(name, tr)


def accept(out):
    base = dict(np.load(os.path.join(HERE, "global_sfm.npz")))
    for q in GEN.QUANTITIES:
        cap = FACTOR * max(float(base[k]) for k in base if k.endswith("_err_fp64_" + q))
        for ci, case in enumerate(CASES):
            e = float(out["c%d_err_fp64_%s" % (ci, q)])
            assert e <= cap, (case[0], q, e, cap, "another first_id")
    for ci, case in enumerate(CASES):
        assert int(out["c%d_ok" % ci]) == case[9] == 0, case[0]
        print(case[0], "ba_counts", out["c%d_ba_counts" % ci].tolist())


if __name__ == "__main__":
    GEN.CASES, GEN.case_inputs, GEN.check_trace = CASES, case_inputs, check_trace
    if os.environ.get("GEN_SFM_PROBE"):
        GEN.fp64_part()
    else:
        t0 = time.time()
        GEN.OUT = OUT + ".unchecked.npz"  # main() writes; the file takes its name once the two conditions hold
        GEN.main()
        accept(dict(np.load(GEN.OUT)))
        os.replace(GEN.OUT, OUT)
        print("wrote", OUT, "wall time %.0f s" % (time.time() - t0))
