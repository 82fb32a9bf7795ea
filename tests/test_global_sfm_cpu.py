"""The reference statement of GlobalSFM::construct and of the PnP of every frame (tests/golden/gen_global_sfm.py) and its fixture
tests/golden/global_sfm.npz: the FP64 half regenerates bit for bit, the stored inputs are synth.make_sfm's, the fixture holds the cases
a device implementation has to be checked on, and the statement recovers the true trajectory."""
import os
import sys

import numpy as np

from conftest import mod

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_global_sfm as GEN  # noqa: E402


def _gold():
    return np.load(os.path.join(HERE, "golden", "global_sfm.npz"))


def test_fp64_part_of_the_fixture_regenerates():
    """(the stored inputs are make_sfm's: fp64_part() calls it again)"""
    gold = _gold()
    again, _ = GEN.fp64_part()
    for k, v in again.items():
        assert k in gold.files, k
        np.testing.assert_array_equal(gold[k], v, err_msg=k)
    rest = set(gold.files) - set(again)
    assert rest and all("_m_" in k or "_err_fp64_" in k for k in rest), sorted(rest)[:5]  # the 50-digit half


def test_fixture_covers_the_issue_s_cases():
    gold = _gold()
    assert [int(gold["c%d_ok" % ci]) for ci in range(len(GEN.CASES))] == [0, 0, 0, 0, 0, 0, 1, 2, 3, 4]
    by = {c[0]: ci for ci, c in enumerate(GEN.CASES)}
    p = lambda n, k: gold["c%d_%s" % (by[n], k)]
    # 24 full-length tracks, l = 0; 40 tracks, at most 20 reach back to frames 0 - 2 and at least 24 span 3 - 10, l = 3
    assert int(p("t24_l0", "in_n_feat")) == 24 and (p("t24_l0", "in_feat_nobs")[:24] == 11).all() and int(p("t24_l0", "in_l")) == 0
    st, no = p("t40_l3", "in_feat_start")[:40], p("t40_l3", "in_feat_nobs")[:40]
    assert int(p("t40_l3", "in_n_feat")) == 40 and int(p("t40_l3", "in_l")) == 3
    assert (st <= 2).sum() <= 20 and ((st <= 3) & (st + no == 11)).sum() >= 24 + 11
    assert ((st + no <= 3)).sum() >= 1 and (no == 1).sum() == 1        # step-5 leftovers; a row that stays untriangulated
    assert p("t40_l3", "point_state").tolist() == (no >= 2).astype(int).tolist()
    # non-key frames, irregular key_index; the wide stride
    assert int(p("t64_f16", "in_n_frames")) == 16 and int(p("t64_f33", "in_n_frames")) == 33 and int(p("t64_f16", "in_n_feat")) == 64
    assert (np.diff(p("t64_f33", "in_key_index")) > 1).any() and (np.diff(p("t64_f33", "in_key_index")) == 1).any()
    assert int(p("t384_wide", "in_n_feat")) == 384 > mod("abi").MAX_FEAT
    # the failures, each met by count or by construction
    assert int(p("fail_ba_it1", "in_ba_max_num_iterations")) == 1 and p("fail_ba_it1", "ba_counts").tolist() == [1, 1, 0]
    assert float(p("fail_ba_it1", "f_ba_cost")[1]) > 5e-3 and float(p("t64_px15", "f_ba_cost")[1]) > 5e-3  # (accepted by convergence alone)
    assert np.isnan(p("fail_nan", "in_relative_T")).sum() == 1
    sf = p("fail_frame5", "in_frame_n_pts")
    k = int(np.flatnonzero(sf)[0])
    known = np.isin(p("fail_frame5", "in_frame_pt_id")[k, : sf[k]], p("fail_frame5", "in_feat_id")[:64])
    assert known.sum() == 5 and sf[k] > 5
    # every BA of an ok case converges on function_tolerance with no rejected step, every decision away from rounding
    for ci, c in enumerate(GEN.CASES):
        if c[9] == 0:
            it, good, term = gold["c%d_ba_counts" % ci].tolist()
            assert term == 3 and good == it - 1 and 3 <= it <= 12, c[0]
        for k in gold.files:
            if k.startswith("c%d_min_margin_" % ci) and not k.endswith(("noise_tests", "noise_step")):
                assert float(gold[k]) > (GEN.PNP_SURE if k.endswith("pnp_reject") else 1e-6), k
        if "c%d_min_margin_noise_step" % ci in gold.files:
            assert float(gold["c%d_min_margin_noise_step" % ci]) < GEN.FLT_EPSILON


def test_statement_recovers_the_true_trajectory():
    """Up to the similarity fixed by frames l and 10.  The numpy run shows, over the six ok cases: rotations within 0.07 - 0.20 degrees,
    positions within 0.5 - 1.2 % of the l - 10 baseline (0.5 px of noise, 1.5 px in t64_px15; relativePose's own 0.05 degrees / 0.5 %).
    The bounds are twice the worst of them."""
    gold = _gold()
    seen = []
    for ci, c in enumerate(GEN.CASES):
        if c[9] != 0:
            continue
        inp = {k[len("c%d_in_" % ci):]: gold[k] for k in gold.files if k.startswith("c%d_in_" % ci)}
        rot, pos = GEN.similarity_error(inp, gold["c%d_f_q" % ci], gold["c%d_f_T" % ci])
        seen.append((c[0], round(float(rot), 3), round(float(pos), 4)))
        assert rot < 0.40 and pos < 0.024, seen[-1]
    print(seen)
