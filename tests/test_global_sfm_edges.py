"""avm_global_sfm_batch on the device at the shapes tests/golden/global_sfm.npz leaves out (tests/golden/global_sfm_edges.npz,
gen_global_sfm_edges.py): chunk tails of 1 and 15 points, a table one row longer than the team, state == 0 rows inside chunks, l = 2, 4, 5
and 9, a chain PnP on exactly 10 and a frame's PnP on exactly 6 points, frames listing 64 and 65 points, 64 frames.

Exact: ok, point_state, ba_counts.  Every quantity: the generator's distance from the 50-digit result, bound = 100 x the largest
err_fp64_<quantity> over the cases of both fixtures (sfm_edge_cases.edge_bounds()); `point` per row as well for the cases with a chunk tail or
holes.  Batches: every row byte-identical to its B = 1 run, whatever its neighbours, position, strides and memory mode.

  name        tracks (start, length, count)                  nf   l  frames    what it reaches
  e_l9_nf33   (0,11,33)                                       33   9  11        chunk tail of 1; nine backward PnPs; constant frame next to 10
  e_l5_nf47   (0,11,25) (2,7,11) (5,6,11)                     47   5  11        chunk tail of 15; both chains non-trivial
  e_nf257     (0,11,40) (0,5,100) (4,7,117)                  257   2  16 IRR16  one row past the 256-thread stride; 17 chunks; frames of > 64 points
  e_holes64   (0,11,30) (2,1,5) (4,6,14) (7,1,3) (8,3,12)     64   0  11        state == 0 rows 30..34 and 49..51: inside chunks 1, 2 and 3
  e_cnt10     (0,11,10) (1,10,20)                             30   0  11        frame 1's chain PnP on exactly 10 points
  e_frame6    T64, hook "frame6"                              64   0  16 IRR16  frame 2 keeps exactly 6 known points
  e_lanes     T64F, hook "npts64_65"                          64   0  16 IRR16  frames 2 and 5 list exactly 64 and 65 points, the last one known
  e_f64       T64                                             64   4  64 KEY64  53 non-key frames, two adjacent keys, a gap of 21 frames
Every BA ends on the function tolerance with no rejected step: ba_counts [6,5,3] [5,4,3] [5,4,3] [5,4,3] [6,5,3] [4,3,3] [3,2,3] [3,2,3].

Measured on an MI355X, B = 1 per case: the distance of the device result from the 50-digit result | the err_fp64 of that case
  case        pnp_q              pnp_t              q                  T                  point              frame_R            frame_T            ba_cost
  e_l9_nf33   2.1e-17 | 5.4e-17  3.3e-16 | 4.5e-16  3.3e-16 | 3.7e-16  4.4e-15 | 1.5e-14  6.0e-15 | 1.7e-14  1.4e-16 | 4.0e-16  4.4e-15 | 1.5e-14  8.5e-15 | 3.7e-15
  e_l5_nf47   1.9e-14 | 8.1e-15  2.7e-13 | 1.1e-13  4.4e-16 | 6.0e-16  6.3e-16 | 6.0e-16  8.4e-16 | 2.2e-15  1.5e-16 | 1.6e-16  6.3e-16 | 6.0e-16  1.0e-14 | 3.6e-13
  e_nf257     1.1e-14 | 1.1e-14  1.1e-13 | 1.1e-13  2.2e-16 | 2.8e-16  2.6e-16 | 2.5e-16  2.7e-15 | 2.1e-15  8.0e-11 | 3.5e-11  2.1e-10 | 1.9e-10  6.3e-15 | 1.4e-14
  e_holes64   1.1e-11 | 3.7e-13  1.1e-10 | 3.2e-12  8.3e-16 | 3.3e-16  1.7e-15 | 3.4e-16  1.8e-14 | 2.2e-15  1.7e-15 | 1.8e-16  1.7e-15 | 3.4e-16  1.6e-11 | 1.3e-13
  e_cnt10     1.0e-12 | 2.3e-11  7.7e-12 | 3.3e-10  2.2e-16 | 4.0e-16  5.4e-16 | 1.3e-15  2.2e-15 | 8.5e-15  1.9e-16 | 7.9e-16  5.4e-16 | 1.3e-15  1.5e-11 | 5.6e-15
  e_frame6    1.1e-16 | 8.4e-17  4.1e-16 | 5.8e-16  4.4e-16 | 2.4e-16  5.0e-16 | 9.1e-16  1.0e-15 | 2.0e-15  4.4e-16 | 6.4e-16  5.2e-16 | 9.1e-16  6.1e-15 | 5.0e-14
  e_lanes     7.8e-15 | 4.8e-15  3.1e-14 | 2.2e-14  2.2e-16 | 2.0e-16  3.5e-16 | 3.8e-16  8.6e-16 | 7.9e-16  4.0e-11 | 1.4e-14  1.2e-10 | 4.0e-14  3.0e-15 | 3.9e-15
  e_f64       9.9e-14 | 1.3e-15  3.8e-13 | 4.8e-15  2.2e-16 | 2.7e-16  5.4e-16 | 5.9e-16  5.8e-16 | 9.0e-16  1.5e-11 | 1.6e-11  1.8e-11 | 3.0e-11  3.4e-15 | 9.6e-14
  bound       2.8e-08            1.4e-07            3.5e-13            1.5e-12            4.4e-12            6.5e-09            2.1e-08            3.6e-11
Per row of `point`: worst row 23 of e_l9_nf33 (6.0e-15; its one-point tail, row 32: 1.4e-15), 46 of e_l5_nf47 (8.4e-16, the tail's last
slot), 236 of e_nf257 (2.7e-15; row 256: 7.1e-16), 61 of e_holes64 (1.8e-14).
The bounds of T and ba_cost are e_l9_nf33's and e_l5_nf47's err_fp64 x 100, 2.1 and 3.1 times sfm_cases.bounds(); the others are
unchanged.  The INITIAL BA cost of e_holes64 (chain at 1e-10: the size of a PnP accept test inside rounding noise that fell the other
way than in the 50-digit run) and of e_cnt10 is off by 1.6e-11 and 1.5e-11: within this bound, beyond the first fixture's 1.2e-11
(DESIGN.md 2.24.1).
"""
import numpy as np
import pytest

import sfm_cases as SC
import sfm_edge_cases as EC
import gen_global_sfm_edges as EDGES  # noqa: E402  (tests/golden: on the path through sfm_cases)
from conftest import mod
from test_global_sfm import same_rows

pytestmark = pytest.mark.gpu
CHUNK = 16
PER_POINT = ["e_l9_nf33", "e_l5_nf47", "e_nf257", "e_holes64"]


def names():
    return EC.edge_names()


def run(ctx, inputs, device=True, max_it=None, **strides):
    """One avm_global_sfm_batch call on the stacked inputs (strides: max_frames, max_feat, max_pts, max_obs of SC.batch); outputs start as
    sentinels.  Returns the outputs as host numpy arrays."""
    sfm, win, fid = SC.batch(inputs, max_it=max_it, **strides)
    out = SC.out_alloc(sfm, win)
    if device:
        sfm, win, out = sfm.to_device(), win.to_device(), out.to_device()
    mod("estimator").Estimator(ctx=ctx).globalSFM(sfm, win, fid, out=out)
    return out.to_host().a


@pytest.fixture(scope="module")
def solo(ctx):
    """the B = 1 result of every edge case, at the case's own strides (computed once, never changed)"""
    return {n: run(ctx, [EC.edge_input(n)]) for n in names()}


def same(batch_out, order, solos):
    """row b of the batch is the solo run of order[b], byte for byte, and its padding is unwritten"""
    for b, n in enumerate(order):
        try:
            same_rows({k: v[b : b + 1] for k, v in batch_out.items()}, [0], [solos[n]])
        except AssertionError as e:
            raise AssertionError("stream %d (%s): %s" % (b, n, e)) from None


@pytest.mark.parametrize("name", [c[0] for c in EDGES.CASES])
def test_solo_parity(solo, name):
    inp, ref, bound = EC.edge_input(name), EC.edge_ref(name), EC.edge_bounds()
    measured = {}
    try:
        SC.check_stream(solo[name], 0, inp, ref, "m_", bound, measured)
    finally:
        print(name, " ".join("%s %.1e | %.1e" % (q, measured.get(q, float("nan")), float(ref["err_fp64_" + q])) for q in SC.GEN.QUANTITIES))
    assert int(solo[name]["ok"][0]) == 0


@pytest.mark.parametrize("name", PER_POINT)
def test_points_row_by_row(solo, name):
    """the distance of `point` per feature: a wrong slot of the last chunk, or of a chunk with holes, is named"""
    inp, ref = EC.edge_input(name), EC.edge_ref(name)
    nf = int(inp["n_feat"])
    got, want = solo[name]["point"][0, :nf], np.asarray(ref["m_point"], float).reshape(-1, 3)[:nf]
    state = np.asarray(ref["point_state"])[:nf]
    d = np.abs(got - want).max(axis=1) / np.abs(want).max()
    j = int(np.argmax(d))
    bound = EC.edge_bounds()["point"]
    print("%s worst row %d (chunk %d, slot %d, state %d): %.2e  bound %.2e" % (name, j, j // CHUNK, j % CHUNK, state[j], d[j], bound))
    tail = slice(nf - (nf % CHUNK or CHUNK), nf)
    print("  last chunk rows %d..%d: worst %.2e" % (tail.start, nf - 1, d[tail].max()))
    bad = np.flatnonzero(~(d <= bound))
    assert bad.size == 0, [(int(r), int(r) // CHUNK, int(r) % CHUNK, float(d[r])) for r in bad]
    # a row no pair of frames triangulates is written as the statement stores it: zeros
    holes = np.flatnonzero(state == 0)
    assert (want[holes] == 0).all() and (got[holes] == 0).all(), holes[(got[holes] != 0).any(axis=1)]
    np.testing.assert_array_equal(solo[name]["point_state"][0, :nf], state)


@pytest.fixture(scope="module")
def eight():
    return [EC.edge_input(n) for n in names()]


@pytest.fixture(scope="module")
def eight_out(ctx, eight):
    return run(ctx, eight, max_frames=64, max_feat=257)


def test_batch_rows_are_the_solo_runs(ctx, eight, eight_out, solo):
    """ragged shapes at common strides (max_frames 64, max_feat 257, one max_pts), in fixture order and reversed"""
    assert eight_out["point"].shape[1] == 257 and eight_out["frame_R"].shape[1] == 64
    same(eight_out, names(), solo)
    same(run(ctx, eight[::-1], max_frames=64, max_feat=257), names()[::-1], solo)


def test_wider_strides_same_bytes(ctx, eight, solo):
    """max_feat 384 (the widest the ABI takes) and max_pts 7 beyond the longest frame list"""
    mp = max(i["frame_pt_id"].shape[1] for i in eight) + 7
    same(run(ctx, eight, max_frames=64, max_feat=384, max_pts=mp), names(), solo)


def test_host_and_device_memory_give_the_same_bytes(ctx, eight, eight_out):
    host = run(ctx, eight, device=False, max_frames=64, max_feat=257)
    for k in host:
        assert host[k].tobytes() == eight_out[k].tobytes(), k


def test_thresholds_from_both_sides(ctx, solo):
    """exactly 10 next to 9 points of a chain PnP, exactly 6 next to 5 of a frame's, in one batch"""
    order = ["e_cnt10", "fail_pnp9", "e_frame6", "fail_frame5"]
    inputs = {n: EC.edge_input(n) if n.startswith("e_") else SC.case_input(SC.NAMES.index(n)) for n in order}
    o = run(ctx, [inputs[n] for n in order], max_it=50)
    assert o["ok"].tolist() == [0, 1, 0, 3]
    alone = {n: solo[n] if n.startswith("e_") else run(ctx, [inputs[n]], max_it=50) for n in order}  # (the edge cases' own cap is 50)
    same(o, order, alone)
