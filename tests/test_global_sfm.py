"""The deterministic half of Estimator::initialStructure on the device (avm_global_sfm_batch, include/avm_init.h) against
tests/golden/global_sfm.npz: the numpy statement of gen_global_sfm.py and its 50-digit run.

Exact: ok, point_state, ba_counts.  Every quantity of pnp_q pnp_t q T point frame_R frame_T ba_cost: the generator's distance from the
50-digit result, bound = 100 x the largest err_fp64_<quantity> over the fixture's cases (sfm_cases.bounds()).

ba_max_num_iterations is one number per batch in the ABI: the batch of all ten cases runs at 50 and its rows are compared with B = 1 runs
at 50 (fail_ba_it1's row is then t64_px15's); the fixture's own cap of 1 is what the B = 1 run of that case uses.

Measured on an MI355X, B = 1 per case: the distance of the device result from the 50-digit result | the err_fp64 of that case
  case        pnp_q              pnp_t              q                  T                  point              frame_R            frame_T            ba_cost
  t24_l0      5.3e-11 | 2.2e-15  8.0e-10 | 1.6e-14  3.1e-15 | 3.6e-16  6.5e-15 | 4.2e-16  5.2e-14 | 2.6e-15  6.1e-15 | 3.5e-16  6.5e-15 | 4.2e-16  7.3e-14 | 9.0e-14
  t40_l3      1.8e-12 | 3.0e-14  2.9e-11 | 3.3e-13  2.2e-16 | 2.6e-16  4.3e-16 | 5.4e-16  4.6e-15 | 1.1e-15  2.1e-16 | 1.3e-16  4.3e-16 | 5.4e-16  2.4e-15 | 1.6e-14
  t64_f16     1.5e-15 | 9.3e-15  1.2e-14 | 6.6e-14  1.1e-16 | 2.3e-16  3.7e-16 | 1.7e-16  6.0e-16 | 1.3e-15  4.6e-11 | 6.5e-11  1.6e-10 | 2.1e-10  5.7e-15 | 1.6e-14
  t64_f33     7.1e-14 | 7.1e-14  1.5e-13 | 1.5e-13  2.2e-16 | 1.6e-16  1.4e-16 | 1.6e-16  3.3e-16 | 4.0e-16  1.5e-12 | 1.6e-11  2.1e-12 | 2.5e-11  3.6e-16 | 2.0e-14
  t384_wide   1.6e-13 | 1.1e-11  1.9e-12 | 1.8e-10  2.2e-16 | 2.8e-16  8.1e-16 | 8.6e-16  1.1e-14 | 1.2e-14  1.7e-16 | 5.5e-16  8.1e-16 | 8.6e-16  3.2e-15 | 1.2e-13
  t64_px15    2.5e-14 | 2.8e-10  1.3e-13 | 1.4e-09  1.1e-16 | 3.5e-15  2.2e-16 | 7.2e-15  4.6e-16 | 4.4e-14  1.7e-16 | 7.0e-15  2.2e-16 | 7.2e-15  1.2e-15 | 2.3e-14
  rejected step, against the live FP64 run:
              4.0e-16            4.6e-15            3.3e-16            6.6e-16            1.8e-15            2.2e-16            6.6e-16            6.8e-15
  bound       2.8e-08            1.4e-07            3.5e-13            7.2e-13            4.4e-12            6.5e-09            2.1e-08            1.2e-11
The failure cases' stages: fail_ba_it1 as t64_px15's chain (ba_cost 1.2e-15), fail_frame5 as t64_f16's (q 1.1e-16, point 6.0e-16).
Where a PnP accept test inside rounding noise falls the other way than in the 50-digit run (here t24_l0, t40_l3; in the numpy run
t384_wide, t64_px15) the chain's poses are at 1e-10 .. 1e-9 and the BA contracts the difference again.
"""
import re

import numpy as np
import pytest

import sfm_cases as SC
from conftest import mod

GEN = SC.GEN
pytestmark = pytest.mark.gpu
OK_CASES = [ci for ci, c in enumerate(GEN.CASES) if c[9] == 0]
FAIL_CASES = [ci for ci, c in enumerate(GEN.CASES) if c[9] != 0]


def run(ctx, inputs, device=True, max_it=None, mutate=None):
    """One avm_global_sfm_batch call on the stacked inputs; outputs start as sentinels.  Returns the outputs as host numpy arrays."""
    sfm, win, fid = SC.batch(inputs, max_it=max_it)
    if mutate:
        mutate(sfm, win)
    out = SC.out_alloc(sfm, win)
    if device:
        sfm, win, out = sfm.to_device(), win.to_device(), out.to_device()
    mod("estimator").Estimator(ctx=ctx).globalSFM(sfm, win, fid, out=out)
    return out.to_host().a


def fixture_ref(ci):
    g, p = SC.gold(), "c%d_" % ci
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p) and "_in_" not in k}


@pytest.fixture(scope="module")
def solo(ctx):
    """the B = 1 result of every fixture case (computed once, never changed)"""
    return [run(ctx, [SC.case_input(ci)]) for ci in range(len(SC.NAMES))]


@pytest.fixture(scope="module")
def solo50(ctx):
    """... with the iteration cap of the ten-case batch (ba_max_num_iterations is one number per batch: fail_ba_it1's rows are then
    t64_px15's)"""
    return [run(ctx, [SC.case_input(ci)], max_it=50) for ci in range(len(SC.NAMES))]


@pytest.mark.parametrize("ci", OK_CASES, ids=[SC.NAMES[ci] for ci in OK_CASES])
def test_parity_ok_cases(solo, ci):
    SC.check_stream(solo[ci], 0, SC.case_input(ci), fixture_ref(ci), "m_", SC.bounds())


@pytest.mark.parametrize("ci", FAIL_CASES, ids=[SC.NAMES[ci] for ci in FAIL_CASES])
def test_failure_cases(solo, ci):
    """ok = 1, 2, 3, 4; the stages the fixture stores within the same bounds; everything else still the sentinel"""
    assert int(solo[ci]["ok"][0]) == GEN.CASES[ci][9]
    SC.check_stream(solo[ci], 0, SC.case_input(ci), fixture_ref(ci), "m_", SC.bounds())


def rot6_input():
    """t40_l3 with relative_R . Rot(axis (1, 2, 3) / sqrt 14, 6 degrees): a BA with one rejected step"""
    inp = dict(SC.case_input(SC.NAMES.index("t40_l3")))
    k = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    th = np.deg2rad(6.0)
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    Rot = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)
    inp["relative_R"] = (inp["relative_R"].reshape(3, 3) @ Rot).reshape(9)
    return inp


def test_ba_with_a_rejected_step(ctx):
    inp = rot6_input()
    tr = GEN.Trace()
    ref = GEN.run(GEN.F64, inp, tr)
    assert int(ref["ok"]) == 0 and np.asarray(ref["ba_counts"]).tolist() == [8, 6, 3]
    GEN.check_trace("t40_l3_rot6", tr)
    ref = {k: (np.asarray(v, float) if k in GEN.QUANTITIES else v) for k, v in ref.items()}
    SC.check_stream(run(ctx, [inp]), 0, inp, ref, "", SC.bounds())


@pytest.fixture(scope="module")
def ten():
    return [SC.case_input(ci) for ci in range(len(SC.NAMES))]


@pytest.fixture(scope="module")
def ten_out(ctx, ten):
    return run(ctx, ten, max_it=50)


def same_rows(batch_out, rows, solos):
    for b, ci in enumerate(rows):
        for k, v in batch_out.items():
            s = solos[ci][k][0]
            got = v[b][tuple(slice(0, n) for n in s.shape)]
            assert got.tobytes() == s.tobytes(), (SC.NAMES[ci], k)
            rest = np.ones(v[b].shape, bool)
            rest[tuple(slice(0, n) for n in s.shape)] = False
            assert (v[b][rest] == (-7 if v.dtype == np.int32 else SC.SENTINEL)).all(), (SC.NAMES[ci], k, "padding written")


def test_batch_rows_are_the_solo_runs(ctx, ten, ten_out, solo50):
    """ragged shapes at common strides (max_frames 33, max_feat 384), in fixture order and reversed: no row depends on its neighbours, its
    position or the strides"""
    n = len(ten)
    same_rows(ten_out, range(n), solo50)
    same_rows(run(ctx, ten[::-1], max_it=50), range(n - 1, -1, -1), solo50)


def test_three_calls_of_different_sizes(ctx, ten, ten_out):
    first = run(ctx, ten, max_it=50)
    run(ctx, [SC.case_input(SC.NAMES.index("t24_l0"))])
    before = ctx.counters()["allocations"]
    third = run(ctx, ten, max_it=50)
    assert ctx.counters()["allocations"] == before
    for k in first:
        assert first[k].tobytes() == third[k].tobytes() == ten_out[k].tobytes(), k


def test_host_and_device_memory_give_the_same_bytes(ctx, ten, ten_out):
    host = run(ctx, ten, device=False, max_it=50)
    for k in host:
        assert host[k].tobytes() == ten_out[k].tobytes(), k


def test_chained_start(ctx):
    synth, buffers = mod("synth"), mod("buffers")
    E = mod("estimator").Estimator(ctx=ctx)
    sf, win, fid, al, _ = synth.make_sfm(2, GEN.T64, n_frames=16, key_index=GEN.IRR16)
    # the SfM alone, for the bits the chained call must hand the alignment
    alone = E.globalSFM(sf.to_device(), win.to_device(), fid).to_host().a
    assert (alone["ok"] == 0).all()
    ald, wind = al.to_device(), win.to_device()
    ald.a["frame_R"][:], ald.a["frame_T"][:] = 0.0, 0.0
    so, ao = E.initialStructure(sf.to_device(), wind, fid, ald, wind)
    assert so.a["frame_R"].data_ptr() == ald.a["frame_R"].data_ptr()
    got = ald.to_host()
    assert got.a["frame_R"].tobytes() == alone["frame_R"].tobytes() and got.a["frame_T"].tobytes() == alone["frame_T"].tobytes()
    assert (ao.to_host().a["ok"] == 1).all()
    # the same frame_R / frame_T from host arrays
    alh, winh = al.copy(), win.copy()
    alh.a["frame_R"], alh.a["frame_T"] = alone["frame_R"].copy(), alone["frame_T"].copy()
    E.visualInitialAlign(alh, winh)
    wd = wind.to_host()
    for k in ("pose", "speedbias", "inv_depth"):
        assert wd.a[k].tobytes() == winh.a[k].tobytes(), k


def refused(ctx, inputs, mutate, device, late=False):
    """late: the change is made to the tables where they live (a NULL table cannot travel)"""
    sfm, win, fid = SC.batch(inputs)
    if not late:
        mutate(sfm, win)
    out = SC.out_alloc(sfm, win)
    if device:
        sfm, win, out = sfm.to_device(), win.to_device(), out.to_device()
    if late:
        mutate(sfm, win)
    with pytest.raises(mod("lib").AvmError) as e:
        mod("estimator").Estimator(ctx=ctx).globalSFM(sfm, win, fid, out=out)
    for k, v in out.to_host().a.items():
        assert (v == (-7 if v.dtype == np.int32 else SC.SENTINEL)).all(), (k, "written by a refused call")
    return int(re.search(r"status (-?\d+)", str(e.value)).group(1)), str(e.value)


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
def test_refusals_write_nothing(ctx, device):
    abi = mod("abi")
    two = [SC.case_input(SC.NAMES.index("t24_l0")), SC.case_input(SC.NAMES.index("t64_f16"))]
    k = int(np.flatnonzero(two[1]["frame_n_pts"])[0])  # the first non-key frame of stream 1

    def put(name, index, value, tables="sfm"):
        def f(sfm, win):
            (sfm if tables == "sfm" else win).a[name][index] = value
        return f

    def dim(name, value):
        def f(sfm, win):
            sfm.dims[name] = value
        return f

    def drop(name):
        def f(sfm, win):
            sfm.a[name] = None
        return f

    def eq_ids(sfm, win):
        sfm.a["frame_pt_id"][1, k, 2] = sfm.a["frame_pt_id"][1, k, 1]

    def desc_keys(sfm, win):
        sfm.a["key_index"][1, 4] = sfm.a["key_index"][1, 3] - 1

    MP = max(i["frame_pt_id"].shape[1] for i in two)
    table_rules = [(put("l", 1, 10), "l outside"), (desc_keys, "key_index"), (eq_ids, "frame_pt_id"), (put("frame_n_pts", (1, k), MP + 1), "frame_n_pts")]
    for mutate, word in table_rules:
        rc, msg = refused(ctx, two, mutate, device)
        assert rc == abi.AVM_ERR_INVALID and "stream 1" in msg and word in msg, msg
    rc, msg = refused(ctx, two, dim("max_frames", 65), device)
    assert rc == abi.AVM_ERR_CAPACITY and "max_frames" in msg, msg
    rc, msg = refused(ctx, two, dim("ba_max_solver_time_s", 0.2), device)
    assert rc == abi.AVM_ERR_INVALID and "ba_max_solver_time_s" in msg, msg
    rc, msg = refused(ctx, two, drop("relative_T"), device, late=True)
    assert rc == abi.AVM_ERR_INVALID and "NULL" in msg, msg


def test_non_finite_observation_ends_its_stream_alone(ctx, solo):
    ci = SC.NAMES.index("t24_l0")
    clean = SC.case_input(ci)
    bad = {k: np.array(v, copy=True) for k, v in clean.items()}
    bad["obs_xy"][5, 0] = np.nan
    o = run(ctx, [bad, clean])
    assert int(o["ok"][0]) != 0
    same_rows({k: v[1:] for k, v in o.items()}, [ci], solo)


def test_cpp_host_initial_structure(ctx):
    """avm_host::Estimator::initialStructure (tests/host_cpp_init/sfm_shim.cpp) on t64_f16's data: the frames' poses, the window's states
    and the outcome are the Python path's, bit for bit - through tables with the C++ side's own (tight) strides."""
    import ctypes as C
    import os

    import align_host

    abi, ib = mod("abi"), mod("init_buffers")
    L = C.CDLL(os.path.join(SC.HERE, "host_cpp_init", "libavm_sfm_shim.so"))
    L.as_create.restype, L.as_last_error.restype, L.as_stamp.restype = C.c_void_p, C.c_char_p, C.c_double
    case = GEN.CASES[SC.NAMES.index("t64_f16")]
    inp, (sf, win, fid, al, _) = GEN.case_inputs(case)
    F, nf = int(inp["n_frames"]), int(inp["n_feat"])
    E = mod("estimator").Estimator(ctx=ctx)
    alp, winp = al.copy(), win.copy()
    so, ao = E.initialStructure(sf, winp, fid, alp, winp)
    assert int(so.a["ok"][0]) == 0 and int(ao.a["ok"][0]) == 1

    H = align_host.AlignHost(L)
    assert H.load(al, win, 0) == 0, H.err()
    ss = ib.SfmBatchArrays.of(sf).struct()
    assert L.ss_load_images(H.h, C.byref(ss), abi.iptr(np.ascontiguousarray(fid, np.int32)), C.c_int(fid.shape[1]), C.c_int(0)) == 0, H.err()
    res = (C.c_int32 * 2)(-1, -1)
    relR, relT = np.ascontiguousarray(sf.a["relative_R"][0]), np.ascontiguousarray(sf.a["relative_T"][0])
    assert L.ss_initial_structure(H.h, C.c_int(int(sf.a["l"][0])), abi.dptr(relR), abi.dptr(relT), res) == 0, H.err()
    assert (res[0], res[1]) == (1, 0)
    fR, fT = np.zeros((F, 9)), np.zeros((F, 3))
    L.ss_frames(H.h, abi.dptr(fR), abi.dptr(fT))
    assert fR.tobytes() == so.a["frame_R"][0, :F].tobytes() and fT.tobytes() == so.a["frame_T"][0, :F].tobytes()
    st = H.state(F, nf)
    assert st["solver_flag"] == 1
    assert st["pose"].tobytes() == winp.a["pose"][0].tobytes() and st["speedbias"].tobytes() == winp.a["speedbias"][0].tobytes()
    np.testing.assert_array_equal(st["inv_depth"][:nf], winp.a["inv_depth"][0, :nf])
