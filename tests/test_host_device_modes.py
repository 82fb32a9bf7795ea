"""GPU tier (-m gpu): AVM_MEM_HOST against AVM_MEM_DEVICE, entry point by entry point.

A host-mode call stages the caller's tables through the ctx's pool (small batches as one packed pinned copy each way,
larger ones table by table), runs the kernels a device-mode call runs on the caller's own buffers, and copies the
outputs back.  Nothing numerical sits in between: every output is equal to the bit.  The sizes are chosen by bytes -
one batch below the 4 MiB pack limit and one above it - not by workload.

avm_triangulate_batch is compared this way by test_gpu_parity.test_triangulation_matches_oracle (its one output,
inv_depth) and is not repeated here.
"""
import ctypes as C

import numpy as np
import pytest

from helpers import abi, buffers, synth

pytestmark = pytest.mark.gpu

PACK_LIMIT = 4 << 20  # csrc/api/staging.hpp: batches up to 4 MiB travel packed, every table rounded up to 64 bytes
SUMMARY_FIELDS = ("num_iterations", "num_successful", "accept_mask", "termination", "cost_trace", "radius_trace")
PRIOR_FIELDS = ("n", "nblk", "blk_kind", "blk_frame", "J", "r", "x0")


def _mod(name):
    import importlib

    return importlib.import_module("anticipated-vins-mono_amd." + name)


def _packed_bytes(arrays):
    return sum((v.nbytes + 63) // 64 * 64 for v in arrays.values())


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# Allocations (avm_debug_counters()[0]) of the first host-mode MARGIN_OLD solve on a fresh ctx, taken from a run of the commit
# before the staging code of avm_api.hip was rewritten over descriptor tables: one per pool name the call touches, so the
# numbers pin the pool names and the pack rule.
FIRST_CALL_ALLOCATIONS = {"packed": 10, "unpacked": 28}


@pytest.fixture(scope="module", params=[(4, "packed"), (64, "unpacked")], ids=lambda p: p[1])
def marg_solve_modes(request):
    """One MARGIN_OLD solve of the same windows: twice in host mode on a fresh ctx, then once in device mode."""
    import torch

    B, path = request.param
    base = synth.make_windows(4, tracks="sparse", n_feat=20, max_feat=150)
    w = base if B == 4 else synth.tile_windows(base, B)
    prior = buffers.PriorOutArrays.alloc(B, 96, 16)
    in_bytes, out_bytes = _packed_bytes(w.a), _packed_bytes(prior.a)
    if path == "packed":
        assert in_bytes <= PACK_LIMIT and out_bytes <= PACK_LIMIT
    else:
        assert B * 96 * 96 * 8 > PACK_LIMIT  # prior_J / prior_out->J alone: neither direction packs
        assert w.a["prior_J"].nbytes > PACK_LIMIT and prior.a["J"].nbytes > PACK_LIMIT
    ctx = _mod("lib").Context(0)
    E = _mod("estimator").Estimator(ctx=ctx, options=abi.default_options())
    assert E.options.marginalization_flag == abi.MARGIN_OLD
    counts = [ctx.counters()["allocations"]]
    h = None
    for _ in range(2):
        h = w.copy()
        hs = buffers.summary_to_numpy(E.optimization(h)).copy()
        counts.append(ctx.counters()["allocations"])
    hp = E.last_marginalization_info
    host_form = ctx.last_solve_form()
    d = w.to_device("cuda:0")
    ds = E.optimization(d)
    torch.cuda.synchronize()
    out = dict(path=path, counts=counts, w=w, h=h, hs=hs, hp=hp, d=d.to_host(), ds=buffers.summary_to_numpy(ds),
               dp=E.last_marginalization_info.to_host(), forms=(host_form, ctx.last_solve_form()))
    ctx.close()
    return out


def test_marginalizing_solve_is_bit_equal_in_host_and_device_mode(marg_solve_modes):
    m = marg_solve_modes
    assert m["forms"] == ("latency", "latency")  # (fewer windows than compute units in both sizes)
    for k in ("pose", "speedbias", "ex_pose", "inv_depth"):
        assert np.array_equal(m["d"].a[k], m["h"].a[k]), k
    assert not np.array_equal(m["h"].a["pose"], m["w"].a["pose"])
    for k in SUMMARY_FIELDS:
        assert np.array_equal(m["ds"][k], m["hs"][k]), k
    assert (m["hs"]["num_iterations"] >= 1).all()
    for k in PRIOR_FIELDS:
        assert np.array_equal(m["dp"].a[k], m["hp"].a[k]), k
    assert (m["hp"].a["n"] > 0).all() and np.isfinite(m["hp"].a["J"]).all()


def test_a_second_identical_host_call_allocates_nothing(marg_solve_modes):
    c0, c1, c2 = marg_solve_modes["counts"]
    print("allocations: fresh ctx %d, after the first host-mode call %d, after the second %d" % (c0, c1, c2))
    assert c2 - c1 == 0
    assert c1 == FIRST_CALL_ALLOCATIONS[marg_solve_modes["path"]]


# The same for the entry points whose staging was moved onto the descriptor tables and array_in / array_out / array_back with the split
# of avm_api.hip into csrc/api/*.hpp: 3 windows, max_feat 16, max_pts 8.  The counts come from a run of these calls against a build of
# commit af70961 (the last one with the single avm_api.hip), not from the code under test.
STAGING_FIRST_CALL_ALLOCATIONS = {"add_image": 15, "imu_push": 10, "solve_view": 15, "store_depths": 7, "keyframe_decision": 8,
                                  "failure_detection": 4, "build_cloud": 12, "select_image": 52}


@pytest.fixture(scope="module")
def staging_calls(ctx):
    """name -> call(ctx): one host-mode call of the entry point on fresh copies of the same small inputs (built once for the eight cases)"""
    import copy

    from test_mixed_batch import MIN_PARALLAX
    from test_select_image import Case
    from test_tracks import GOOD, _image, _set_tracks

    from helpers import blank_windows

    # (the rows of test_tracks._small in tables of strides 16 / 64: four of the five pass the solve's filter)
    w = blank_windows(3, max_feat=16, max_obs=64, max_samp=8)
    feats = [dict(id=i, start=st, obs=[(0.1 * i, 0.01 * k) for k in range(no)], inv_depth=0.5)
             for i, st, no in ((10, 0, 10), (4, 2, 8), (2, 3, 3), (8, 7, 3), (6, 9, 1))]
    fid = _set_tracks(w, [copy.deepcopy(feats) for _ in range(3)], False)
    w.a["imu_n"][:] = 4
    img = _image(GOOD, max_pts=8)
    E = lambda ctx: _mod("estimator").Estimator(ctx=ctx, options=abi.default_options())
    tables = lambda: buffers.TrackTables(w.copy(), fid.copy(), 16, 64)
    viewed = tables()
    E(ctx).solve_view(viewed)
    assert viewed.view.a["n_feat"].tolist() == [4, 4, 4]
    case = Case([(0, 0, 0, 0, 1, 0), (1, 1, 0, 1, 1, 0), (8, 5, 2, 4, 1, 1)], max_pts=8, max_used=8, max_tracked=16)
    k1_pos, k1_quat = w.a["pose"][:, 10, :3].copy(), w.a["pose"][:, 10, 3:].copy()
    return {
        "add_image": lambda ctx: E(ctx).addFeatureCheckParallax(w.copy(), fid.copy(), img.copy(), MIN_PARALLAX),
        "imu_push": lambda ctx: E(ctx).push_imu(w.copy(), np.full(3, 2), np.full((3, 4), 0.005), np.zeros((3, 4, 3)), np.zeros((3, 4, 3))),
        "solve_view": lambda ctx: E(ctx).solve_view(tables()),
        "store_depths": lambda ctx: E(ctx).setDepth(viewed),
        "keyframe_decision": lambda ctx: E(ctx).keyframe_decision(w.copy(), MIN_PARALLAX),
        "failure_detection": lambda ctx: E(ctx).failureDetection(w.copy(), np.zeros((3, 3))),
        "build_cloud": lambda ctx: _mod("feature_selector").FeatureSelector(ctx=ctx).initKDTree(w.copy(), k1_pos, k1_quat, max_cloud=9),
        "select_image": lambda ctx: case.run(ctx, "host", False),
    }


@pytest.mark.parametrize("name", sorted(STAGING_FIRST_CALL_ALLOCATIONS))
def test_staging_allocations_of_the_smaller_entry_points(staging_calls, name):
    call = staging_calls[name]
    fresh = _mod("lib").Context(0)
    counts = [fresh.counters()["allocations"]]
    for _ in range(2):
        call(fresh)
        counts.append(fresh.counters()["allocations"])
    fresh.close()
    print("allocations of %s: fresh ctx %d, after the first host-mode call %d, after the second %d" % ((name,) + tuple(counts)))
    assert counts[2] - counts[1] == 0
    assert counts[1] - counts[0] == STAGING_FIRST_CALL_ALLOCATIONS[name]


@pytest.fixture(scope="module")
def small_windows():
    """3 small windows with ragged IMU intervals (short enough for MARGIN_SECOND_NEW's merge of the last two)."""
    w = synth.make_windows(3, tracks="sparse", n_feat=12, max_feat=16, max_samp=40)
    w.a["imu_n"][:] = np.random.default_rng(4).integers(5, 18, w.a["imu_n"].shape)
    return w


def test_dead_reckoning_host_and_device_mode(estimator, small_windows):
    w = small_windows.copy()
    w.a["pose"][:, 10], w.a["speedbias"][:, 10] = w.a["pose"][:, 9], w.a["speedbias"][:, 9]
    h, d = w.copy(), w.to_device("cuda:0")
    estimator.imu_propagate(h)
    estimator.imu_propagate(d)
    assert not np.array_equal(h.a["pose"], w.a["pose"])
    for k, v in d.to_host().a.items():
        assert np.array_equal(v, h.a[k]), k


@pytest.mark.parametrize("flag,shift", [(abi.MARGIN_OLD, True), (abi.MARGIN_SECOND_NEW, False)], ids=["old", "second_new"])
def test_window_roll_host_and_device_mode(estimator, small_windows, flag, shift):
    h, d = small_windows.copy(), small_windows.to_device("cuda:0")
    estimator.slideWindow(h, flag, shift, 5.0)
    estimator.slideWindow(d, flag, shift, 5.0)
    assert not np.array_equal(h.a["pose"], small_windows.a["pose"])
    for k, v in d.to_host().a.items():
        assert np.array_equal(v, h.a[k]), k


def test_preintegration_host_and_device_mode(estimator, small_windows):
    import torch

    B = 3
    host = estimator.preintegrate(small_windows.copy())
    d = small_windows.to_device("cuda:0")
    outs = [torch.zeros(x.shape, dtype=torch.float64, device="cuda:0") for x in host]
    s = d.struct()
    rc = estimator.ctx._L.avm_imu_preintegrate_batch(estimator.ctx.h, C.byref(estimator.options), d.mem, C.byref(s), *[abi.dptr(t) for t in outs])
    estimator.ctx.check(rc, "avm_imu_preintegrate_batch")
    torch.cuda.synchronize()
    assert host[0].shape == (B, 10, 10) and np.abs(host[0]).max() > 0
    for a, t in zip(host, outs):
        assert np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize("loss", [False, True], ids=["plain", "loss"])
def test_factor_evaluation_host_and_device_mode(estimator, small_windows, loss):
    import torch

    host = estimator.eval_factors(small_windows.copy(), apply_loss=loss)
    keys = ("proj_r", "proj_J", "imu_r", "imu_J", "prior_res", "cost")
    d = small_windows.to_device("cuda:0")
    outs = {k: torch.zeros(host[k].shape, dtype=torch.float64, device="cuda:0") for k in keys}
    s = d.struct()
    rc = estimator.ctx._L.avm_window_eval_factors(estimator.ctx.h, C.byref(estimator.options), d.mem, C.byref(s), int(loss),
                                                  *[abi.dptr(outs[k]) for k in keys])
    estimator.ctx.check(rc, "avm_window_eval_factors")
    torch.cuda.synchronize()
    assert (host["cost"] > 0).all()
    for k in keys:
        assert np.array_equal(outs[k].cpu().numpy(), host[k]), k


def test_depth_cloud_host_and_device_mode(selector, small_windows):
    import torch

    B, mc = 3, 9  # (fewer slots than features with a depth: the cloud is cut at max_cloud in both modes)
    k1_pos, k1_quat = small_windows.a["pose"][:, 10, :3].copy(), small_windows.a["pose"][:, 10, 3:].copy()
    n, xy, dep = selector.initKDTree(small_windows.copy(), k1_pos, k1_quat, max_cloud=mc)
    d = small_windows.to_device("cuda:0")
    dn = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    dxy = torch.zeros((B, mc, 2), dtype=torch.float64, device="cuda:0")
    ddep = torch.zeros((B, mc), dtype=torch.float64, device="cuda:0")
    s = d.struct()
    kp, kq = _dev(k1_pos), _dev(k1_quat)
    rc = selector.ctx._L.avm_fsel_build_cloud(selector.ctx.h, d.mem, C.byref(s), abi.dptr(kp), abi.dptr(kq), mc, abi.iptr(dn), abi.dptr(dxy),
                                              abi.dptr(ddep))
    selector.ctx.check(rc, "avm_fsel_build_cloud")
    torch.cuda.synchronize()
    assert (n > 0).all()
    assert np.array_equal(dn.cpu().numpy(), n) and np.array_equal(dxy.cpu().numpy(), xy) and np.array_equal(ddep.cpu().numpy(), dep)


@pytest.mark.parametrize("path", ["packed", "unpacked"])
def test_select_host_and_device_mode(selector, path):
    if path == "packed":
        pr = synth.make_fsel(2, horizon=2, n_cand=40, n_used=2, n_cloud=10, max_features=8)
        assert _packed_bytes(pr.a) <= PACK_LIMIT
    else:
        # the strides set the bytes: the depth cloud's two tables alone are 64 x 4096 x 24 B
        pr = synth.make_fsel(64, horizon=2, n_cand=40, n_used=2, n_cloud=10, max_features=8, max_cloud=4096)
        assert 64 * 4096 * 24 > PACK_LIMIT and pr.a["cloud_xy"].nbytes + pr.a["cloud_depth"].nbytes == 64 * 4096 * 24
    h = selector.select_batch(pr)
    form = selector.ctx.last_fsel_form()
    d = selector.select_batch(pr.to_device("cuda:0")).to_host()
    assert selector.ctx.last_fsel_form() == form
    assert (h.a["n_selected"] > 0).all()
    assert np.array_equal(d.a["n_selected"], h.a["n_selected"]) and np.array_equal(d.a["selected_ids"], h.a["selected_ids"])
    for q in range(pr.n_problems):  # (fvalues beyond n_selected are not written)
        n = int(h.a["n_selected"][q])
        assert np.array_equal(d.a["fvalues"][q, :n], h.a["fvalues"][q, :n])
