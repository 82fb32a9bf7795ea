"""CPU tier of Estimator::visualInitialAlign: the fixture's FP64 half regenerates, the ctypes structs match the header, and the C++
host marshals all_image_frame into avm_align_batch.  (The statuses of malformed tables need an avm_ctx, which needs a device:
tests/test_visual_align.py, test_statuses_and_timings.)"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from conftest import mod

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import gen_visual_align as GEN  # noqa: E402


def test_fp64_part_of_the_fixture_regenerates():
    gold = np.load(os.path.join(HERE, "golden", "visual_align.npz"))
    again = GEN.fp64_part()
    for k, v in again.items():
        assert k in gold.files, k
        np.testing.assert_array_equal(gold[k], v, err_msg=k)
    rest = set(gold.files) - set(again)
    assert rest and all("_m_" in k or "_err_fp64_" in k for k in rest), sorted(rest)[:5]  # the 50-digit half


def test_fixture_keeps_its_decisions_away_from_rounding():
    gold = np.load(os.path.join(HERE, "golden", "visual_align.npz"))
    oks = 0
    for ci, case in enumerate(GEN.CASES):
        p = "c%d_" % ci
        if p + "f_s_linear" in gold.files:
            gl, sl, Gn = np.linalg.norm(gold[p + "f_g_linear"]), float(gold[p + "f_s_linear"][0]), np.linalg.norm(gold[p + "g_opt"])
            assert abs(abs(gl - Gn) - 1.0) > 0.05 and abs(sl) > 0.05, case[0]
        if gold[p + "ok"]:
            oks += 1
            assert abs(float(gold[p + "f_s"][0]) / GEN.TRUE_SCALE - 1.0) < 0.10, case[0]
    assert oks == len(GEN.CASES) - 3 and sorted({c[2] for c in GEN.CASES}) == [3, 4, 5, 11, 16, 17, 33, 64]


def test_ctypes_structs_match_the_header(abi):
    L = mod("lib").lib()
    out = (C.c_int * 32)()
    n = L.avm_debug_align_layout(out)
    got = [out[i] for i in range(n)]
    want = [C.sizeof(abi.AlignBatch), C.sizeof(abi.AlignOut), abi.MAX_ALIGN_FRAMES]
    want += [getattr(abi.AlignBatch, f).offset for f, _ in abi.AlignBatch._fields_]
    want += [getattr(abi.AlignOut, f).offset for f, _ in abi.AlignOut._fields_]
    assert got == want
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "avm.h")).read()
    assert "#define AVM_ABI_VERSION 6" in hdr  # no existing struct or entry point changed


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    import align_host

    return align_host.build_shim(tmp_path_factory.mktemp("align_shim"))


def test_cpp_host_marshals_all_image_frame(shim, synth):
    """all_image_frame / Headers -> avm_align_batch, key_index included, ragged intervals; no device is touched."""
    import align_host

    al, win = synth.make_align(2, 17, key_index=GEN.IRR17, first_id=40, ragged=True, bgs0=(0.001, 0.002, -0.003), n_feat=6)
    H = align_host.AlignHost(shim)
    for w in range(2):
        assert H.load(al, win, w) == 0, H.err()
        rc, t = H.marshal(17, al.dims["max_samp"])
        assert rc == 0, H.err()
        assert t["n_frames"] == 17
        for k in ("frame_R", "frame_T", "tic", "imu_n", "imu_dt", "imu_acc", "imu_gyr", "imu_lin_ba", "imu_lin_bg", "key_index"):
            np.testing.assert_array_equal(t[k], al.a[k][w], err_msg=k)
    # the tables take the strides of the frames that are there
    rc, t = H.marshal(20, al.dims["max_samp"] + 3)
    assert rc == 0 and t["n_frames"] == 17 and not t["imu_acc"][16:].any()
    np.testing.assert_array_equal(t["imu_acc"][:16, : al.dims["max_samp"] + 1], al.a["imu_acc"][1])
    # a header without a frame, too many frames: errors before any device work
    assert H.load(al, win, 0, drop_header=4) == 0
    rc, _ = H.marshal(17, al.dims["max_samp"])
    assert rc == mod("abi").AVM_ERR_INVALID and "Headers[4]" in H.err()
    big, _ = synth.make_align(1, 65, frame_samples=2)
    assert H.load(big, None, 0) == 0
    rc, _ = H.marshal(65, 2)
    assert rc == mod("abi").AVM_ERR_CAPACITY and "64" in H.err()
    rc, res = H.align()  # (the capacity error comes before the context is opened)
    assert rc == mod("abi").AVM_ERR_CAPACITY
