"""CPU tier: the text of csrc/sfm/*.hpp - the chain, the PnP, the BA, the frames' PnP, the table rules - compiled for the host with a
team of one thread (tests/host_cpp_init/sfm_host.cpp) against the statement's fixture, with the bounds and the exact quantities of the
device test (tests/test_global_sfm.py).  What only the device has (wave reductions, the MFMA product, the staging) is not covered here."""
import ctypes as C
import os

import numpy as np
import pytest

import sfm_cases as SC
from conftest import mod

HERE = os.path.dirname(os.path.abspath(__file__))
LIB = os.path.join(HERE, "host_cpp_init", "libsfm_host.so")


def _bounds():
    """The issue's bounds, except for the INITIAL cost of the BA.  That number is 1/2 sum r^2 at the chain's output, residuals r of the
    size of the image noise sigma = 0.5 / 460.  A chain that is off by a relative delta (a PnP accept test inside rounding noise that
    fell the other way: DESIGN.md 2.24; delta is bounded by pnp_t's bound) moves every prediction by up to delta in normalized
    coordinates, the cost by up to sum |r| delta, that is by 2 delta / sigma of itself - where the points of later frames were triangulated
    from the frame in question; the 50-digit run, the FP64 numpy run and this build each take those tests in their own way."""
    b = SC.bounds()
    b["ba_cost0"] = max(b["ba_cost"], 2 * b["pnp_t"] / (0.5 / 460.0))
    return b


def _run(inputs):
    abi = mod("abi")
    L = C.CDLL(LIB)
    L.sfm_host_run.restype = C.c_int
    L.sfm_host_run.argtypes = [C.POINTER(abi.SfmBatch), C.POINTER(abi.WindowBatch), abi.c_ip, C.POINTER(abi.SfmOut)]
    sfm, win, fid = SC.batch(inputs)
    out = SC.out_alloc(sfm, win)
    ss, sw, so = sfm.struct(), win.struct(), out.struct()
    rc = L.sfm_host_run(C.byref(ss), C.byref(sw), abi.iptr(fid), C.byref(so))
    return rc, out.a


@pytest.mark.parametrize("ci", range(len(SC.NAMES)), ids=SC.NAMES)
def test_host_build_matches_the_fixture(ci):
    g = SC.gold()
    inp = SC.case_input(ci)
    rc, o = _run([inp])
    assert rc == 0
    p = "c%d_" % ci
    ref = {k[len(p):]: v for k, v in g.items() if k.startswith(p) and "_in_" not in k}
    SC.check_stream(o, 0, inp, ref, "m_", _bounds())


def test_host_rules_name_stream_and_rule():
    kern = {"l": 1, "n_frames": 2, "key_index": 3, "frame_n_pts": 4, "frame_pt_id": 5}
    good = SC.case_input(SC.NAMES.index("t64_f16"))
    k = int(np.flatnonzero(good["frame_n_pts"])[0])  # the first non-key frame
    for what, rule in kern.items():
        bad = {k: np.array(v, copy=True) for k, v in good.items()}
        if what == "l":
            bad["l"] = np.int32(10)
        elif what == "n_frames":
            bad["n_frames"] = np.int32(10)
        elif what == "key_index":
            bad["key_index"][4] = bad["key_index"][3]
        elif what == "frame_n_pts":
            bad["frame_n_pts"][k] = bad["frame_pt_id"].shape[1] + 1
        else:
            bad["frame_pt_id"][k, 2] = bad["frame_pt_id"][k, 1]
        rc, o = _run([good, bad])
        assert rc == 8 * 1 + rule, (what, rc)
        assert (o["ok"] == -7).all()
