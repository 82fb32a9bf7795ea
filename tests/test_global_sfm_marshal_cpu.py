"""CPU tier: avm_host::marshal_sfm (include/avm_host.hpp) and the host rule function of avm_global_sfm_batch's table check in a stand-alone
program (tests/host_cpp_init/marshal_main.cpp, its own main) under the address and undefined-behaviour sanitizers.  One process takes
t384_wide, then t24_l0, then t64_f33 - large, small, large - through the same tables object; a stub in place of the entry point writes
every output array to its full declared extent.  Nothing of HIP is linked, no Python process runs under a sanitizer."""
import os
import subprocess

import numpy as np

import sfm_cases as SC
from conftest import ROOT

HERE = os.path.dirname(os.path.abspath(__file__))
ORDER = ["t384_wide", "t24_l0", "t64_f33"]
I32 = ["feat_start", "feat_nobs", "feat_obs_begin", "feat_id", "key_index", "frame_n_pts", "frame_pt_id"]
F64 = ["obs_xy", "frame_pt_xy", "relative_R", "relative_T", "ex_pose"]


def _write(path, inp):
    nf, F, P = int(inp["n_feat"]), int(inp["n_frames"]), inp["frame_pt_id"].shape[1]
    no = int((inp["feat_obs_begin"][:nf] + inp["feat_nobs"][:nf]).max())
    with open(path, "wb") as f:
        f.write(np.array([int(inp["l"]), F, nf, P, no], np.int32).tobytes())
        for k in ("feat_start", "feat_nobs", "feat_obs_begin", "feat_id"):
            f.write(np.ascontiguousarray(inp[k][:nf], np.int32).tobytes())
        f.write(np.ascontiguousarray(inp["key_index"], np.int32).tobytes())
        f.write(np.ascontiguousarray(inp["frame_n_pts"][:F], np.int32).tobytes())
        f.write(np.ascontiguousarray(inp["frame_pt_id"][:F], np.int32).tobytes())
        f.write(np.ascontiguousarray(inp["obs_xy"][:no], np.float64).tobytes())
        f.write(np.ascontiguousarray(inp["frame_pt_xy"][:F], np.float64).tobytes())
        for k in ("relative_R", "relative_T", "ex_pose"):
            f.write(np.ascontiguousarray(inp[k], np.float64).tobytes())


def _read(path):
    raw = open(path, "rb").read()
    l, F, nf, P, no = np.frombuffer(raw, np.int32, 5)
    out, off = {"l": l, "n_frames": F, "n_feat": nf, "max_pts": P, "max_obs": no}, 20
    shapes = {"feat_start": (nf,), "feat_nobs": (nf,), "feat_obs_begin": (nf,), "feat_id": (nf,), "key_index": (11,), "frame_n_pts": (F,),
              "frame_pt_id": (F, P), "obs_xy": (no, 2), "frame_pt_xy": (F, P, 2), "relative_R": (9,), "relative_T": (3,), "ex_pose": (7,)}
    for k in I32 + F64:
        dt = np.int32 if k in I32 else np.float64
        n = int(np.prod(shapes[k]))
        out[k] = np.frombuffer(raw, dt, n, off).reshape(shapes[k])
        off += n * np.dtype(dt).itemsize
    assert off == len(raw)
    return out


def test_marshal_and_rules_under_sanitizers(tmp_path):
    exe = str(tmp_path / "marshal_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                           "-DSFM_HD=inline", "-I" + os.path.join(ROOT, "include"), os.path.join(HERE, "host_cpp_init", "marshal_main.cpp"), "-o", exe])
    files = []
    for name in ORDER:
        files.append(str(tmp_path / (name + ".bin")))
        _write(files[-1], SC.case_input(SC.NAMES.index(name)))
    r = subprocess.run([exe] + files, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    assert r.stderr == "", r.stderr[-2000:]  # the sanitizers' reports go there
    for name, path in zip(ORDER, files):
        inp, got = SC.case_input(SC.NAMES.index(name)), _read(path + ".out")
        nf, F = int(inp["n_feat"]), int(inp["n_frames"])
        assert (int(got["l"]), int(got["n_frames"]), int(got["n_feat"])) == (int(inp["l"]), F, nf)
        assert int(got["max_pts"]) == max(1, int(inp["frame_n_pts"].max()))
        for k in ("feat_start", "feat_nobs", "feat_obs_begin", "feat_id"):
            np.testing.assert_array_equal(got[k], inp[k][:nf], err_msg=k)
        np.testing.assert_array_equal(got["key_index"], inp["key_index"])
        np.testing.assert_array_equal(got["frame_n_pts"], inp["frame_n_pts"][:F])
        P = int(got["max_pts"])
        np.testing.assert_array_equal(got["frame_pt_id"], inp["frame_pt_id"][:F, :P])
        np.testing.assert_array_equal(got["frame_pt_xy"], inp["frame_pt_xy"][:F, :P])
        np.testing.assert_array_equal(got["obs_xy"], inp["obs_xy"][: got["obs_xy"].shape[0]])
        for k in ("relative_R", "relative_T", "ex_pose"):
            np.testing.assert_array_equal(got[k], inp[k], err_msg=k)
