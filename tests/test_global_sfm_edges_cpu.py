"""CPU tier of tests/golden/global_sfm_edges.npz (gen_global_sfm_edges.py).

Shape checks: every case still reaches the edge it was made for - its nf and chunk tail, l, n_frames, where its state == 0 rows sit,
the point counts that meet a threshold by equality (recomputed here from the stored tables), the 64 and 65 listed points.  A case that
a regeneration moved off its edge fails here, not silently on the device.

Host build: the text of csrc/sfm/*.hpp with a team of one thread (tests/host_cpp_init/libsfm_host.so) on every edge case, as
test_global_sfm_host_cpu.py runs the first fixture: check_stream against the 50-digit m_* with sfm_edge_cases.edge_bounds(), the BA's initial
cost held to the bound derived from pnp_t's as there."""
import numpy as np
import pytest

import sfm_cases as SC
import sfm_edge_cases as EC
import gen_global_sfm_edges as EDGES  # noqa: E402  (tests/golden: on the path through sfm_cases)
from test_global_sfm_host_cpu import _run

CHUNK, WAVE, TEAM = 16, 64, 256
# name: (nf, l, n_frames, rows with point_state == 0)
SHAPES = {
    "e_l9_nf33": (33, 9, 11, []),
    "e_l5_nf47": (47, 5, 11, []),
    "e_nf257": (257, 2, 16, []),
    "e_holes64": (64, 0, 11, [30, 31, 32, 33, 34, 49, 50, 51]),
    "e_cnt10": (30, 0, 11, []),
    "e_frame6": (64, 0, 16, []),
    "e_lanes": (64, 0, 16, []),
    "e_f64": (64, 4, 64, []),
}
TAIL = {"e_l9_nf33": 1, "e_l5_nf47": 15, "e_nf257": 1, "e_holes64": 0}


def _bounds():
    """edge_bounds(), the BA's INITIAL cost as test_global_sfm_host_cpu._bounds derives it: 2 delta / sigma with delta = pnp_t's bound"""
    b = EC.edge_bounds()
    b["ba_cost0"] = max(b["ba_cost"], 2 * b["pnp_t"] / (0.5 / 460.0))
    return b


def _sees(inp, f):
    nf = int(inp["n_feat"])
    s, n = inp["feat_start"][:nf], inp["feat_nobs"][:nf]
    return (s <= f) & (f < s + n)


def _known(inp, ref, k):
    """which of frame k's listed points frame_pnp counts: the id is a row of feat_id (the first such row) with point_state set"""
    nf = int(inp["n_feat"])
    row = {int(i): j for j, i in reversed(list(enumerate(inp["feat_id"][:nf])))}
    ids = inp["frame_pt_id"][k, : int(inp["frame_n_pts"][k])]
    return np.array([int(i) in row and bool(ref["point_state"][row[int(i)]]) for i in ids])


def test_names_and_order():
    assert EC.edge_names() == list(SHAPES) == [c[0] for c in EDGES.CASES]


@pytest.mark.parametrize("name", list(SHAPES))
def test_case_reaches_its_edge(name):
    inp, ref = EC.edge_input(name), EC.edge_ref(name)
    nf, l, F, holes = SHAPES[name]
    assert (int(inp["n_feat"]), int(inp["l"]), int(inp["n_frames"])) == (nf, l, F)
    assert int(ref["ok"]) == 0 and int(inp["ba_max_num_iterations"]) == 50
    assert np.flatnonzero(ref["point_state"][:nf] == 0).tolist() == holes
    assert (inp["feat_nobs"][:nf][holes] == 1).all() and (np.delete(inp["feat_nobs"][:nf], holes) >= 2).all()
    key = inp["key_index"].tolist()
    assert key[0] == 0 and key[-1] == F - 1  # no frame in front of the first key frame or behind the last
    if name in TAIL:
        assert nf % CHUNK == TAIL[name]
    if name == "e_nf257":
        assert nf == TEAM + 1 and -(-nf // CHUNK) == 17 and int(inp["frame_n_pts"].max()) > WAVE
    if name == "e_holes64":  # every hole run has live rows on both sides; chunks 1, 2, 3 each hold holes and live rows
        st = ref["point_state"][:nf].reshape(-1, CHUNK)
        assert [int((c == 0).sum()) for c in st] == [0, 2, 3, 3]
        assert st[2, 3:].all() and st[3, 0] and st[3, 4:].all() and st[1, :14].all()
    if name == "e_cnt10":  # frame 1's PnP: the points triangulated from (l, 10) = (0, 10) so far that frame 1 sees
        first = _sees(inp, 0) & _sees(inp, 10) & (ref["point_state"][:nf] != 0)
        assert int((first & _sees(inp, 1)).sum()) == 10
        assert int((first & _sees(inp, 2)).sum()) == 10  # (tracks from frame 1 on are triangulated after frame 1's PnP: 30 from here)
    if name in ("e_frame6", "e_lanes", "e_nf257", "e_f64"):
        nonkey = [k for k in range(F) if k not in key]
        assert (inp["frame_n_pts"][key] == 0).all()
        counts = [int(_known(inp, ref, k).sum()) for k in nonkey]
        assert min(counts) >= 6
        if name == "e_frame6":
            assert counts[0] == 6 and int(inp["frame_n_pts"][nonkey[0]]) == 6 + 3 and min(counts[1:]) > 6
        if name == "e_lanes":
            assert [int(inp["frame_n_pts"][k]) for k in nonkey[:2]] == [WAVE, WAVE + 1]
            assert counts[:2] == [WAVE - 1, WAVE]
            for k in nonkey[:2]:  # the last listed point, the one a lane reaches in its second trip (or lane 63 in its first), counts
                kn = _known(inp, ref, k)
                assert kn[-1] and not kn[0]
    if name == "e_f64":
        d = np.diff(key)
        assert F == 64 and (d == 1).any() and d.max() >= 20 and F - 11 == 53


@pytest.mark.parametrize("name", list(SHAPES))
def test_err_fp64_within_ten_times_the_first_fixture(name):
    """the generator's condition on the inputs, so that edge_bounds() stays within 10 x bounds()"""
    ref, b = EC.edge_ref(name), SC.bounds()
    for q in SC.GEN.QUANTITIES:
        assert float(ref["err_fp64_" + q]) <= 10 * b[q] / 100, q
    eb = EC.edge_bounds()
    assert all(b[q] <= eb[q] <= 10 * b[q] for q in b)


@pytest.mark.parametrize("name", list(SHAPES))
def test_host_build_matches_the_edge_fixture(name):
    inp = EC.edge_input(name)
    rc, o = _run([inp])
    assert rc == 0
    SC.check_stream(o, 0, inp, EC.edge_ref(name), "m_", _bounds())
