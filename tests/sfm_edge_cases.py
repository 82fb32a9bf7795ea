"""TEST INFRASTRUCTURE: the edge fixture tests/golden/global_sfm_edges.npz (gen_global_sfm_edges.py: chunk tails, holes, l = 5 and 9,
thresholds met by count, 64 / 65 listed points, 64 frames) next to sfm_cases.py, whose batch(), out_alloc() and check_stream() its tests
use unchanged, and the bound of those tests: 100 x the largest err_fp64_<quantity> over the cases of BOTH fixtures."""
import os

import numpy as np

import sfm_cases as SC

_edge_gold = None


def edge_gold():
    global _edge_gold
    if _edge_gold is None:
        _edge_gold = dict(np.load(os.path.join(SC.HERE, "golden", "global_sfm_edges.npz")))
    return _edge_gold


def edge_names():
    return [str(n) for n in edge_gold()["names"]]


def edge_input(name):
    g = edge_gold()
    p = "c%d_in_" % edge_names().index(name)
    return {k[len(p):]: g[k] for k in g if k.startswith(p)}


def edge_ref(name):
    """everything the fixture stores of the case but its inputs: ok, point_state, ba_counts, f_*, m_*, err_fp64_*"""
    g = edge_gold()
    p = "c%d_" % edge_names().index(name)
    return {k[len(p):]: v for k, v in g.items() if k.startswith(p) and "_in_" not in k}


def edge_bounds():
    """per quantity: 100 x the FP64 numpy run's own worst distance from the 50-digit run over the cases of both fixtures"""
    gs = (SC.gold(), edge_gold())
    return {q: 100 * max(float(g[k]) for g in gs for k in g if k.endswith("_err_fp64_" + q)) for q in SC.GEN.QUANTITIES}
