"""CPU tier of avm_fsel_select_image_batch (FeatureSelector::select() on device-resident images): the header and the ctypes prototype,
and select_statement, the list / dict statement of the bookkeeping around the selection that tests/test_select_image.py holds the
kernels against - written from feature_selector.cpp:98-120, 156-196 and pinned here by hand-written cases, and by the existing
FeatureSelector.select (its select_batch stubbed) over a random id stream.  No GPU.
"""
import ctypes as C
import importlib

import numpy as np

from helpers import abi
from helpers import header_arg_count as _header_arg_count, header_text as _header

fs_m = importlib.import_module("anticipated-vins-mono_amd.feature_selector")
lib_m = importlib.import_module("anticipated-vins-mono_amd.lib")


def select_statement(state, image, prob, initialized, init_thresh, prune_lost, pick):
    """One FeatureSelector::select() on `image`, a dict {feature id: row} (any tuple: copied as it is), with `prob` {feature id: fPROB}.
    state: dict(last_feature_id, tracked: list in append order, first_image), updated in place.  pick(cand, used) stands for
    selectInformativeFeatures: cand = [(id, row, prob)] and used = [(id, row)], both ascending; it returns the selected ids in selection
    order.  Returns dict(cand, used, selected, image_out): the selector problem's candidate and used points as the call writes them
    (cand is empty for an uninitialized window: n_cand = 0), the selection, and the image the back end receives {id: row}."""
    ids = sorted(image)
    last = state["last_feature_id"]
    new = [i for i in ids if i > last]                       # splitOnFeatureId: upper_bound, strictly greater
    old = [i for i in ids if i <= last]
    if new:
        state["last_feature_id"] = new[-1]
    found = [f for f in state["tracked"] if f in old]        # image.find() after the split: among the old points only
    subset = set(found)
    used = [(i, image[i]) for i in sorted(subset)]
    cand = [(i, image[i], prob[i]) for i in new] if initialized else []
    if prune_lost:
        state["tracked"][:] = found
    selected = []
    if initialized:
        selected = list(pick(cand, used))
        subset |= set(selected)
    elif state["first_image"]:
        subset = set(new)                                    # subset.swap(image_new)
        state["tracked"].extend(new)
        state["first_image"] = 0
    if not initialized and len(subset) < init_thresh:
        subset |= set(old)                                   # subset.insert(image.begin(), image.end())
    state["tracked"].extend(selected)
    return dict(cand=cand, used=used, selected=selected, image_out={i: image[i] for i in sorted(subset)})


# ---------------------------------------------------------------- header and prototype
def test_header_declares_the_entry_point_and_the_prototype_matches():
    name = "avm_fsel_select_image_batch"
    assert _header_arg_count(name) == 11 == len(abi.PROTOTYPES[name][1])
    assert name in lib_m.EXPORTS
    assert "#define AVM_ABI_VERSION 6 " in _header() and abi.AVM_ABI_VERSION == 6
    assert "typedef struct avm_select_state {" in _header()
    S = abi.SelectState
    assert [f[0] for f in S._fields_] == ["max_tracked", "last_feature_id", "n_tracked", "tracked_id", "first_image"]
    assert (C.sizeof(S), S.last_feature_id.offset, S.first_image.offset) == (40, 8, 32)
    L = lib_m.lib()                                          # (loads without a GPU)
    assert L.avm_fsel_select_image_batch.argtypes == abi.PROTOTYPES[name][1]
    for word in ("never issues a lost id again", "decided BEFORE the selection", "conservative on purpose"):
        assert word in _header(), word


# ---------------------------------------------------------------- the statement on hand-written cases
def _img(*ids):
    return {i: (0.1 * i, -0.1 * i) for i in ids}, {i: 0.5 + 0.001 * i for i in ids}


def _state(last, tracked, first=0):
    return dict(last_feature_id=last, tracked=list(tracked), first_image=first)


def _first_two(cand, used):
    return [c[0] for c in cand[:2]][::-1]                    # a selection order that is not ascending


def test_split_is_a_strict_upper_bound():
    image, prob = _img(3, 5, 8, 9)
    # last_feature_id equal to an image id: that point is old
    st = _state(5, [5, 3])
    r = select_statement(st, image, prob, True, 0, False, _first_two)
    assert [c[0] for c in r["cand"]] == [8, 9] and [u[0] for u in r["used"]] == [3, 5]
    assert r["cand"][0] == (8, image[8], prob[8]) and r["used"][1] == (5, image[5])
    assert r["selected"] == [9, 8] and sorted(r["image_out"]) == [3, 5, 8, 9] and r["image_out"][9] == image[9]
    assert st == dict(last_feature_id=9, tracked=[5, 3, 9, 8], first_image=0)
    # below all: every point is new, nothing can be found
    st = _state(2, [3, 5])
    r = select_statement(st, image, prob, True, 0, False, _first_two)
    assert [c[0] for c in r["cand"]] == [3, 5, 8, 9] and r["used"] == [] and sorted(r["image_out"]) == [3, 5]
    assert st == dict(last_feature_id=9, tracked=[3, 5, 5, 3], first_image=0)
    # above all: nothing is new, last_feature_id stays
    st = _state(20, [9, 4, 3])
    r = select_statement(st, image, prob, True, 0, False, _first_two)
    assert r["cand"] == [] and [u[0] for u in r["used"]] == [3, 9] and r["selected"] == [] and sorted(r["image_out"]) == [3, 9]
    assert st == dict(last_feature_id=20, tracked=[9, 4, 3], first_image=0)


def test_empty_image_nothing_tracked_and_a_tracked_id_above_last_feature_id():
    st = _state(7, [4, 6], first=1)
    r = select_statement(st, {}, {}, True, 0, False, _first_two)
    assert r == dict(cand=[], used=[], selected=[], image_out={}) and st == _state(7, [4, 6], first=1)
    r = select_statement(st, {}, {}, False, 5, True, _first_two)          # ... uninitialized: the first image is consumed, the list pruned
    assert r == dict(cand=[], used=[], selected=[], image_out={}) and st == _state(7, [], first=0)
    # nothing tracked: only what is selected passes
    image, prob = _img(3, 5, 8, 9)
    st = _state(5, [])
    r = select_statement(st, image, prob, True, 0, False, _first_two)
    assert r["used"] == [] and sorted(r["image_out"]) == [8, 9] and st["tracked"] == [9, 8]
    # a tracked id above last_feature_id is in the image, but among the new points: never found
    st = _state(5, [8, 3])
    r = select_statement(st, image, prob, True, 0, False, lambda cand, used: [9])
    assert [u[0] for u in r["used"]] == [3] and [c[0] for c in r["cand"]] == [8, 9] and sorted(r["image_out"]) == [3, 9]
    assert st["tracked"] == [8, 3, 9]
    st = _state(5, [8, 3])
    select_statement(st, image, prob, True, 0, True, lambda cand, used: [9])
    assert st["tracked"] == [3, 9]                                         # ... and pruning drops it


def test_kappa_zero_selects_nothing():
    image, prob = _img(3, 5, 8, 9)
    st = _state(5, [3, 5])
    r = select_statement(st, image, prob, True, 0, False, lambda cand, used: [])
    assert [c[0] for c in r["cand"]] == [8, 9] and sorted(r["image_out"]) == [3, 5] and st == _state(9, [3, 5])


def test_first_image_and_init_thresh():
    image, prob = _img(3, 5, 8, 9, 12)
    never = lambda cand, used: 1 / 0                                       # an uninitialized window runs no selection
    # the first image: the subset BECOMES the new points (a tracked old point is dropped), all of them tracked from now on
    st = _state(5, [3], first=1)
    r = select_statement(st, image, prob, False, 3, False, never)
    assert r["cand"] == [] and [u[0] for u in r["used"]] == [3] and sorted(r["image_out"]) == [8, 9, 12]   # 3 points: init_thresh 3 does not fire
    assert st == _state(12, [3, 8, 9, 12], first=0)
    st = _state(5, [3], first=1)
    r = select_statement(st, image, prob, False, 4, False, never)           # 3 < 4: every old point joins
    assert sorted(r["image_out"]) == [3, 5, 8, 9, 12] and st == _state(12, [3, 8, 9, 12], first=0)
    # a later uninitialized image appends nothing; the subset is the tracked points
    st = _state(8, [3, 8], first=0)
    r = select_statement(st, image, prob, False, 2, False, never)
    assert sorted(r["image_out"]) == [3, 8] and st == _state(12, [3, 8], first=0)
    st = _state(8, [3, 8], first=0)
    r = select_statement(st, image, prob, False, 3, False, never)           # 2 < 3: the old points 3, 5, 8 - not the new ones
    assert sorted(r["image_out"]) == [3, 5, 8] and st == _state(12, [3, 8], first=0)
    # an initialized window never looks at init_thresh or first_image
    st = _state(8, [3], first=1)
    r = select_statement(st, image, prob, True, 99, False, lambda cand, used: [12])
    assert sorted(r["image_out"]) == [3, 12] and st == _state(12, [3, 12], first=1)


def test_pruning_is_an_order_preserving_compaction():
    image, prob = _img(3, 5, 8, 9)
    tracked = [5, 40, 3, 41, 1]                                            # lost ids in the middle and at the end
    st = _state(5, tracked)
    r0 = select_statement(st, image, prob, True, 0, False, _first_two)
    assert st["tracked"] == [5, 40, 3, 41, 1, 9, 8]
    st = _state(5, tracked)
    r1 = select_statement(st, image, prob, True, 0, True, _first_two)
    assert st["tracked"] == [5, 3, 9, 8] and r0 == r1                      # the same problem, selection and image


# ---------------------------------------------------------------- against FeatureSelector.select over a random id stream
class _StubOut:
    def __init__(self, ids):
        self.a = {"n_selected": np.array([len(ids)], np.int32), "selected_ids": np.array([list(ids) + [-1]], np.int32)}

    def to_host(self):
        return self


def test_statement_equals_feature_selector_select_over_five_frames():
    rng = np.random.default_rng(5)
    MAXF, THRESH = 9, 6

    def pick(cand_ids, used_ids):
        kappa = max(0, MAXF - len(used_ids))
        order = sorted(cand_ids, key=lambda i: (i * 7919) % 101)
        return order[:min(kappa, len(order), 3)]

    sel = fs_m.FeatureSelector(ctx=object())
    sel.setParameters(True, MAXF, THRESH)
    st = dict(last_feature_id=sel.lastFeatureId_, tracked=[], first_image=1)
    alive, next_id, n_selected = [], 1, 0
    for frame, initialized in enumerate([False, False, True, True, True]):
        alive = [i for i in alive if rng.uniform() < 0.8]                  # ids are lost for good, new ones are larger than any before
        born = int(rng.integers(2, 7)) if frame else 4
        alive += list(range(next_id, next_id + born))
        next_id += born
        image = {i: (float(i), float(frame)) for i in alive}
        prob = {i: 0.5 for i in alive}
        builder = lambda new_ids, used_ids: (new_ids, used_ids)
        sel.select_batch = lambda p: _StubOut(pick(*p))
        ref_image = dict(image)
        tracked_ref, selected_ref = sel.select(ref_image, builder, initialized)
        r = select_statement(st, image, prob, initialized, THRESH, False, lambda cand, used: pick([c[0] for c in cand], [u[0] for u in used]))
        assert r["image_out"] == ref_image and r["selected"] == selected_ref, frame
        assert st["tracked"] == tracked_ref and st["last_feature_id"] == sel.lastFeatureId_, frame
        assert bool(st["first_image"]) == bool(getattr(sel, "firstImage_", True)), frame
        n_selected += len(selected_ref)
    assert n_selected >= 3 and len(st["tracked"]) > len(set(st["tracked"]) & set(alive))      # something was selected, something was lost
