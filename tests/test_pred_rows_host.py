"""The device-side selection of predicted proposals on the host: the numpy restatement of tests/pred_rows_cases.py against
the reference's own outputs (tests/golden/pred_rows_ref.npz, written by tests/golden/make_golden_pred_rows.py) under the
comparison stated in include/gps_hip.h; the emulated device law; the exports and argument checks of gps_obj_select_pred
and gps_proposal_labels, which come before any launch; and the wrapper's host-side refusals.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pred_rows_cases as C  # noqa: E402
import rows_cases  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_objects import select_rows  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "pred_rows_ref.npz"))
KEYS = ("sel", "tgt_id", "n_sel", "iou25", "iou50", "labels", "n_rem", "is_multiple", "is_hard", "order")


def gold(case):
    return {k: GOLD[f"{case['name']}/{k}"] for k in KEYS}


def test_entries_are_declared_bound_and_built():
    lib = _native.load()
    for name in ("gps_obj_select_pred", "gps_proposal_labels"):
        assert name in _native.declared_symbols() and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.gps_abi_version() == 11                                         # additive: the ABI number does not move
    from sceneverse_amd.csrc import build
    assert ("gps_obj_select_pred.hip", ["-ffp-contract=off"]) in build.SOURCES
    assert ("gps_refer.hip", ["-ffp-contract=off"]) in build.SOURCES
    text = open(_native.HEADER_PATH).read()
    for cite in ("base.py:353-366", "base.py:420-450", "base.py:427", "scannet.py:50", "list(set(...))", "ASCENDING"):
        assert cite in text, cite
    csrc = os.path.dirname(build.__file__)
    for src in ("gps_refer.hip", "gps_obj_select_pred.hip"):                   # Box / iou are stated once
        body = open(os.path.join(csrc, src)).read()
        assert '#include "gps_box_dev.h"' in body and "struct Box" not in body, src
    for src in ("gps_obj_select.hip", "gps_obj_select_pred.hip"):              # ... and so are the compaction and the rank loop
        body = open(os.path.join(csrc, src)).read()
        assert '#include "gps_rows_dev.h"' in body and "ulonglong2" not in body and "__ballot(kept)" not in body, src


def test_cases_contain_what_they_claim():
    C.check_construction()
    assert list({3, 9}) == [9, 3]                                              # the set order the reference's block takes
    case = C.CASES[1]
    g = gold(case)
    rows = [b for b in range(len(case["rows"])) if g["iou25"][b].sum() == 2 and set(g["sel"][b][:2].tolist()) == {3, 9}]
    assert rows and all(g["sel"][b][:2].tolist() == [9, 3] for b in rows)      # the reference has them as 9, 3
    mine = C.restate_case(case, order=g["order"])
    assert all(mine["row_obj"][b][:2].tolist() == [3, 9] for b in rows)        # ... this library ascending


@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_restatement_equals_the_reference(case):
    g = gold(case)
    got = C.restate_case(case, order=g["order"])
    assert g["order"].shape == (len(case["rows"]), case["M"])
    for b in range(len(case["rows"])):
        assert C.compare_with_reference(got, g, b, case["M"]) == [], (case["name"], b)
        k = int(g["iou25"][b].sum())                                            # tgt_slot: the last slot of the block
        want = -1 if k == 0 else (k - 1 if len(case["rows"][b]["props"]) > case["M"] else int(np.flatnonzero(g["iou25"][b])[-1]))
        assert got["tgt_slot"][b] == want


def test_the_label_map_and_tgt_label_matter():
    case = next(c for c in C.CASES if c["name"] == "pred_M5_map")
    plain = C.restate_case(dict(case, label_map=None), order=gold(case)["order"])
    assert not np.array_equal(plain["is_multiple"], gold(case)["is_multiple"])
    assert np.array_equal(plain["is_hard"], gold(case)["is_hard"])
    case = next(c for c in C.CASES if c["name"] == "pred_M5_tgtlabel")
    own = dict(case, rows=[dict(r, tgt_label=None) for r in case["rows"]])
    assert not np.array_equal(C.restate_case(own, order=gold(case)["order"])["row_obj"], gold(case)["sel"])


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_gives_a_permutation_of_remained(case):
    seed = (5 << 60) + 17
    got = C.restate_case(case, seed=seed)
    for b, row in enumerate(case["rows"]):
        n_rem, n = int(got["n_rem"][b]), int(got["n_sel"][b])
        o = C.device_order(seed, b, n_rem)
        assert sorted(o.tolist()) == list(range(n_rem))
        assert np.array_equal(o, rows_cases.device_order(seed, b, n_rem))       # one law for both selections
        sel = got["row_obj"][b][:n]
        assert len(set(sel.tolist())) == n and (sel >= 0).all() and (sel < len(row["props"])).all()
        assert (got["row_obj"][b][n:] == -1).all()
        if n_rem:
            assert n == case["M"]
    again, other = C.restate_case(case, seed=seed), C.restate_case(case, seed=seed + 1)
    assert np.array_equal(again["row_obj"], got["row_obj"])
    if (got["n_rem"] > 1).any():
        assert not np.array_equal(other["row_obj"], got["row_obj"])
    for k in ("n_rem", "iou25", "tgt_slot", "is_hard"):
        assert np.array_equal(other[k], got[k]), k


# ---- the C entries' checks ------------------------------------------------------------------------------------------------
def _call(lib, **kw):
    """gps_obj_select_pred with a valid argument set (non-NULL stand-in addresses: nothing is launched when a check fails
    first) in which the named arguments are replaced."""
    a = dict(B=2, O=80, M=79, n_objects=100, n_labels=12, boxes=16, labels=16, match_labels=16, scan_range=16, prop_range=16,
             tgt_obj=16, tgt_label=None, label_map=None, order=None, R=0, seed=0, seed_dev=None, row_obj=16, tgt_slot=16,
             n_sel=16, n_rem=16, is_multiple=16, is_hard=16, iou25=None, iou50=None, tgt_id=None, obj_labels=None, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return lib.gps_obj_select_pred(*a.values())


def test_argument_checks_come_before_any_launch():
    lib = _native.load()
    OK, INVALID, UNSUPPORTED = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT, _native.GPS_ERR_UNSUPPORTED
    for bad in (dict(B=-1), dict(O=-1), dict(n_objects=-1), dict(n_labels=-1), dict(R=-1), dict(M=0), dict(M=-3), dict(M=81),
                dict(order=16, R=78), dict(order=16, R=0), dict(boxes=None), dict(labels=None), dict(match_labels=None),
                dict(scan_range=None), dict(prop_range=None), dict(tgt_obj=None), dict(row_obj=None), dict(tgt_slot=None),
                dict(n_sel=None), dict(n_rem=None), dict(is_multiple=None), dict(is_hard=None), dict(iou25=16),
                dict(iou25=16, iou50=16, tgt_id=16), dict(obj_labels=16), dict(iou50=16, tgt_id=16, obj_labels=16)):
        assert _call(lib, **bad) == INVALID, bad
    assert _call(lib, M=1, O=1) == UNSUPPORTED and _call(lib, M=1, O=2) == UNSUPPORTED
    assert _call(lib, O=513) == UNSUPPORTED and _call(lib, O=513, M=513) == UNSUPPORTED
    none = dict(boxes=None, labels=None, match_labels=None, scan_range=None, prop_range=None, tgt_obj=None, row_obj=None,
                tgt_slot=None, n_sel=None, n_rem=None, is_multiple=None, is_hard=None)
    assert _call(lib, B=0, **none) == OK
    assert _call(lib, B=0, M=0, **none) == INVALID and _call(lib, B=0, M=1, **none) == UNSUPPORTED
    assert _call(lib, B=0, iou25=16, **none) == INVALID
    # gps_proposal_labels(n_props, n_objects, boxes, labels, prop_id, ann_range, match_labels, stream)
    assert lib.gps_proposal_labels(0, 5, None, None, None, None, None, None) == OK
    assert lib.gps_proposal_labels(-1, 5, 16, 16, 16, 16, 16, None) == INVALID
    assert lib.gps_proposal_labels(3, -1, 16, 16, 16, 16, 16, None) == INVALID
    for k in range(5):
        args = [16] * 5
        args[k] = None
        assert lib.gps_proposal_labels(3, 5, *args, None) == INVALID, k


# ---- the wrapper's refusals, all raised before a device is touched --------------------------------------------------------
def _packed(n_props):
    """Two scans of 4 annotated objects on the CPU; scan s0 has n_props proposals, s1 none (no add_proposals)."""
    p = G.PackedScans("cpu")
    pts, col, inst = np.zeros((4, 3), np.float32), np.zeros((4, 3), np.uint8), np.arange(4)
    for sid in ("s0", "s1"):
        p.add_scan(sid, pts, col, inst, list(range(4)), inst_labels=[3] * 4)
    p.add_proposals("s0", pts, col, np.ones((n_props, 4), bool), [3] * n_props)
    return p.finalize()


def test_wrapper_refusals():
    packed, big = _packed(6), _packed(1025)
    pred = dict(pc_type="pred")
    with pytest.raises(ValueError, match="1025 proposals > 1024"):
        select_rows(big, ["s0"], 5, tgt_obj=[0], **pred)
    with pytest.raises(ValueError, match="no proposals"):
        select_rows(packed, ["s0", "s1"], 5, tgt_obj=[0, 0], **pred)
    with pytest.raises(ValueError, match="no proposals"):
        select_rows(packed, ["s1"], 5, mode="pretrain", keep=G.keep_table(C.INT2CAT), **pred)
    with pytest.raises(ValueError, match="outside its scan"):
        select_rows(packed, ["s0"], 5, tgt_obj=[4], **pred)
    with pytest.raises(ValueError, match="outside its scan"):
        select_rows(packed, ["s0"], 5, tgt_obj=[-1], **pred)
    with pytest.raises(ValueError, match="max_keep"):
        select_rows(packed, ["s0"], 5, O=4, tgt_obj=[0], **pred)
    with pytest.raises(ValueError, match="max_keep >= 2"):
        select_rows(packed, ["s0"], 1, tgt_obj=[0], **pred)
    with pytest.raises(ValueError, match="object slots"):
        select_rows(packed, ["s0"], 5, O=513, tgt_obj=[0], **pred)
    with pytest.raises(ValueError, match="tgt_obj"):
        select_rows(packed, ["s0"], 5, **pred)
    with pytest.raises(ValueError, match="integer positions"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0, 1], **pred)
    with pytest.raises(ValueError, match="tgt_label"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], tgt_label=[3, 3], **pred)
    with pytest.raises(ValueError, match="pc_type"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], pc_type="proposals")
    with pytest.raises(ValueError, match="belong to pc_type='pred'"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], keep=G.keep_table(C.INT2CAT), targets=True)
    with pytest.raises(ValueError, match="belong to pc_type='pred'"):
        select_rows(packed, ["s0"], 5, mode="pretrain", keep=G.keep_table(C.INT2CAT), tgt_label=[3], **pred)
    with pytest.raises(ValueError, match="order"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], order=torch.zeros((1, 4), dtype=torch.int32), **pred)
    with pytest.raises(ValueError, match="pair"):
        select_rows(packed, torch.zeros((1, 2), dtype=torch.int32), 5, tgt_obj=[0], **pred)
    with pytest.raises(RuntimeError, match="no CPU path"):
        select_rows(packed, ["s0"], 5, tgt_obj=[0], targets=True, **pred)
    with pytest.raises(RuntimeError, match="no CPU path"):
        select_rows(packed, ["s0"], 5, mode="pretrain", keep=G.keep_table(C.INT2CAT), **pred)
    with pytest.raises(RuntimeError, match="no CPU path"):
        G.proposal_labels(packed)
    with pytest.raises(RuntimeError, match="finalize"):
        select_rows(G.PackedScans("cpu"), [], 5, tgt_obj=[], **pred)
    assert packed.match_labels is None                                         # a device product, like the boxes
    # batch_rows still refuses the over-long proposal scan, and now names what takes it
    with pytest.raises(ValueError, match=r'> max_obj_len 5; select_rows\(pc_type="pred"\)'):
        G.batch_rows(packed, ["s0"], 5, proposals=True)
    assert G.scan_ranges(packed, ["s0"], proposals=True).tolist() == [[8, 14]]
    assert G.scan_ranges(packed, ["s1", "s0"]).tolist() == [[4, 8], [0, 4]]
    with pytest.raises(KeyError):
        G.scan_ranges(packed, ["s1"], proposals=True)
