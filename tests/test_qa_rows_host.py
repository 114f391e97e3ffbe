"""The device-side ScanQA / SQA3D batch on the host: the numpy restatement of tests/qa_rows_cases.py against the reference's
own outputs (tests/golden/qa_rows_ref.npz, written by tests/golden/make_golden_qa_rows.py), bit for bit; the emulated
device law; the export and the argument checks of gps_obj_select_qa, which come before any launch; and the wrapper's
host-side refusals.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import qa_rows_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data import gpu_qa as Q  # noqa: E402
from sceneverse_amd.data.gpu_qa import PackedQuestions, qa_rows  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "qa_rows_ref.npz"))
KEYS = ("row_obj", "n_sel", "n_rem", "order", "pick", "sqa_type", "obj_labels", "tgt_object_id", "tgt_object_label", "answer_label")


def gold(case):
    return {k: GOLD[f"{case['name']}/{k}"] for k in KEYS}


def test_entry_is_declared_bound_and_built():
    lib = _native.load()
    name = "gps_obj_select_qa"
    assert name in _native.declared_symbols() and name in _native.SIGNATURES and hasattr(lib, name)
    assert lib.gps_abi_version() == 11                                         # additive: the ABI number does not move
    from sceneverse_amd.csrc import build
    assert ("gps_obj_select_qa.hip", ["-ffp-contract=off"]) in build.SOURCES
    text = open(_native.HEADER_PATH).read()
    for cite in ("scannet_old.py:326-484", "scannet_old.py:94-232", "GPS_QA_MAX_TGT 32", "S + 4", "unkept targets",
                 "repeated targets", "k > M", "EMPTY rows"):
        assert cite in text, cite
    assert (_native.QA_MAX_TGT, _native.QA_PRED, _native.QA_MATCHED, _native.QA_TRAIN, _native.QA_INT64) == (32, 1, 2, 4, 8)
    body = open(os.path.join(os.path.dirname(build.__file__), "gps_obj_select_qa.hip")).read()
    assert '#include "gps_box_dev.h"' in body and '#include "gps_rows_dev.h"' in body      # Box / iou, compaction, fill law: stated once
    assert "struct Box" not in body and "ulonglong2" not in body


def test_cases_contain_what_they_claim():
    share, n_rows = C.check_construction()
    assert share <= 0.25 and n_rows == sum(len(c["rows"]) for c in C.CASES)
    for c in C.CASES:                            # ref=False only for the four definitions and out-of-range ids
        assert c["ref"] or c["name"].endswith("_odd")
    assert {c["O"] - c["M"] for c in C.CASES} == {0, 1}


@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_restatement_equals_the_reference(case):
    g = gold(case)
    B = len(case["rows"])
    assert g["order"].shape == (B, case["M"]) and g["row_obj"].shape == (B, case["O"])
    got = C.restate_case(case, order=g["order"], pick=g["pick"])
    for k in C.OUT_KEYS:
        if k != "n_tgt":
            assert np.array_equal(got[k], g[k]), (case["name"], k, np.flatnonzero((got[k] != g[k]).reshape(B, -1).any(1)))
    if case["kind"] == "sqa3d":                  # no target ever: the pad slot behind the row, class 5
        assert (got["n_tgt"] == 0).all() and (g["tgt_object_label"].sum(1) == 1).all() and g["tgt_object_label"][:, 5].all()
        slot = np.minimum(g["n_sel"], case["O"] - 1)
        assert (g["tgt_object_id"][np.arange(B), slot] == (g["n_sel"] < case["O"])).all()


def test_the_pick_and_the_per_variant_keep_matter():
    case = next(c for c in C.CASES if c["name"] == "sqa_gt_M5_lang")
    g = gold(case)
    assert len(set(g["pick"].tolist())) > 1
    first = C.restate_case(case, order=g["order"], pick=np.zeros_like(g["pick"]))
    assert not np.array_equal(first["n_sel"], g["n_sel"]) or not np.array_equal(first["row_obj"], g["row_obj"])
    got = C.restate_case(case, order=g["order"], pick=g["pick"])
    vf = C.var_first(case)
    assert np.array_equal(got["sent_idx"], vf[:-1] + g["pick"])


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_gives_a_permutation_of_remained(case):
    seed = (5 << 60) + 17
    got = C.restate_case(case, seed=seed)
    for b, row in enumerate(case["rows"]):
        n_rem, n = int(got["n_rem"][b]), int(got["n_sel"][b])
        assert sorted(C.device_order(seed, b, n_rem).tolist()) == list(range(n_rem))
        sel = got["row_obj"][b][:n]
        assert len(set(sel.tolist())) == n and (sel >= 0).all() and (sel < max(len(row["scan"][1]), 1)).all()
        assert (got["row_obj"][b][n:] == -1).all()
        if n_rem:
            assert n == case["M"]
        assert 0 <= C.device_pick(seed, b, len(row["texts"])) < len(row["texts"])
    again, other = C.restate_case(case, seed=seed), C.restate_case(case, seed=seed + 1)
    assert all(np.array_equal(again[k], got[k]) for k in got)
    if (got["n_rem"] > 1).any():
        assert not np.array_equal(other["row_obj"], got["row_obj"])
    drawn_keep = case["lang"] and case["kind"] == "sqa3d"                      # the pick chooses the keep row there
    for k in ("n_tgt", "answer_label", "sqa_type") + (() if drawn_keep else ("n_rem", "n_sel")):
        assert np.array_equal(other[k], got[k]), k
    if case["kind"] == "sqa3d" and case["name"] != "sqa_pred_M5":
        picks = [C.device_pick(s, b, 3) for s in range(seed, seed + 4) for b in range(8)]
        assert set(picks) == {0, 1, 2}


# ---- the C entry's checks -------------------------------------------------------------------------------------------------
def _table(**kw):
    a = dict(nq=3, n_tgt=4, n_ans=5, n_var=3, ann_range=16, prop_range=16, tgt_first=16, tgt_id=16, tgt_label=16, ans_first=16,
             ans_id=16, sqa_type=16, var_first=16, var_text=16)
    assert set(kw) <= set(a)
    a.update(kw)
    return _native.QAQuestions(*a.values())


def _call(lib, table=None, **kw):
    """gps_obj_select_qa with a valid argument set (non-NULL stand-in addresses: nothing is launched when a check fails
    first) in which the named arguments are replaced."""
    table = _table() if table is None else table
    a = dict(B=2, O=80, M=79, A=100, n_objects=100, n_labels=607, flags=_native.QA_MATCHED,
             questions=ctypes.byref(table) if table is not False else None, q_idx=16, boxes=16, labels=16, match_labels=16,
             keep=16, keep_rows=0, order=None, R=0, pick=None, seed=0, seed_dev=None, row_obj=16, n_sel=16, n_rem=16, n_tgt=16,
             sent_idx=16, sqa_type=16, obj_labels=16, tgt_object_id=16, tgt_object_label=16, answer_label=16, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return lib.gps_obj_select_qa(*a.values())


def test_argument_checks_come_before_any_launch():
    lib = _native.load()
    OK, INVALID, UNSUPPORTED = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT, _native.GPS_ERR_UNSUPPORTED
    pred = _native.QA_PRED | _native.QA_MATCHED
    for bad in (dict(B=-1), dict(O=-1), dict(A=-1), dict(n_objects=-1), dict(n_labels=-1), dict(keep_rows=-1), dict(R=-1),
                dict(M=0), dict(M=-3), dict(M=81), dict(order=16, R=78), dict(order=16, R=0), dict(flags=16), dict(flags=-1),
                dict(q_idx=None), dict(labels=None), dict(match_labels=None), dict(keep=None), dict(row_obj=None),
                dict(n_sel=None), dict(n_rem=None), dict(n_tgt=None), dict(sent_idx=None), dict(sqa_type=None),
                dict(obj_labels=None), dict(tgt_object_id=None), dict(tgt_object_label=None), dict(answer_label=None), dict(flags=pred, boxes=None)):
        assert _call(lib, **bad) == INVALID, bad
    assert _call(lib, table=False) == INVALID
    for bad in (dict(nq=-1), dict(n_tgt=-1), dict(n_ans=-1), dict(n_var=-1), dict(ann_range=None), dict(tgt_first=None),
                dict(tgt_id=None), dict(tgt_label=None), dict(ans_first=None), dict(ans_id=None), dict(sqa_type=None),
                dict(var_first=None), dict(var_text=None)):
        assert _call(lib, table=_table(**bad)) == INVALID, bad
    assert _call(lib, table=_table(prop_range=None), flags=pred) == INVALID
    assert _call(lib, O=513) == UNSUPPORTED and _call(lib, O=513, M=513) == UNSUPPORTED
    none = dict(q_idx=None, boxes=None, labels=None, match_labels=None, keep=None, row_obj=None, n_sel=None, n_rem=None,
                n_tgt=None, sent_idx=None, sqa_type=None, obj_labels=None, tgt_object_id=None, tgt_object_label=None, answer_label=None)
    assert _call(lib, B=0, **none) == OK
    assert _call(lib, B=0, M=1, O=1, **none) == OK                             # M = 1 is a row of one object: defined here
    assert _call(lib, B=0, M=0, **none) == INVALID and _call(lib, B=0, O=513, **none) == UNSUPPORTED


# ---- the wrapper's refusals, all raised before a device is touched --------------------------------------------------------
def _packed(n_objects=4, n_props=6):
    """Two scans on the CPU; s0 has n_props proposals, s1 none."""
    p = G.PackedScans("cpu")
    for sid in ("s0", "s1"):
        n = n_objects if sid == "s0" else 4
        pts, col = np.zeros((n, 3), np.float32), np.zeros((n, 3), np.uint8)
        pts[:, 0] = np.arange(n)
        p.add_scan(sid, pts, col, np.arange(n), list(range(n)), inst_labels=[3] * n)
    pts, col = np.zeros((n_objects, 3), np.float32), np.zeros((n_objects, 3), np.uint8)
    p.add_proposals("s0", pts, col, np.ones((n_props, n_objects), bool), [3] * n_props)
    return p.finalize()


def _questions(packed):
    q = PackedQuestions("cpu")
    assert q.add_question("s0", [1, 0], [5, -100, 7], texts=[4, 9, 2], sqa_type=3) == 0
    assert q.add_question("s1", [], [], texts=11) == 1
    return q.finalize(packed)


def test_packed_questions_tables():
    q = _questions(_packed())
    assert q.n_questions == 2 and q.n_variants == 4
    assert q.ann_range.tolist() == [[0, 4], [4, 8]] and q.prop_range.tolist() == [[8, 14], [0, 0]]
    assert q.tgt_first.tolist() == [0, 2, 2] and q.tgt_id.tolist() == [1, 0] and q.tgt_label.tolist() == [3, 3]
    assert q.ans_first.tolist() == [0, 2, 2] and q.ans_id.tolist() == [5, 7]   # the id < 0 is dropped, as stoi(..) >= 0 does
    assert q.var_first.tolist() == [0, 3, 4] and q.var_text.tolist() == [4, 9, 2, 11] and q.sqa_type.tolist() == [3, 0]
    assert all(t.dtype == torch.int32 for t in (q.ann_range, q.tgt_id, q.ans_first, q.var_text, q.sqa_type))
    p = _packed()
    for bad, match in ((dict(targets=[4]), "outside scan"), (dict(targets=[-1]), "outside scan")):
        qq = PackedQuestions("cpu")
        qq.add_question("s0", texts=0, **bad)
        with pytest.raises(ValueError, match=match):
            qq.finalize(p)
    qq = PackedQuestions("cpu")
    with pytest.raises(ValueError, match="targets > 32"):
        qq.add_question("s0", list(range(33)))
    with pytest.raises(ValueError, match="one label per target"):
        qq.add_question("s0", [0, 1], tgt_labels=[3])
    with pytest.raises(ValueError, match="at least one text"):
        qq.add_question("s0", texts=[])
    with pytest.raises(ValueError, match="sqa_type"):
        qq.add_question("s0", sqa_type=6)
    with pytest.raises(RuntimeError, match="finalize"):
        qq.finalize(G.PackedScans("cpu"))


def test_wrapper_refusals():
    packed = _packed()
    q = _questions(packed)
    keep = G.keep_table(C.INT2CAT)
    with pytest.raises(ValueError, match="pc_type"):
        qa_rows(packed, q, [0], 5, keep=keep, pc_type="proposals")
    with pytest.raises(ValueError, match="max_keep"):
        qa_rows(packed, q, [0], 5, O=4, keep=keep)
    with pytest.raises(ValueError, match="max_keep"):
        qa_rows(packed, q, [0], 0, keep=keep)
    with pytest.raises(ValueError, match="object slots"):
        qa_rows(packed, q, [0], 5, O=513, keep=keep)
    with pytest.raises(ValueError, match="n_answers"):
        qa_rows(packed, q, [0], 5, n_answers=-1, keep=keep)
    with pytest.raises(ValueError, match="keep is required"):
        qa_rows(packed, q, [0], 5)
    with pytest.raises(ValueError, match="keep must be"):
        qa_rows(packed, q, [0], 5, keep=keep.float())
    with pytest.raises(ValueError, match="one per variant"):
        qa_rows(packed, q, [0], 5, keep=keep[None].repeat(3, 1))
    with pytest.raises(ValueError, match="width of keep"):
        qa_rows(packed, q, [0], 5, keep=keep, n_labels=12)
    with pytest.raises(ValueError, match="question number outside"):
        qa_rows(packed, q, [2], 5, keep=keep)
    with pytest.raises(ValueError, match="question number outside"):
        qa_rows(packed, q, [-1], 5, keep=keep)
    with pytest.raises(ValueError, match="q_idx must hold"):
        qa_rows(packed, q, [0.5], 5, keep=keep)
    with pytest.raises(ValueError, match="no proposals"):
        qa_rows(packed, q, [0, 1], 5, pc_type="pred")
    with pytest.raises(ValueError, match="order"):
        qa_rows(packed, q, [0], 5, keep=keep, order=torch.zeros((1, 4), dtype=torch.int32))
    with pytest.raises(ValueError, match="pick must hold"):
        qa_rows(packed, q, [0], 5, keep=keep, pick=[0, 1])
    with pytest.raises(ValueError, match="pick outside"):
        qa_rows(packed, q, [0, 1], 5, keep=keep, pick=[2, 1])
    big = _packed(n_objects=1025, n_props=1025)
    with pytest.raises(ValueError, match="1025 objects > 1024"):
        qa_rows(big, _questions(big), [0], 5, keep=keep)
    with pytest.raises(ValueError, match="1025 proposals > 1024"):
        qa_rows(big, _questions(big), [0], 5, pc_type="pred")
    with pytest.raises(RuntimeError, match="no CPU path"):
        qa_rows(packed, q, [0, 1], 5, keep=keep, pick=[2, 0])
    with pytest.raises(RuntimeError, match="no CPU path"):
        qa_rows(packed, q, [0], 5, pc_type="pred")
    with pytest.raises(RuntimeError, match="finalize"):
        qa_rows(packed, PackedQuestions("cpu"), [], 5, keep=keep)
    assert Q.QA_MAX_TGT == 32 and Q.N_LABELS_607 == 607


def test_synth_packed_questions():
    from sceneverse_amd.data.synthetic import synth_packed_questions
    packed = _packed(n_objects=9)
    q = synth_packed_questions(packed, ["s0", "s1"], 40, n_texts=17, seed=3)
    assert q.n_questions == 40 and 40 <= q.n_variants <= 120
    assert int(q.var_text.max()) < 17 and int(q.ans_id.max()) < 8864 and set(q.sqa_type.tolist()) <= set(range(6))
    k = np.diff(q.tgt_first.numpy())
    assert k.min() == 0 and k.max() == 3
    for i in range(40):                          # every target inside its question's scan
        t = q.tgt_id[q.tgt_first[i]:q.tgt_first[i + 1]]
        assert ((t >= q.ann_range[i, 0]) & (t < q.ann_range[i, 1])).all() and len(set(t.tolist())) == len(t)
