"""The answer-accuracy evaluators on the host: the two entries of libgps_hip.so (gps_answer_hits, gps_answer_fold) are
declared, bound and exported and check their arguments before any HIP call; the counters refuse CPU tensors; the
pure-torch oracle of the ranking law in tests/answers_cases.py, with the evaluators' arithmetic on top, equals the
reference's own results (tests/golden/answers_ref.npz, written by tests/golden/make_golden_answers.py) EXACTLY -- which
pins the oracle the GPU tests use to the reference; and one tie, worked out by hand, where torch.topk and the law
differ.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import answers_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "answers_ref.npz"))
OK, INVALID = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT


def test_entries_are_declared_bound_and_exported():
    lib = _native.load()
    declared = _native.declared_symbols()
    for name in ("gps_answer_hits", "gps_answer_fold"):
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.gps_abi_version() == 11                   # additive: the ABI number does not move
    text = open(_native.HEADER_PATH).read()
    for macro, value in (("MAX_K", _native.ANSWER_MAX_K), ("MAX_TYPES", _native.ANSWER_MAX_TYPES),
                         ("WORDS", _native.ANSWER_WORDS), ("WAVE_MAX_COLS", _native.ANSWER_WAVE_MAX_COLS),
                         ("FOLD_MAX_CLS", _native.ANSWER_FOLD_MAX_CLS)):
        assert f"#define GPS_ANSWER_{macro} {value}" in text
    assert "#define GPS_HIP_ABI_VERSION 11" in text
    # the header's struct, field for field on an LP64 target
    A = _native.AnswerHitsArgs
    assert ctypes.sizeof(A) == 88 and A.ld.offset == 16 and A.label.offset == 32 and A.type.offset == 48
    assert A.k.offset == 60 and A.rows_dev.offset == 64 and A.words.offset == 80


def _args(**kw):
    """Well-formed arguments over made-up (never dereferenced) addresses, with overrides."""
    f = dict(rows=4, cols=80, scores=4096, ld=80, scores_bf16=0, label_kind=0, label=8192, ld_label=80, type=None,
             n_types=0, k=10, rows_dev=None, topk=None, words=16384)
    f.update(kw)
    return _native.AnswerHitsArgs(**f)


def _hits(**kw):
    return _native.load().gps_answer_hits(ctypes.byref(_args(**kw)), None)


def test_answer_hits_argument_checks_come_before_any_hip_call():
    assert _native.load().gps_answer_hits(None, None) == INVALID
    for bad in (dict(scores=None), dict(label=None), dict(words=None), dict(k=0), dict(k=17), dict(k=-1), dict(ld=79),
                dict(ld_label=79), dict(n_types=9), dict(n_types=-1), dict(rows=-1), dict(cols=0), dict(label_kind=3),
                dict(scores=4098), dict(scores=4097, scores_bf16=1)):
        assert _hits(**bad) == INVALID, bad
        if "rows" not in bad:                            # checked even when there is nothing to launch
            assert _hits(rows=0, **bad) == INVALID, bad
    # nothing to launch: GPS_OK without a device
    assert _hits(rows=0) == OK
    assert _hits(rows=0, k=16, n_types=8, type=64, cols=8864, ld=8867, ld_label=8864, scores=4098, scores_bf16=1) == OK


def test_answer_fold_argument_checks_come_before_any_hip_call():
    fold = _native.load().gps_answer_fold
    w = ctypes.c_double(16.0)
    assert fold(None, 64, 1, 6, w, None, 8, 8, 8, 8, None) == INVALID            # no words
    assert fold(64, 64, 1, 6, w, None, None, 8, 8, 8, None) == INVALID           # no last
    assert fold(64, None, 1, 6, w, None, 8, 8, 8, 8, None) == INVALID            # n_cls without cls_words
    assert fold(64, 64, 9, 6, w, 8, 8, None, None, None, None) == INVALID        # more than 8 cls rows
    assert fold(64, 64, -1, 6, w, 8, 8, None, None, None, None) == INVALID
    # the float64 form (sums == NULL)
    assert fold(64, 64, 1, 6, w, None, 8, None, 8, 8, None) == INVALID           # no acc
    assert fold(64, 64, 1, 6, w, None, 8, 8, None, 8, None) == INVALID           # no type_total
    assert fold(64, 64, 1, 6, w, None, 8, 8, 8, None, None) == INVALID           # no total
    assert fold(64, 64, 2, 6, w, None, 8, 8, 8, 8, None) == INVALID              # one obj_cls_raw problem at most
    assert fold(64, 64, 1, 9, w, None, 8, 8, 8, 8, None) == INVALID              # more than 8 types
    assert fold(64, 64, 1, 6, ctypes.c_double(0.0), None, 8, 8, 8, 8, None) == INVALID   # B = 0


@pytest.mark.parametrize("name", ["ScanQACounter", "SQA3DCounter"])
def test_counters_refuse_cpu_tensors(name):
    from sceneverse_amd import engine
    c = getattr(engine, name)("cpu")
    with pytest.raises(RuntimeError, match="no CPU path"):
        c.update(C.batch("scanqa" if name == "ScanQACounter" else "sqa3d", 1))
    c.reset()
    assert c.result() == {} and c.last() == {}
    with pytest.raises(RuntimeError, match="topk=True"):
        c.last_topk()
    assert getattr(engine, name)("cpu", topk=True).last_topk() is None


# ---- the oracle of the law against the reference ----------------------------------------------------------------------
def test_fixture_covers_the_cases_it_claims():
    assert C.SIZES == (16, 7, 33) and C.V == {"scanqa": 8864, "sqa3d": 706}
    types = [set(C.batch("sqa3d", i)["sqa_type"].tolist()) for i in range(3)]
    assert all(4 not in s for s in types)                                   # one type never occurs
    assert [3 in s for s in types] == [True, False, True]                   # one type is absent from one batch only
    for task in C.V:
        for i in range(3):
            d = C.batch(task, i)
            assert d["answer_scores"].dtype == torch.float32
            assert bool((d["answer_label"].sum(1) == 0).any())              # some rows are unanswerable
            assert bool(C.tie_free(d["answer_scores"]).all())               # the reference is a valid oracle here
            # ... and stays one on the bf16 grid
            assert bool(C.tie_free(d["answer_scores"].to(torch.bfloat16).float()).all())
            # tie-free: torch.topk has no choice left
            assert torch.equal(torch.topk(d["answer_scores"], C.K, -1)[1], C.ranked(d["answer_scores"])[:, :C.K])
    assert GOLD["sqa3d/0/type_count"][4] == 1e-10 and GOLD["sqa3d/1/type_count"][3] == 1e-10
    assert GOLD["sqa3d/0/type_count"][3] > 1


def test_scanqa_oracle_reproduces_the_reference_exactly():
    keys = C.SCANQA_KEYS
    assert tuple(GOLD["scanqa/keys"].tolist()) == keys
    batches = [C.batch("scanqa", i) for i in range(3)]
    for i, d in enumerate(batches):
        pairs = C.scanqa_pairs(d)
        assert tuple(pairs) == keys
        got = np.asarray([pairs[k] for k in keys], dtype=np.int64)
        assert np.array_equal(got, GOLD[f"scanqa/{i}/pairs"]), (i, got)
        assert np.array_equal(C.as_array({k: h / max(c, 1) for k, (h, c) in pairs.items()}, keys),
                              GOLD[f"scanqa/{i}/metrics"])
    assert np.array_equal(C.as_array(C.scanqa_record(batches), keys), GOLD["scanqa/record"])


def test_sqa3d_oracle_reproduces_the_reference_exactly():
    keys = C.SQA_KEYS
    assert tuple(GOLD["sqa3d/keys"].tolist()) == keys
    batches = [C.batch("sqa3d", i) for i in range(3)]
    for i, d in enumerate(batches):
        m = C.sqa3d_metrics(d)
        assert np.array_equal(C.as_array(m, keys), GOLD[f"sqa3d/{i}/metrics"]), i
        assert np.array_equal(C.as_array(m, [f"type{t}_count" for t in range(C.N_TYPES)]), GOLD[f"sqa3d/{i}/type_count"])
    assert np.array_equal(C.as_array(C.sqa3d_record(batches), keys), GOLD["sqa3d/record"])


# ---- why the law exists --------------------------------------------------------------------------------------------------
def test_a_tie_where_torch_topk_and_the_law_differ():
    """scores [1, 3, 3, 2, 3, 0], k = 2.  By hand: the greatest value 3 sits in columns 1, 2 and 4; the law takes the
    lower columns first, so the two best are [1, 2] and place 0 is torch.argmax's answer 1.  torch.topk on the CPU
    returns two columns holding 3 as well -- but not those two, and not starting at the arg-max: with the label on
    column 1, `ans1` (argmax) counts a hit that the reference's own top-2 misses."""
    x = torch.tensor([[1.0, 3.0, 3.0, 2.0, 3.0, 0.0]])
    assert int(torch.argmax(x, dim=-1)) == 1
    law = C.topk_ids(x, 2)[0].tolist()
    assert law == [1, 2]
    ids = torch.topk(x, 2, -1)[1][0].tolist()
    assert x[0, ids].tolist() == [3.0, 3.0]                                 # a valid top-2 by value ...
    assert ids != law                                                       # ... that is not the law's
    label = torch.tensor([[0, 1, 0, 0, 0, 0]])
    assert C.words(x, label, k=2)[:3] == [1, 1, 1]                          # hit at place 0, so among the two best too
    # the three sort keys: NaN is above +inf and does not tie with it; -0.0 == +0.0 keep their columns' order
    y = torch.tensor([[float("inf"), float("nan"), -0.0, 0.0, float("nan"), float("-inf")]])
    assert C.ranked(y)[0].tolist() == [1, 4, 0, 2, 3, 5]
