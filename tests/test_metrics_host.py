"""The device-side evaluators on the host: the two entries of libgps_hip.so (gps_cls_hits, gps_metrics_fold) are declared,
bound and exported and check their arguments before any launch; the counters refuse CPU tensors; the float64
restatement of fold + record in tests/metrics_cases.py equals the reference's own results
(tests/golden/metrics_ref.npz, written by tests/golden/make_golden_metrics.py) EXACTLY -- which pins the order of
operations before any GPU is involved.  No GPU."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import metrics_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "metrics_ref.npz"))
ENTRIES = ("gps_cls_hits", "gps_metrics_fold")
OK, INVALID, UNSUPPORTED = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT, _native.GPS_ERR_UNSUPPORTED


def test_entries_are_declared_bound_and_exported():
    lib = _native.load()
    declared = _native.declared_symbols()
    for name in ENTRIES:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.gps_abi_version() == 11                   # additive: the ABI number does not move
    text = open(_native.HEADER_PATH).read()
    assert f"#define GPS_CLS_HITS_WAVE_MAX_COLS {_native.CLS_HITS_WAVE_MAX_COLS}" in text
    assert f"#define GPS_CLS_HITS_MAX_PROBLEMS {_native.CLS_HITS_MAX_PROBLEMS}" in text
    assert f"#define GPS_METRICS_MAX_TERMS {_native.METRICS_MAX_TERMS}" in text
    assert "#define GPS_HIP_ABI_VERSION 11" in text
    from sceneverse_amd.csrc import build
    assert ("gps_metrics.hip", ["-ffp-contract=off"]) in build.SOURCES


def _problem(**kw):
    """A well-formed problem over made-up (never dereferenced) addresses, with overrides."""
    f = dict(rows=4, cols=80, logits=4096, ld=80, logits_bf16=0, use_ignore=0, ignore_index=0, labels=8192, rows_dev=None,
             sel=None, split_a=None, split_b=None, mask_elem_bytes=1, reserved=0, counters=16384)
    f.update(kw)
    return _native.ClsHitsProblem(**f)


def _hits(*problems, n=None):
    arr = (_native.ClsHitsProblem * max(len(problems), 1))(*problems)
    return _native.load().gps_cls_hits(arr, len(problems) if n is None else n, None)


def test_cls_hits_argument_checks_come_before_any_launch():
    lib = _native.load()
    assert lib.gps_cls_hits(None, 0, None) == OK                         # nothing to do
    assert lib.gps_cls_hits(None, 1, None) == INVALID
    assert _hits(_problem(), n=-1) == INVALID
    assert _hits(_problem(rows=-1)) == INVALID
    assert _hits(_problem(cols=-1)) == INVALID
    assert _hits(_problem(cols=0)) == INVALID
    assert _hits(_problem(ld=79)) == INVALID                             # pitch < cols
    assert _hits(_problem(logits=None)) == INVALID
    assert _hits(_problem(labels=None)) == INVALID
    assert _hits(_problem(counters=None)) == INVALID
    assert _hits(_problem(mask_elem_bytes=4)) == INVALID
    assert _hits(_problem(mask_elem_bytes=0)) == INVALID
    assert _hits(_problem(logits=4098)) == INVALID                       # fp32 rows must start on a 4-byte boundary
    assert _hits(_problem(logits=4097, logits_bf16=1)) == INVALID
    assert _hits(_problem(rows=0), _problem(rows=4, ld=8)) == INVALID    # every problem is checked
    assert _hits(*[_problem(rows=0)] * 9) == UNSUPPORTED                 # more than 8 problems
    # every rows == 0: GPS_OK without a launch (there is no device here to launch on)
    assert _hits(_problem(rows=0)) == OK
    assert _hits(*[_problem(rows=0, logits=None, labels=None, counters=None, cols=30522, ld=30528)] * 8) == OK


def test_metrics_fold_argument_checks_come_before_any_launch():
    lib = _native.load()
    T = _native.MetricTerm
    terms = (T * 17)(*[T(hits=64, count=128, eps=1e-8) for _ in range(17)])
    w = ctypes.c_double(3.0)
    assert lib.gps_metrics_fold(-1, terms, w, 0, 8, 8, 8, None) == INVALID
    assert lib.gps_metrics_fold(2, terms, w, 3, 8, 8, 8, None) == INVALID        # the mean covers more than the terms
    assert lib.gps_metrics_fold(2, terms, w, -1, 8, 8, 8, None) == INVALID
    assert lib.gps_metrics_fold(17, terms, w, 2, 8, 8, 8, None) == UNSUPPORTED
    assert lib.gps_metrics_fold(2, None, w, 2, 8, 8, 8, None) == INVALID
    assert lib.gps_metrics_fold(2, terms, w, 2, None, 8, 8, None) == INVALID
    assert lib.gps_metrics_fold(2, terms, w, 2, 8, None, 8, None) == INVALID
    assert lib.gps_metrics_fold(2, terms, w, 2, 8, 8, None, None) == INVALID
    bad = (T * 2)(T(hits=None, count=128), T(hits=64, count=128))
    assert lib.gps_metrics_fold(2, bad, w, 2, 8, 8, 8, None) == INVALID          # a term without a hits word
    bad = (T * 2)(T(hits=64, count=None), T(hits=64, count=128))
    assert lib.gps_metrics_fold(2, bad, w, 2, 8, 8, 8, None) == INVALID          # no count and no constant denominator


def test_struct_layouts_match_the_header():
    # the header's structs, field for field on an LP64 target: natural alignment, no packing
    assert ctypes.sizeof(_native.ClsHitsProblem) == 96 and _native.ClsHitsProblem.counters.offset == 88
    assert _native.ClsHitsProblem.ld.offset == 16 and _native.ClsHitsProblem.labels.offset == 40
    assert ctypes.sizeof(_native.MetricTerm) == 56 and _native.MetricTerm.eps.offset == 32


@pytest.mark.parametrize("name", ["PretrainCounter", "ReferIt3DCounter", "ObjClsCounter"])
def test_counters_refuse_cpu_tensors(name):
    from sceneverse_amd import engine
    c = getattr(engine, name)("cpu")
    seq = {"PretrainCounter": "pre", "ReferIt3DCounter": "referit", "ObjClsCounter": "objcls"}[name]
    with pytest.raises(RuntimeError, match="no CPU path"):
        c.update(C.batch(seq, 0))
    c.reset()
    if name == "ReferIt3DCounter":
        assert c.result() == {} and c.result(include_count=True) == {}
    elif name == "ObjClsCounter":
        assert c.result(include_count=True) == {"accuracy": (0, 0)} and c.result() == {"accuracy": 0.0}
    else:
        assert c.result() == {} and c.last() == {}
        with pytest.raises(ValueError):
            engine.PretrainCounter("cpu", keys=["og_accuracy"])


def test_train_step_without_metrics_has_no_counter():
    import inspect
    from sceneverse_amd.engine import GPSTrainStep
    assert inspect.signature(GPSTrainStep.__init__).parameters["train_metrics"].default is False


@pytest.mark.parametrize("seq", C.PRETRAIN)
def test_pretrain_restatement_reproduces_the_reference_exactly(seq):
    keys, sizes = C.SEQUENCES[seq]
    assert tuple(GOLD[f"{seq}/keys"].tolist()) == tuple(keys)
    per_batch, record = C.pretrain_record(seq)
    for i, r in enumerate(per_batch):
        got = np.asarray([r[k] for k in keys], dtype=np.float64)
        assert np.array_equal(got, GOLD[f"{seq}/{i}/metrics"]), (seq, i, got, GOLD[f"{seq}/{i}/metrics"])
    got = np.asarray([record[k] for k in keys], dtype=np.float64)
    assert np.array_equal(got, GOLD[f"{seq}/record"]), (seq, got, GOLD[f"{seq}/record"])


@pytest.mark.parametrize("seq", ["referit", "perscene", "objcls"])
def test_count_restatement_reproduces_the_reference_exactly(seq):
    keys, sizes = C.SEQUENCES[seq]
    assert tuple(GOLD[f"{seq}/keys"].tolist()) == tuple(keys)
    total = np.zeros((len(keys), 2), dtype=np.int64)
    for i in range(len(sizes)):
        pairs = C.count_pairs(seq, i)
        assert tuple(sorted(pairs)) == tuple(sorted(keys))
        got = np.asarray([pairs[k] for k in keys], dtype=np.int64)
        assert np.array_equal(got, GOLD[f"{seq}/{i}/pairs"]), (seq, i)
        assert np.array_equal(got[:, 0] / np.maximum(got[:, 1], 1), GOLD[f"{seq}/{i}/metrics"])
        total += got
    assert np.array_equal(total[:, 0] / np.maximum(total[:, 1], 1), GOLD[f"{seq}/record"])


def test_fixture_covers_the_cases_it_claims():
    W = _native.CLS_HITS_WAVE_MAX_COLS
    assert C.V > W >= C.C and C.O < W                        # the LM rows take the wide schedule, the others the narrow one
    for seq, (keys, sizes) in C.SEQUENCES.items():
        assert len(sizes) >= 3 and len(set(sizes)) == len(sizes), seq      # different B: the weighting shows
    k = list(C.PRE_KEYS)
    # a batch without a labelled token and a batch without a masked object: 0 / 1e-8
    d = C.batch("pre", 1)
    assert int((d["masked_lm_labels"] != -1).sum()) == 0 and GOLD["pre/1/metrics"][k.index("lang_cls_acc_mask")] == 0.0
    d = C.batch("pre", 2)
    assert int((d["obj_masks"] & ~d["obj_sem_masks"]).sum()) == 0
    assert GOLD["pre/2/metrics"][k.index("obj_cls_post_acc_mask")] == 0.0 and GOLD["pre/2/metrics"][k.index("obj_cls_post_acc")] > 0
    # the weighting: record() is not the plain mean of the batch ratios
    plain = np.mean([GOLD[f"pre/{i}/metrics"] for i in range(4)], axis=0)
    assert np.abs(plain - GOLD["pre/record"]).max() > 1e-3
    # tgt_object_id == O never hits; og_acc divides by B without an eps
    d = C.batch("pre", 3)
    assert int(d["tgt_object_id"][1, 0]) == C.O and int(d["obj_masks"][2].sum()) == 0
    assert GOLD["pre/3/metrics"][k.index("og_acc")] in (0.0, 0.25, 0.5, 0.75)
    # the planted rows: tie -> first, all -inf -> 0, NaN -> the first NaN
    d = C.batch("pre", 0)
    lm = d["txt_lm_cls_logits"]
    assert C.argmax_rows(lm[1, :3].numpy()).tolist() == [100, 0, 8] and d["masked_lm_labels"][1, :3].tolist() == [100, 0, 5]
    assert torch.argmax(lm[1, :3], dim=-1).tolist() == [100, 0, 8]
    assert C.argmax_rows(d["obj_cls_post_logits"][0, :3].numpy()).tolist() == [4, 0, 36]
    assert bool(torch.isinf(d["og3d_logits"][0]).all()) and GOLD["pre/0/metrics"][0] == 1.0
    for name, t in d.items():                                # every logit is a bf16 number
        if t.is_floating_point():
            assert torch.equal(t.nan_to_num(nan=0.0), t.to(torch.bfloat16).float().nan_to_num(nan=0.0)), name
    # pre_min has no og_acc / raw / pre keys; referit batch 1 has no hard item; objcls batch 1 has no object
    assert "og_acc" not in C.PRE_MIN_KEYS and "tgt_object_id" not in C.batch("pre_min", 0)
    r = list(C.REFER_KEYS)
    assert GOLD["referit/1/pairs"][r.index("og_acc_hard")].tolist() == [0, 0]
    assert GOLD["objcls/1/pairs"].tolist() == [[0, 0]] and GOLD["objcls/1/metrics"].tolist() == [0.0]
    assert C.batch("perscene", 0)["og3d_logits"].dim() == 3


def test_lazy_margin_premise_holds_for_the_head_the_gpu_test_uses():
    """tests/test_gpu_metrics.py compares the bf16 hit count of the lazy masked-LM path with the arg-max of the fp32
    logits on the rows whose top-two margin exceeds 2^-7 * max(|top1|, |top2|); at least 75 % of its labelled rows must
    be such rows.  The inputs are made on the CPU from a seed: checked here on the fp32 logits alone."""
    head, hidden, labels = C.lazy_case()
    with torch.no_grad():
        logits = head(hidden).reshape(-1, C.LAZY_VOCAB)
    lab = labels.reshape(-1)
    rows = logits[lab != -1]
    clear = C.clear_margin(rows)
    assert len(rows) >= 16 and clear.float().mean().item() >= 0.75, (len(rows), clear.float().mean().item())
