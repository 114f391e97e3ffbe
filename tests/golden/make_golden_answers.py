"""Generate tests/golden/answers_ref.npz by running the REFERENCE's own `ScanQAEval` (evaluator/scanqa_eval.py) and
`SQA3DEval` (evaluator/sqa3d_eval.py) -- imported unmodified from /root/reference, only runnable in the build container
-- on the batches of tests/answers_cases.py (three batches of B = 16, 7, 33; V = 8864 / 706), on the CPU:

  scanqa/keys, sqa3d/keys   the metric names, in the order of the arrays below
  scanqa/<i>/pairs          batch_metrics(batch i, include_count=True) as (hits, count) int64
  scanqa/<i>/metrics        batch_metrics(batch i) as float64
  scanqa/record             BaseEvaluator.record() after update() over the three batches
  sqa3d/<i>/metrics         batch_metrics(batch i) as float64;  sqa3d/<i>/type_count  its type{t}_count
  sqa3d/record              SQA3DEval.record() after update() over the three batches

The methods are called on bare objects (`object.__new__` + the attributes they read): the constructors read annotation
files.  `evaluator.build.gather_dict` is the identity of a one-process run.

The reference ranks with torch.topk, which promises no order among equal values, so it is a valid oracle only for
inputs WITHOUT ties: this script asserts that no row has two equal values among its 11 best -- a condition on the inputs,
which also excludes all-zero rows -- before it trusts a single number.

The record sums rely on Python's `sum()` adding left to right with one rounding per addition.  That holds for the
CPython 3.10 this was generated with; CPython >= 3.12 compensates float sums, where the reference itself would give other
last bits.

    python tests/golden/make_golden_answers.py
"""
import builtins
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
builtins.__POINTNET2_SETUP__ = True

import answers_cases as C  # noqa: E402


def scanqa():
    import evaluator.build as build
    from evaluator.scanqa_eval import ScanQAEval
    build.gather_dict = lambda accelerator, d: d
    ev = object.__new__(ScanQAEval)
    ev.accelerator, ev.best_result, ev.save = types.SimpleNamespace(is_main_process=True), -np.inf, False
    ev.target_metric = "ans1_acc"
    ev.reset()
    keys = C.SCANQA_KEYS
    out = {"scanqa/keys": np.asarray(keys)}
    for i in range(len(C.SIZES)):
        d = C.batch("scanqa", i)
        assert bool(C.tie_free(d["answer_scores"]).all()), ("scanqa", i)
        pairs = ev.batch_metrics(d, include_count=True)
        ratios = ev.batch_metrics(d, include_count=False)
        assert set(pairs) == set(keys) == set(ratios), sorted(pairs)
        out[f"scanqa/{i}/pairs"] = np.asarray([pairs[k] for k in keys], dtype=np.int64)
        out[f"scanqa/{i}/metrics"] = np.asarray([ratios[k] for k in keys], dtype=np.float64)
        ev.update(d)
    _, rec = ev.record()
    out["scanqa/record"] = np.asarray([rec[k] for k in keys], dtype=np.float64)
    return out


def sqa3d():
    from evaluator.sqa3d_eval import SQA3DEval
    ev = object.__new__(SQA3DEval)
    ev.save, ev.best_result = False, -np.inf
    ev.eval_dict = {k: [] for k in C.SQA_KEYS}                           # the constructor's dict (sqa3d_eval.py:17-22)
    ev.reset()
    keys = C.SQA_KEYS
    out = {"sqa3d/keys": np.asarray(keys)}
    seen = []
    for i in range(len(C.SIZES)):
        d = C.batch("sqa3d", i)
        assert bool(C.tie_free(d["answer_scores"]).all()), ("sqa3d", i)
        seen.append(set(d["sqa_type"].tolist()))
        m = ev.batch_metrics(d)
        assert m["total_count"] == C.SIZES[i]
        out[f"sqa3d/{i}/metrics"] = np.asarray([m[k] for k in keys], dtype=np.float64)
        out[f"sqa3d/{i}/type_count"] = np.asarray([m[f"type{t}_count"] for t in range(C.N_TYPES)], dtype=np.float64)
        ev.update(d)
    assert all(4 not in s for s in seen) and sum(3 not in s for s in seen) == 1, seen
    _, rec = ev.record()
    out["sqa3d/record"] = np.asarray([rec[k] for k in keys], dtype=np.float64)
    return out


def main():
    assert sys.version_info < (3, 12), "sum() must add left to right (see the docstring)"
    out = {}
    out.update(scanqa())
    out.update(sqa3d())
    for task in ("scanqa", "sqa3d"):
        print(task, "record", dict(zip(out[f"{task}/keys"].tolist(), np.round(out[f"{task}/record"], 4).tolist())))
        for i in range(len(C.SIZES)):
            print("   batch", i, np.round(out[f"{task}/{i}/metrics"], 4).tolist())
    path = os.path.join(HERE, "answers_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
