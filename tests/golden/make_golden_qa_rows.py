"""Generate tests/golden/qa_rows_ref.npz by calling the REFERENCE's own `ScanNetScanQAOld.__getitem__` (data/datasets/
scannet_old.py:326-484) and `ScanNetSQA3D.__getitem__` (:94-232) for every row of the `ref` cases of
tests/qa_rows_cases.py -- imported unmodified from /root/reference (only runnable in the build container).  `self` is a
SimpleNamespace.  'gt' scans are marker clouds (every object's cloud is ONE row that holds its position, the method of
make_golden_rows.py); 'pred' scans are the corner clouds of pred_rows_cases.py laid out like make_golden_pred_rows.py does
(`scan_data_of`), the proposals' clouds recognised by identity.  `_obj_processing_post` is stubbed to hand the markers
back, so what the reference selected, and in which order, is read off its own call.  `random` is seeded per row;
`random.shuffle` is wrapped with the recorder of make_golden_rows.py and `random.choice` likewise, from which the replay
`order` and `pick` follow.  The answer vocabularies are the reference's own classes: ScanQAAnswer over the names "0" ..
"A-1", SQA3DAnswer over the same with 'u' in the last place; an answer outside the vocabulary is the string "zzz".
Only the reference's OUTPUTS are stored: the selected positions, n_rem, the first M entries of `order`, the pick,
sqa_type, obj_labels and the three multi-hots as uint8 (their dtypes are asserted here: float32 for ScanQA, int64 for
SQA3D; tgt_object_id's n + 1 entries cut or padded to O).

The file is written only if the restatement of qa_rows_cases.py reproduces every row exactly, and the share of rows
WITHOUT a reference is printed (at most a quarter: qa_rows_cases.check_construction).

    python tests/golden/make_golden_qa_rows.py
"""
import builtins
import os
import random
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
sys.path.insert(0, "/root/reference")
sys.path.insert(0, os.path.join(HERE, "ref_stubs"))
builtins.__POINTNET2_SETUP__ = True

import pred_rows_cases as PC  # noqa: E402
import qa_rows_cases as C  # noqa: E402
from make_golden_pred_rows import scan_data_of  # noqa: E402
from make_golden_rows import ShuffleRecorder  # noqa: E402


class ChoiceRecorder:
    """Stands in for random.choice while one reference call runs: at most one call, its index recorded."""

    def __init__(self):
        self.pick = None
        self._choice = random.choice

    def __enter__(self):
        def rec(seq):
            assert self.pick is None, "a second choice"
            got = self._choice(seq)
            self.pick = [i for i, s in enumerate(seq) if s is got][0]
            return got

        random.choice = rec
        return self

    def __exit__(self, *exc):
        random.choice = self._choice
        return False


def reference_row(case, b, row, mod):
    """-> what the reference's __getitem__ returns for the row, the markers' meaning, the two recorders."""
    from data.data_utils import ScanQAAnswer, SQA3DAnswer
    M, A = case["M"], case["A"]
    sid = C.scene_id(case, b)
    if case["pc_type"] == "pred":
        data = scan_data_of(PC.make_scene(row["scan"][1]), np.arange(12))
        where = {id(p): k for k, p in enumerate(data["obj_pcds_pred"])}
        ann_labels = PC.ANN_LABELS
    else:
        labels = [int(l) for l in row["scan"][1]]
        data = {"obj_pcds": [np.full((1, 6), p, dtype=np.float64) for p in range(len(labels))], "inst_labels": labels}
        where = {id(p): k for k, p in enumerate(data["obj_pcds"])}
        ann_labels = labels

    def obj_processing_post(obj_pcds, obj_labels, is_need_bbox=False, rot_aug=False):
        marks = torch.tensor([where[id(p)] for p in obj_pcds], dtype=torch.long)
        return marks, torch.zeros(len(obj_pcds), 6), torch.zeros(len(obj_pcds), 6), torch.LongTensor(list(obj_labels))

    names = [str(i) for i in range(A)]
    strings = [names[a] if 0 <= a < A else "zzz" for a in row["answers"]]
    sqa = case["kind"] == "sqa3d"
    if sqa:
        names[-1] = "u"
        strings = [s if s != str(A - 1) else "u" for s in strings]
    tl = [ann_labels[t] for t in row["tgt"]] if row["tgt_label"] is None else row["tgt_label"]
    fake = types.SimpleNamespace(
        pc_type=case["pc_type"], sem_type="607", max_obj_len=M, filter_lang=case["lang"], int2cat=C.INT2CAT,
        cat2int=C.CAT2INT, scan_data={sid: data}, base_dir="", num_answers=A, _obj_processing_post=obj_processing_post,
        rot_aug=False)
    if sqa:
        assert not row["tgt"]
        fake.split = "train"
        fake.answer_vocab = SQA3DAnswer(names)
        fake.questions_map = {sid: {b: {"situation": list(row["situations"]), "question": row["question"]}}}
        fake.lang_data = [{"question_id": b, "scene_id": sid, "answers": [{"answer": s} for s in strings], "position": None,
                           "rotation": None}]
        fn = mod.ScanNetSQA3D.__getitem__
    else:
        fake.is_test = False
        fake.answer_vocab = ScanQAAnswer(names)
        fake.lang_data = [{"question_id": b, "scene_id": sid, "object_ids": list(row["tgt"]),
                           "object_names": [C.INT2CAT[l] for l in tl], "answers": strings, "question": row["question"]}]
        fn = mod.ScanNetScanQAOld.__getitem__
    random.seed(1000 * case["seed"] + b)
    with ShuffleRecorder() as rec, ChoiceRecorder() as ch:
        d = fn(fake, 0)
    return d, rec, ch


def reference_case(case, mod):
    B, M, O, A = len(case["rows"]), case["M"], case["O"], case["A"]
    sqa = case["kind"] == "sqa3d"
    out = {"row_obj": np.full((B, O), -1, np.int32), "n_sel": np.zeros(B, np.int32), "n_rem": np.zeros(B, np.int32),
           "order": np.full((B, M), -1, np.int32), "pick": np.zeros(B, np.int32), "sqa_type": np.zeros(B, np.int64),
           "obj_labels": np.full((B, O), -100, np.int64), "tgt_object_id": np.zeros((B, O), np.uint8),
           "tgt_object_label": np.zeros((B, C.N_LABELS), np.uint8), "answer_label": np.zeros((B, A), np.uint8)}
    for b, row in enumerate(case["rows"]):
        d, rec, ch = reference_row(case, b, row, mod)
        marks = d["obj_fts"].numpy()
        n = len(marks)
        assert n <= M
        out["row_obj"][b, :n] = marks
        out["n_sel"][b] = n
        out["obj_labels"][b, :n] = d["obj_labels"].numpy()
        order = rec.order()
        out["n_rem"][b] = len(order)
        out["order"][b, :min(M, len(order))] = order[:M]
        out["pick"][b] = 0 if ch.pick is None else ch.pick
        assert (ch.pick is not None) == sqa
        want = torch.int64 if sqa else torch.float32
        for key in ("tgt_object_id", "tgt_object_label", "answer_label"):
            assert d[key].dtype == want and set(d[key].unique().tolist()) <= {0, 1}, (key, d[key].dtype)
        flags = d["tgt_object_id"].numpy()
        assert len(flags) == n + 1 and d["tgt_object_label"].shape == (C.N_LABELS,) and d["answer_label"].shape == (A,)
        out["tgt_object_id"][b, :min(n + 1, O)] = flags[:O]
        out["tgt_object_label"][b] = d["tgt_object_label"].numpy()
        out["answer_label"][b] = d["answer_label"].numpy()
        if sqa:
            out["sqa_type"][b] = d["sqa_type"]
            assert d["sentence"] == row["texts"][out["pick"][b]]
    mine = C.restate_case(case, order=out["order"], pick=out["pick"])
    bad = [k for k in C.OUT_KEYS if k != "n_tgt" and not np.array_equal(mine[k], out[k])]
    rows = case["rows"]
    print(f"{case['name']}: {B} rows, restatement equal: {not bad} {bad if bad else ''}| cropped "
          f"{int((out['n_rem'] > 0).sum() + ((out['n_sel'] == M) & (out['n_rem'] == 0)).sum())}, random fill "
          f"{int((out['n_rem'] > 0).sum())} (n_rem up to {int(out['n_rem'].max())}), targets per row up to "
          f"{int(out['tgt_object_id'].sum(1).max())}, picks {sorted(set(out['pick'].tolist()))}, variants up to "
          f"{max(len(r['texts']) for r in rows)}")
    return {f"{case['name']}/{k}": v for k, v in out.items()}, not bad


def main():
    import data.datasets.scannet_old as mod
    share, n_rows = C.check_construction()
    out, ok = {}, True
    for c in C.REF_CASES:
        o, same = reference_case(c, mod)
        out.update(o)
        ok = ok and same
    print(f"rows without a reference (restatement only): {share:.1%} of {n_rows} (the cap is 25%)")
    if not ok:
        raise SystemExit("the restatement does not reproduce the reference: qa_rows_ref.npz NOT written")
    path = os.path.join(HERE, "qa_rows_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
