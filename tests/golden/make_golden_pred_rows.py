"""Generate tests/golden/pred_rows_ref.npz by calling the REFERENCE's own `ScanBase._getitem_refer` (data/datasets/
base.py:324-512) with `pc_type: 'pred'` for every row of the `ref` cases of tests/pred_rows_cases.py -- imported unmodified
from /root/reference (only runnable in the build container).  `self` is a SimpleNamespace and `scan_data` is laid out as
tests/golden/make_golden_refer.py lays it out (`_load_scan`, base.py:98-141, with the reference's `convert_pc_to_box`);
`max_obj_len` is the case's M, what ScanNetSpatialRefer makes of the config's value (scannet.py:50).  `_obj_processing_aug`
is stubbed to hand back, for every cloud it is given, that proposal's POSITION in its scan (the clouds are passed on by
identity), so what the reference selected, and in which order, is read off its own call.  `random` is seeded per row and
`random.shuffle` is wrapped with the recorder of make_golden_rows.py.  Only the reference's OUTPUTS are stored: the
selected positions, tgt_object_id, both flag vectors (their n + 1 entries cut or padded to O; the entry cut is 0),
obj_labels, is_multiple / is_hard, n_rem and the first M entries of `order` -- and, for the end-to-end batch of
pred_rows_cases.py, what `ScanReferEval.batch_metrics` (evaluator/scanrefer_eval.py:14-87) counts on logits that are a
function of the proposal, placed into slots by the reference's own rows.

The file is written only if the restatement of pred_rows_cases.py reproduces every row under the comparison stated in
include/gps_hip.h (`compare_with_reference`) -- which also says that every `ref` row is one the reference runs without
failing its own assertion.

    python tests/golden/make_golden_pred_rows.py
"""
import builtins
import collections
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

import pred_rows_cases as C  # noqa: E402
from make_golden_rows import ShuffleRecorder  # noqa: E402


def scan_data_of(s, id_map):
    """One entry of ScanBase.scan_data, the keys _getitem_refer reads; label counts as in scannet.py:70-76."""
    from data.data_utils import convert_pc_to_box
    pcds = np.concatenate([s["points"], s["colors"] / 127.5 - 1], 1)
    assert pcds.dtype == np.float64
    d = {"obj_pcds": [pcds[s["instance_labels"] == i] for i in s["inst_ids"]], "inst_labels": list(s["inst_labels"]),
         "inst_ids": list(s["inst_ids"])}
    d["obj_pcds_pred"] = [pcds[m == 1, :] for m in s["masks"]]
    assert all(p.shape[0] > 0 for p in d["obj_pcds_pred"])
    d["inst_labels_pred"] = list(s["prop_labels"])
    for key, src in (("", "obj_pcds"), ("_pred", "obj_pcds_pred")):
        boxes = [convert_pc_to_box(p) for p in d[src]]
        d["obj_center" + key] = [b[0] for b in boxes]
        d["obj_box_size" + key] = [b[1] for b in boxes]
    d["label_count"] = collections.Counter(d["inst_labels"])
    d["label_count_multi"] = collections.Counter(int(id_map[l]) for l in d["inst_labels"])
    return d


def reference_case(case):
    import data.datasets.base as base
    B, M, O = len(case["rows"]), case["M"], case["O"]
    id_map = case["label_map"] if case["label_map"] is not None else np.arange(C.N_LABELS)
    converter = types.SimpleNamespace(id_to_scannetid={i: int(id_map[i]) for i in range(C.N_LABELS)})
    out = {"sel": np.full((B, O), -1, np.int32), "tgt_id": np.zeros(B, np.int64), "n_sel": np.zeros(B, np.int32),
           "iou25": np.zeros((B, O), np.int64), "iou50": np.zeros((B, O), np.int64), "labels": np.full((B, O), -100, np.int64),
           "n_rem": np.zeros(B, np.int32), "is_multiple": np.zeros(B, bool), "is_hard": np.zeros(B, bool),
           "order": np.full((B, M), -1, np.int32)}
    for b, row in enumerate(case["rows"]):
        sid = C.scene_id(case, b)
        data = scan_data_of(C.make_scene(row["props"]), id_map)
        where = {id(p): k for k, p in enumerate(data["obj_pcds_pred"])}

        def obj_processing_aug(obj_pcds, obj_labels, is_need_bbox=False):
            marks = torch.tensor([where[id(p)] for p in obj_pcds], dtype=torch.long)
            return marks, torch.zeros(len(obj_pcds), 6), torch.zeros(len(obj_pcds), 6), torch.LongTensor(list(obj_labels))

        label = C.ANN_LABELS[row["tgt"]] if row["tgt_label"] is None else row["tgt_label"]
        lang = [{"item_id": sid, "scan_id": sid, "target_id": C.INST0 + row["tgt"], "utterance": "the thing near the door",
                 "instance_type": C.INT2CAT[label]}]
        fake = types.SimpleNamespace(
            lang_data=lang, use_scene_cap=False, pc_type="pred", scan_data={sid: data}, filter_lang=False, int2cat=C.INT2CAT,
            cat2int=C.CAT2INT, max_obj_len=M, load_scene_pcds=False, aug_cfg=True, _obj_processing_aug=obj_processing_aug,
            label_converter=converter)
        random.seed(1000 * case["seed"] + b)
        with ShuffleRecorder() as rec:
            d = base.ScanBase._getitem_refer(fake, 0)
        marks = d["obj_fts"].numpy()
        n = len(marks)
        assert n <= M and len(d["tgt_object_id_iou25"]) == n + 1
        out["sel"][b, :n] = marks
        out["n_sel"][b] = n
        out["tgt_id"][b] = int(d["tgt_object_id"])
        for key, src in (("iou25", "tgt_object_id_iou25"), ("iou50", "tgt_object_id_iou50")):
            flags = d[src].numpy()
            assert not flags[O:].any() and flags[n] == 0
            out[key][b, :min(n + 1, O)] = flags[:O]
        out["labels"][b, :n] = d["obj_labels"].numpy()
        out["is_multiple"][b], out["is_hard"][b] = bool(d["is_multiple"]), bool(d["is_hard"])
        order = rec.order()
        out["n_rem"][b] = len(order)
        out["order"][b, :min(M, len(order))] = order[:M]
    mine = C.restate_case(case, order=out["order"])
    bad = {b: C.compare_with_reference(mine, out, b, M) for b in range(B)}
    bad = {b: v for b, v in bad.items() if v}
    swapped = sum(not np.array_equal(mine["row_obj"][b], out["sel"][b]) for b in range(B))
    print(f"{case['name']}: {B} rows, restatement equal under the stated comparison: {not bad} {bad if bad else ''}| cropped "
          f"{int((np.asarray([len(r['props']) for r in case['rows']]) > M).sum())}, random fill {int((out['n_rem'] > 0).sum())} "
          f"(n_rem up to {int(out['n_rem'].max())}), pinned block in another order {swapped}, multiple "
          f"{int(out['is_multiple'].sum())}, hard {int(out['is_hard'].sum())}")
    return {f"{case['name']}/{k}": v for k, v in out.items()}, not bad


def reference_metrics(case, out):
    """ScanReferEval.batch_metrics(include_count=True) (evaluator/scanrefer_eval.py:14-87) on the end-to-end batch: the
    proposals' scores placed into slots by the REFERENCE's own rows -> (7, 2) [hits, count] in METRIC_KEYS order."""
    from evaluator.scanrefer_eval import ScanReferEval
    from refer_cases import METRIC_KEYS
    rows = C.e2e_rows()
    g = {k: out[f"{case['name']}/{k}"][rows] for k in ("sel", "iou25", "iou50", "tgt_id", "labels", "is_multiple", "n_sel")}
    batch = {"og3d_logits": torch.from_numpy(C.slot_logits(case, rows, g["sel"])),
             "tgt_object_id_iou25": torch.from_numpy(g["iou25"]), "tgt_object_id_iou50": torch.from_numpy(g["iou50"]),
             "tgt_object_id": torch.from_numpy(g["tgt_id"]).reshape(-1, 1), "is_multiple": torch.from_numpy(g["is_multiple"]),
             "obj_labels": torch.from_numpy(g["labels"]),
             "obj_masks": torch.arange(case["O"])[None, :] < torch.from_numpy(g["n_sel"])[:, None]}
    m = ScanReferEval.batch_metrics(types.SimpleNamespace(save=False), batch, include_count=True)
    res = np.asarray([m[k] for k in METRIC_KEYS], dtype=np.int64)
    print(f"end to end: rows {rows} of {case['name']}:", {k: tuple(m[k]) for k in METRIC_KEYS})
    assert 0 < res[0, 0] < len(rows) and 0 < res[6, 0] < len(rows) and res[1, 0] < res[0, 0]    # neither all nor none
    return res


def main():
    C.check_construction()
    out, ok = {}, True
    for c in C.REF_CASES:
        o, same = reference_case(c)
        out.update(o)
        ok = ok and same
        if c["name"] == C.E2E_CASE:
            out["e2e/metrics"] = reference_metrics(c, out)
    if not ok:
        raise SystemExit("the restatement does not reproduce the reference: pred_rows_ref.npz NOT written")
    path = os.path.join(HERE, "pred_rows_ref.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
