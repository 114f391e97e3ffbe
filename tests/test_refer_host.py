"""The ScanRefer target path on the host: the three entries of libgps_hip.so are declared, bound and exported and check
their arguments before any launch; `PackedScans.add_proposals` bookkeeping; the float64 restatement of
tests/refer_cases.py against the reference's own outputs (tests/golden/refer_ref.npz, written by
tests/golden/make_golden_refer.py) -- exact.  No GPU."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import refer_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "refer_ref.npz"))
ENTRIES = ("gps_obj_boxes", "gps_refer_targets", "gps_refer_metrics")


def test_entries_are_declared_bound_and_exported():
    lib = _native.load()
    declared = _native.declared_symbols()
    for name in ENTRIES:
        assert name in declared and name in _native.SIGNATURES and hasattr(lib, name), name
    assert lib.gps_abi_version() == 11                   # additive: the ABI number does not move
    text = open(_native.HEADER_PATH).read()
    assert f"#define GPS_OBJ_BOXES_CHUNK {G.BOXES_CHUNK}" in text and f"#define GPS_REFER_MAX_OBJ {G.REFER_MAX_OBJ}" in text
    from sceneverse_amd.csrc import build
    assert ("gps_refer.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_argument_checks_come_before_any_launch():
    lib = _native.load()
    OK, INVALID, UNSUPPORTED = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT, _native.GPS_ERR_UNSUPPORTED
    # gps_obj_boxes(n_objects, n_points, n_work, xyz, records, work, workspace, boxes, stream)
    assert lib.gps_obj_boxes(-1, 0, 0, None, 1, None, None, None, None) == INVALID
    assert lib.gps_obj_boxes(4, -1, 0, None, 1, None, None, None, None) == INVALID
    assert lib.gps_obj_boxes(4, 10, -1, 16, 1, 16, 16, 16, None) == INVALID
    assert lib.gps_obj_boxes(0, 0, 0, None, 1, None, None, None, None) == OK
    assert lib.gps_obj_boxes(4, 10, 2, 16, 1, 16, None, 16, None) == INVALID         # no workspace
    assert lib.gps_obj_boxes(4, 10, 2, 8, 1, 16, 16, 16, None) == INVALID            # records not 16-byte aligned
    # gps_refer_targets(B, O, n_objects, mode, boxes, labels, row_obj, tgt_obj, scan_range, iou25, iou50, tgt_id,
    #                   obj_labels, stream)
    assert lib.gps_refer_targets(-1, 8, 4, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == INVALID
    assert lib.gps_refer_targets(2, 8, -1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == INVALID
    assert lib.gps_refer_targets(2, 0, 4, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == INVALID
    assert lib.gps_refer_targets(2, 8, 4, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == INVALID   # mode
    assert lib.gps_refer_targets(0, 8, 4, 0, None, None, None, None, None, None, None, None, None, None) == OK
    assert lib.gps_refer_targets(2, 513, 4, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, None) == UNSUPPORTED
    assert lib.gps_refer_targets(2, 8, 4, 0, 1, 1, None, 1, 1, 1, 1, 1, 1, None) == INVALID  # no row table
    # gps_refer_metrics(B, O, logits, ld, logits_bf16, iou25, iou50, tgt_id, is_multiple, counters, stream)
    assert lib.gps_refer_metrics(-1, 8, 1, 8, 0, 1, 1, 1, 1, 1, None) == INVALID
    assert lib.gps_refer_metrics(2, 8, 1, 4, 0, 1, 1, 1, 1, 1, None) == INVALID              # pitch < O
    assert lib.gps_refer_metrics(0, 8, None, 8, 0, None, None, None, None, None, None) == OK
    assert lib.gps_refer_metrics(2, 8, 1, 8, 1, 1, 1, 1, 1, None, None) == INVALID           # no counters


def test_work_list_covers_every_segment_once():
    sizes = np.array([1, 4095, 4096, 4097, 70000, 2, 8192], dtype=np.int64)
    work = G.boxes_work_list(sizes)
    off = np.concatenate([[0], np.cumsum(sizes)])
    assert work.dtype == np.int64 and work.shape == (1 + 1 + 1 + 2 + 18 + 1 + 2, 3)
    assert work[:, 2].min() >= 1 and work[:, 2].max() <= G.BOXES_CHUNK
    seen = np.zeros(off[-1], dtype=np.int64)
    for o, first, n in work:
        assert off[o] <= first and first + n <= off[o + 1]
        seen[first:first + n] += 1
    assert np.all(seen == 1)
    assert G.boxes_work_list(np.zeros(0, np.int64)).shape == (0, 3)


@pytest.mark.parametrize("records", [True, False], ids=["records", "arrays"])
def test_add_proposals_bookkeeping(records):
    packed = C.pack(records=records)
    s = C.scene("small")
    objs, props = packed.scan_objects("small"), packed.scan_proposals("small")
    assert list(objs) == list(range(0, 6)) and packed.scan_inst_ids("small") == [3, 7, 2, 9, 4, 5]
    # proposals follow the scan's annotated objects; the empty mask (2) is skipped
    assert list(props) == list(range(6, 13))
    assert len(packed.scan_proposals("big")) == 79 and len(packed.scan_proposals("empty")) == 0
    assert packed.scan_objects("big").start == 13 and packed.scan_proposals("big").start == 33
    keep = [q for q in range(8) if s["masks"][q].any()]
    assert keep == [0, 1, 3, 4, 5, 6, 7]
    off = packed.obj_offsets.numpy()
    xyz = packed.xyz.numpy()[:, :3]
    for g, q in zip(props, keep):                            # points in pcds[mask == 1] order
        assert np.array_equal(xyz[off[g]:off[g + 1]], s["points"][s["masks"][q] == 1])
    if records:                                              # the colours travel in the record's 4th word
        rgb = packed.xyz.numpy().view(np.uint8).reshape(-1, 16)[:, 12:15]
    else:
        rgb = packed.rgb.numpy()
    g = props[1]
    assert np.array_equal(rgb[off[g]:off[g + 1]], s["colors"][s["masks"][1] == 1])
    # overlapping masks: the shared points are stored once per proposal
    shared = int((s["masks"][1] & s["masks"][5]).sum())
    assert shared > 0 and packed.sizes_host[props[1]] + packed.sizes_host[props[4]] == \
        int(s["masks"][1].sum()) + int(s["masks"][5].sum())
    labels = packed.labels.numpy()
    assert labels.dtype == np.int32 and labels[list(objs)].tolist() == [5, 6, 7, 0, 7, 8]
    assert labels[list(props)].tolist() == [9, 10, 11, 3, 10, 9, 4]
    rows = G.batch_rows(packed, ["small", "empty", "big"], 80, proposals=True)
    assert rows.dtype == torch.int32 and rows[0, :7].tolist() == list(props) and bool((rows[0, 7:] == -1).all())
    assert bool((rows[1] == -1).all()) and rows[2, :79].tolist() == list(packed.scan_proposals("big")) and rows[2, 79] == -1
    assert G.batch_rows(packed, ["small"], 8)[0, :6].tolist() == list(objs)      # the annotated rows keep their meaning
    with pytest.raises(ValueError):
        G.batch_rows(packed, ["big"], 50, proposals=True)
    assert packed.boxes is None                              # the boxes are a device product


def test_add_proposals_order_and_defaults():
    s = C.scene("empty")
    p = G.PackedScans("cpu")
    with pytest.raises(KeyError):
        p.add_proposals("empty", s["points"], s["colors"], s["masks"], s["prop_labels"])
    p.add_scan("empty", s["points"], s["colors"], s["instance_labels"], s["inst_ids"])      # no inst_labels: -100
    p.add_proposals("empty", s["points"], s["colors"], np.ones((1, len(s["points"])), np.uint8), [7])
    with pytest.raises(ValueError):
        p.add_proposals("empty", s["points"], s["colors"], s["masks"], s["prop_labels"])
    p.finalize()
    assert p.labels.tolist() == [-100, -100, -100, 7] and list(p.scan_proposals("empty")) == [3]
    assert p.sizes_host[3] == len(s["points"])
    with pytest.raises(ValueError):
        G.PackedScans("cpu").add_scan("x", s["points"], s["colors"], s["instance_labels"], s["inst_ids"], inst_labels=[1])


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_restatement_reproduces_the_reference_exactly(case):
    name = case[0]
    f25, f50, tgt, labels = C.restate_case(case)
    assert np.array_equal(f25, GOLD[f"{name}/iou25"]) and np.array_equal(f50, GOLD[f"{name}/iou50"])
    assert np.array_equal(tgt, GOLD[f"{name}/tgt_id"]) and np.array_equal(labels, GOLD[f"{name}/labels"])


def test_fixture_covers_the_cases_it_claims():
    s = C.scene("small")
    gt, prop, _ = C.scene_boxes(s)
    ids, labels = C.kept(s)
    a, b, t = gt[ids.index(3)], gt[ids.index(7)], gt[ids.index(2)]
    # the proposal that is all of B overlaps A (first in scan order) and B at >= 0.25, and takes A's label
    assert C.iou(a, prop[0]) >= 0.25 and C.iou(b, prop[0]) > C.iou(a, prop[0])
    assert GOLD["pred8/labels"][0, 0] == labels[ids.index(3)] == 5
    # nested dyadic boxes: volume ratio exactly 1/4 and 1/2, IoU just below the thresholds
    assert np.array_equal(t, [2.5, 4.5, 0.5, 1, 1, 1])
    assert np.array_equal(prop[2], [2.5, 4.5, 0.125, 1, 1, 0.25]) and np.array_equal(prop[3], [2.5, 4.5, 0.25, 1, 1, 0.5])
    assert 0.25 - 1e-8 < C.iou(prop[2], t) < 0.25 and 0.5 - 1e-8 < C.iou(prop[3], t) < 0.5
    assert GOLD["pred8/iou25"][0].tolist() == [0, 1, 0, 1, 1, 0, 0, 0] and GOLD["pred8/iou50"][0].tolist() == [0, 1, 0, 0, 1, 0, 0, 0]
    # two proposals >= 0.25 on the target: the largest index; none: n_b; no proposals at all: 0
    assert GOLD["pred8/tgt_id"].tolist()[:2] == [4, 7] and GOLD["pred8/tgt_id"][5] == 0
    # IoUs spread over (0, 1)
    v = [C.iou(p, t) for p in prop[1:5]] + [C.iou(prop[5], gt[ids.index(4)]), C.iou(prop[6], gt[ids.index(5)])]
    assert min(v) < 0.2 and max(v) > 0.8 and sum(0.3 < x < 0.7 for x in v) >= 2
    # O = 80 with n_b = 79, hits on both sides of slot 64
    assert (GOLD["pred80/labels"][0] != -100).sum() == 79
    assert sorted(np.flatnonzero(GOLD["pred80/iou25"][2]).tolist()) == [24, 44, 64]
    assert GOLD["pred80/tgt_id"].tolist() == [60, 63, 64, 70, 78, 59, 4, 0, 64, 70]
    # 'gt' items: one-hot, the wall is dropped unless it is the target
    assert GOLD["gt8/iou25"].sum(1).tolist() == [1] * 6 and GOLD["gt8/labels"][1, :6].tolist() == [5, 6, 7, 7, 8, 0]
    # the logits: a tie, an all -inf row, a NaN row
    x = C.case_logits(C.CASES[0])
    assert x[0, 4] == x[0, 7] == x[0].max() and bool(torch.isinf(x[1]).all()) and bool(torch.isnan(x[2, [3, 5]]).all())
    assert torch.equal(x.nan_to_num(nan=0.0), x.to(torch.bfloat16).float().nan_to_num(nan=0.0))   # all bf16 numbers
    for name in C.CASE_IDS:
        m = GOLD[f"{name}/metrics"]
        assert m.shape == (7, 2) and m[0, 1] == len(GOLD[f"{name}/tgt_id"])


def test_refer_targets_rejects_a_full_row_and_the_cpu():
    packed = C.pack()
    with pytest.raises(RuntimeError):                        # no CPU path
        G.refer_targets(packed, G.batch_rows(packed, ["small"], 8, proposals=True), [2], ["small"], "pred")
    with pytest.raises(RuntimeError):
        G.obj_boxes(packed)
    # 7 proposals in 7 slots: the reference's n_b + 1 flags do not fit (its pad_tensors asserts)
    with pytest.raises(ValueError):
        G.refer_targets(packed, G.batch_rows(packed, ["small"], 7, proposals=True), [2], ["small"], "pred")
    with pytest.raises(ValueError):
        G.refer_targets(packed, G.batch_rows(packed, ["small"], 8, proposals=True), [2], ["small"], "both")


def test_counter_refuses_cpu_tensors():
    from sceneverse_amd.engine import ScanReferCounter
    c = ScanReferCounter("cpu")
    batch = {"tgt_object_id_iou25": torch.zeros(2, 8, dtype=torch.int64), "tgt_object_id_iou50": torch.zeros(2, 8, dtype=torch.int64),
             "tgt_object_id": torch.zeros(2, 1, dtype=torch.int64), "is_multiple": torch.zeros(2, dtype=torch.bool)}
    with pytest.raises(RuntimeError):
        c.update(torch.zeros(2, 8), batch)
    assert c.result(include_count=True)["og_acc_iou25"] == (0, 0) and c.result()["og_acc"] == 0.0
