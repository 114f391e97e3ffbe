"""The ScanRefer target path on the GPU (csrc/gps_refer.hip): boxes of every packed object, the IoU targets of a
batch and the evaluator's counts, against numpy and against the reference's own outputs
(tests/golden/refer_ref.npz, tests/golden/make_golden_refer.py).  Every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import refer_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "refer_ref.npz"))
_CACHE = {}


def _packed():
    if "packed" not in _CACHE:
        _CACHE["packed"] = C.pack(device=DEV)
    return _CACHE["packed"]


def _numpy_boxes(packed):
    """convert_pc_to_box on the packed points themselves, float64 like the loader's rows."""
    xyz = packed.xyz.cpu().numpy()[:, :3].astype(np.float64)
    off = packed.obj_offsets.cpu().numpy()
    out = np.empty((packed.n_objects, 6), dtype=np.float64)
    for g in range(packed.n_objects):
        p = xyz[off[g]:off[g + 1]]
        lo, hi = p.min(0), p.max(0)
        out[g, :3], out[g, 3:] = (lo + hi) / 2, hi - lo
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.mark.parametrize("records", [True, False], ids=["records", "arrays"])
def test_boxes_are_bit_equal_to_numpy(records):
    rng = np.random.default_rng(5)
    chunk = G.BOXES_CHUNK
    sizes = [1, chunk - 1, chunk, chunk + 1, 70000, 300, 2]          # one point; one chunk -1 / 0 / +1; 18 chunks
    pts = (rng.standard_normal((sum(sizes), 3)) * rng.uniform(0.1, 5.0, size=3)).astype(np.float32)
    inst = np.repeat(np.arange(len(sizes)), sizes)
    perm = rng.permutation(len(pts))
    pts, inst = pts[perm], inst[perm]
    colors = rng.integers(0, 256, size=(len(pts), 3)).astype(np.uint8)
    masks = np.stack([(inst == 4) & (pts[:, 0] > 0), (inst == 4) & (pts[:, 1] > 0) | (inst == 5), inst == 0])
    packed = G.PackedScans(DEV, records=records)
    packed.add_scan("s", pts, colors, inst, list(range(len(sizes))), inst_labels=list(range(len(sizes))))
    packed.add_proposals("s", pts, colors, masks, [1, 2, 3])         # the first two store the same points twice
    packed.finalize()
    assert packed.records == records and packed.n_objects == len(sizes) + 3
    assert packed.boxes.shape == (packed.n_objects, 6) and packed.boxes.dtype == torch.float64
    want = _numpy_boxes(packed)
    got = packed.boxes.cpu().numpy()
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(got[0, 3:], [0, 0, 0]) and np.array_equal(got[0, :3], pts[inst == 0][0].astype(np.float64))
    again = G.obj_boxes(packed).cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got))
    # the fixture's scenes too, proposals included (they duplicate points of the annotated objects)
    p2 = C.pack(device=DEV, records=records)
    assert np.array_equal(_bits(p2.boxes.cpu().numpy()), _bits(_numpy_boxes(p2)))


def test_boxes_with_non_finite_coordinates():
    pts = np.array([[1, 2, 3], [-np.inf, 5, 6], [4, np.nan, np.inf], [0, 0, 0], [7, 8, 9], [1, 1, 1]], dtype=np.float32)
    inst = np.array([0, 0, 0, 1, 1, 1])
    packed = G.PackedScans(DEV)
    packed.add_scan("s", pts, np.zeros((6, 3), np.uint8), inst, [0, 1])
    packed.finalize()
    got = packed.boxes.cpu().numpy()
    with np.errstate(invalid="ignore"):
        want = _numpy_boxes(packed)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[1], [3.5, 4, 4.5, 7, 8, 9])
    # x: min -inf, max 4; y holds a NaN; z: min 3, max +inf
    assert np.isnan(got[0]).tolist() == [False, True, False, False, True, False]
    assert got[0, [0, 2, 3, 5]].tolist() == [-np.inf, np.inf, np.inf, np.inf]
    assert np.array_equal(got[0], want[0], equal_nan=True)


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_targets_equal_the_reference(case):
    name, O, mode = case[0], case[1], case[2]
    packed = _packed()
    rows, tgt, sids = C.case_inputs(packed, case)
    res = G.refer_targets(packed, rows, tgt, sids, mode)
    B = len(sids)
    assert res["tgt_object_id"].shape == (B, 1) and all(t.dtype == torch.int64 for t in res.values())
    assert np.array_equal(res["tgt_object_id_iou25"].cpu().numpy(), GOLD[f"{name}/iou25"])
    assert np.array_equal(res["tgt_object_id_iou50"].cpu().numpy(), GOLD[f"{name}/iou50"])
    assert np.array_equal(res["tgt_object_id"].cpu().numpy().reshape(-1), GOLD[f"{name}/tgt_id"])
    assert np.array_equal(res["obj_labels"].cpu().numpy(), GOLD[f"{name}/labels"])
    pad = (rows < 0).numpy()
    assert np.all(res["obj_labels"].cpu().numpy()[pad] == -100)
    assert np.all(res["tgt_object_id_iou25"].cpu().numpy()[pad] == 0) and np.all(res["tgt_object_id_iou50"].cpu().numpy()[pad] == 0)
    # out=: the same values written in place, rows and targets already on the device
    out = {"tgt_object_id_iou25": torch.full((B, O), 7, dtype=torch.int64, device=DEV),
           "tgt_object_id_iou50": torch.full((B, O), 7, dtype=torch.int64, device=DEV),
           "tgt_object_id": torch.full((B, 1), 7, dtype=torch.int64, device=DEV),
           "obj_labels": torch.full((B, O), 7, dtype=torch.int64, device=DEV)}
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    res2 = G.refer_targets(packed, rows.to(DEV), torch.tensor(tgt, device=DEV), sids, mode, out=out)
    for k in out:
        assert res2[k].data_ptr() == ptrs[k] and torch.equal(out[k], res[k]), k
    with pytest.raises(ValueError):
        G.refer_targets(packed, rows, tgt, sids, mode, out=dict(out, obj_labels=out["obj_labels"].int()))


def _batch(name):
    return {"tgt_object_id_iou25": torch.from_numpy(GOLD[f"{name}/iou25"]).to(DEV),
            "tgt_object_id_iou50": torch.from_numpy(GOLD[f"{name}/iou50"]).to(DEV),
            "tgt_object_id": torch.from_numpy(GOLD[f"{name}/tgt_id"]).to(DEV)[:, None],
            "is_multiple": torch.from_numpy(GOLD[f"{name}/is_multiple"]).to(DEV)}


def _pairs(name, times=1):
    return {k: (int(h) * times, int(n) * times) for k, (h, n) in zip(C.METRIC_KEYS, GOLD[f"{name}/metrics"])}


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_metrics_equal_the_reference(case, dtype):
    from sceneverse_amd.engine import ScanReferCounter
    name, O = case[0], case[1]
    logits = C.case_logits(case).to(DEV).to(dtype)
    batch = _batch(name)
    counter = ScanReferCounter(DEV)
    counter.update(logits, batch)
    assert counter.result(include_count=True) == _pairs(name)
    ratios = counter.result()
    assert ratios == {k: h / max(n, 1) for k, (h, n) in _pairs(name).items()}
    wide = torch.full((logits.shape[0], O + 5), 100.0, dtype=dtype, device=DEV)     # a row pitch: the tail is not read
    wide[:, :O] = logits
    counter.update(wide[:, :O], batch)
    assert counter.result(include_count=True) == _pairs(name, 2)                   # two updates accumulate
    assert counter.counts[7].item() == 0                                           # the spare counter
    counter.reset()
    assert counter.counts.tolist() == [0] * 8
    assert counter.result(include_count=True)["og_acc"] == (0, 0)


def test_update_is_capturable():
    """No host sync in `update`: one update captured in a graph, replayed twice."""
    from sceneverse_amd.engine import ScanReferCounter
    case = C.CASES[1]
    logits, batch = C.case_logits(case).to(DEV), _batch(case[0])
    batch["is_multiple"] = batch["is_multiple"].to(torch.uint8)
    counter = ScanReferCounter(DEV)
    counter.update(logits, batch)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        counter.update(logits, batch)
    graph.replay()
    graph.replay()
    assert counter.result(include_count=True) == _pairs(case[0], 3)


def test_end_to_end_rows_to_counts():
    """Rows of proposals -> obj_processing_aug + refer_targets -> the GroundHeadV1 model's og3d_logits -> the counter."""
    from util import gps_cfg, lang_dir
    from sceneverse_amd.data.synthetic import synth_batch
    from sceneverse_amd.engine import GPSTrainStep, ScanReferCounter, scanrefer_accuracy
    packed = _packed()
    sids, O = ["small", "small"], 8
    tgt = [C.kept(C.scene("small"))[0].index(i) for i in (2, 7)]
    rows = G.batch_rows(packed, sids, O, proposals=True)
    batch = synth_batch(2, n_obj=O, txt_len=20, seed=3, min_real=3, device=DEV)
    batch.pop("scene_txt_ids"), batch.pop("scene_txt_masks")
    objs = G.obj_processing_aug(packed, rows, 1024, seed=1, need_boxes=True)
    targets = G.refer_targets(packed, rows, tgt, sids, "pred")
    batch.update(objs)
    batch.update(targets)
    batch["obj_sem_masks"] = batch["obj_masks"].clone()
    batch["is_multiple"] = torch.tensor([True, False], device=DEV)
    assert batch["obj_masks"].sum(1).tolist() == [7, 7] and batch["obj_boxes"].shape == (2, O, 6)
    assert targets["tgt_object_id"].reshape(-1).tolist() == [4, 0]
    step = GPSTrainStep(gps_cfg(lang_dir(0), heads="ground", use_scene_cap=False), device=DEV, ddp=False)
    out, total, _ = step.evaluate(dict(batch))
    logits = out["og3d_logits"]
    assert logits.shape == (2, O) and bool(torch.isfinite(total))
    counter = ScanReferCounter(DEV)
    counter.update(logits, batch)
    got = counter.result()
    want = scanrefer_accuracy(logits.float(), batch["tgt_object_id_iou25"], batch["tgt_object_id_iou50"])
    assert got["og_acc_iou25"] == want["og_acc_iou25"] and got["og_acc_iou50"] == want["og_acc_iou50"]
    pairs = counter.result(include_count=True)
    assert pairs["og_acc_iou25"][1] == 2 and pairs["og_acc_iou25_multiple"][1] == 1 and pairs["og_acc_iou25_unique"][1] == 1
    pred = logits.float().argmax(-1)
    assert pairs["og_acc"][0] == int((pred == batch["tgt_object_id"].reshape(-1)).sum())
