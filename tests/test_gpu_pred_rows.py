"""The device-side selection of predicted proposals on the GPU (csrc/gps_obj_select_pred.hip through sceneverse_amd/data/
gpu_objects.py: PackedScans.match_labels, select_rows(pc_type="pred")): the matched labels against refer_targets' own,
replays of the reference's shuffles against the reference's outputs (tests/golden/pred_rows_ref.npz) under the comparison
stated in include/gps_hip.h, the device fill law against its numpy emulation (tests/pred_rows_cases.py), the fused target
outputs against refer_targets, one graph capture together with obj_processing_post, and one run through ScanReferCounter.
Every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import pred_rows_cases as C  # noqa: E402
import refer_cases  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_objects import select_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "pred_rows_ref.npz"))
ROW_KEYS = ("row_obj", "tgt_slot", "n_sel", "n_rem", "is_multiple", "is_hard")
TGT_KEYS = ("tgt_object_id_iou25", "tgt_object_id_iou50", "tgt_object_id", "obj_labels")
RESTATED = {"tgt_object_id_iou25": "iou25", "tgt_object_id_iou50": "iou50", "tgt_object_id": "tgt_id", "obj_labels": "labels"}
_CACHE = {}


def _packed():
    """All cases' scenes as ONE PackedScans, packed once for the module."""
    if "packed" not in _CACHE:
        _CACHE["packed"] = C.pack(device=DEV)
    return _CACHE["packed"]


def _tables(case):
    """-> (scan ids, device tables (annotated ranges, proposal ranges), targets on the device, first proposal id per row)."""
    packed = _packed()
    sids = [C.scene_id(case, b) for b in range(len(case["rows"]))]
    tabs = (G.scan_ranges(packed, sids), G.scan_ranges(packed, sids, proposals=True))
    tgt = torch.tensor([r["tgt"] for r in case["rows"]], dtype=torch.int64, device=DEV)
    return sids, tabs, tgt, np.asarray([packed.scan_proposals(s).start for s in sids], dtype=np.int64)


def _kw(case, dev="cpu"):
    kw = {"O": case["O"], "pc_type": "pred"}
    if case["label_map"] is not None:
        kw["label_map"] = torch.from_numpy(case["label_map"]).to(dev)
    if any(r["tgt_label"] is not None for r in case["rows"]):
        own = [C.ANN_LABELS[r["tgt"]] if 0 <= r["tgt"] < len(C.ANN) else 0 for r in case["rows"]]
        kw["tgt_label"] = torch.tensor([o if r["tgt_label"] is None else r["tgt_label"] for o, r in zip(own, case["rows"])],
                                       dtype=torch.int32, device=dev)
    return kw


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, what, targets=True):
    assert set(got) == set(ROW_KEYS + (TGT_KEYS if targets else ()))
    for k in ROW_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)
    if targets:
        for k in TGT_KEYS:
            assert got[k].dtype == np.int64 and np.array_equal(got[k].reshape(want[RESTATED[k]].shape), want[RESTATED[k]]), (what, k)
        assert got["tgt_object_id"].shape == (len(want["tgt_id"]), 1)


def _positions(got, first):
    """A launched batch with POSITIONS in row_obj and the restatement's key names: what compare_with_reference reads."""
    pos = np.where(got["row_obj"] >= 0, got["row_obj"] - first[:, None], -1)
    return dict(got, row_obj=pos, iou25=got["tgt_object_id_iou25"], iou50=got["tgt_object_id_iou50"],
                tgt_id=got["tgt_object_id"].reshape(-1), labels=got["obj_labels"])


def _buffers(B, O):
    """Static buffers holding values no launch writes."""
    out = {k: torch.full((B, O) if k == "row_obj" else (B,), -7, dtype=torch.int32, device=DEV) for k in ROW_KEYS[:4]}
    out["is_multiple"] = torch.full((B,), 7, dtype=torch.uint8, device=DEV)
    out["is_hard"] = torch.ones((B,), dtype=torch.bool, device=DEV)
    for k in TGT_KEYS:
        out[k] = torch.full((B, 1 if k == "tgt_object_id" else O), -7, dtype=torch.int64, device=DEV)
    return out


def _refer_targets_of(case, row_obj, tabs, tgt):
    """gps_refer_targets('pred') on a row table of this case -> the four target tensors."""
    return _np(G.refer_targets(_packed(), row_obj, tgt, tabs[0], "pred"))


# ---- matched labels ---------------------------------------------------------------------------------------------------------
def _match_labels_against_refer_targets(packed, sids):
    """packed.match_labels of every proposal of the scans == the obj_labels gps_refer_targets('pred') writes for it, in
    rows of up to 512 proposals."""
    match = packed.match_labels.cpu().numpy()
    labels = packed.labels.cpu().numpy()
    assert match.dtype == np.int32 and match.shape == (packed.n_objects,)
    rows, row_sid = [], []
    for sid in sids:
        ann = packed.scan_objects(sid)
        assert np.array_equal(match[ann.start:ann.stop], labels[ann.start:ann.stop])     # an annotated object: its own label
        props = np.asarray(packed.scan_proposals(sid), dtype=np.int32)
        for at in range(0, len(props), G.REFER_MAX_OBJ):
            rows.append(props[at:at + G.REFER_MAX_OBJ])
            row_sid.append(sid)
    table = np.full((len(rows), G.REFER_MAX_OBJ), -1, dtype=np.int32)
    for i, r in enumerate(rows):
        table[i, :len(r)] = r
    got = G.refer_targets(packed, torch.from_numpy(table).to(DEV), [0] * len(rows), row_sid, "pred")["obj_labels"].cpu().numpy()
    real = table >= 0
    assert np.array_equal(got[real], match[table[real]].astype(np.int64))
    return match, labels, table[real]


def test_match_labels_equal_refer_targets_on_the_case_scenes():
    packed = _packed()
    sids = [C.scene_id(c, b) for c in C.CASES for b in range(len(c["rows"]))]
    match, labels, props = _match_labels_against_refer_targets(packed, sids)
    assert (match[props] != labels[props]).any() and (match[props] == labels[props]).any()
    for case in C.CASES[:2]:                                                    # ... and the restatement's, proposal by proposal
        for b, row in enumerate(case["rows"]):
            r = packed.scan_proposals(C.scene_id(case, b))
            assert match[r.start:r.stop].tolist() == [C.matched_label(*q) for q in row["props"]]


def test_match_labels_equal_refer_targets_on_the_refer_scenes():
    packed = refer_cases.pack(("small", "big", "empty"), DEV)
    match, labels, props = _match_labels_against_refer_targets(packed, ["small", "big", "empty"])
    assert (match[props] != labels[props]).any()
    assert G.proposal_labels(packed).data_ptr() != packed.match_labels.data_ptr()
    assert torch.equal(G.proposal_labels(packed), packed.match_labels)


# ---- the rows ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_replay_equals_the_reference(case):
    name, M, O = case["name"], case["M"], case["O"]
    packed = _packed()
    sids, tabs, tgt_d, first = _tables(case)
    B = len(sids)
    ref = {k: GOLD[f"{name}/{k}"] for k in ("sel", "tgt_id", "n_sel", "iou25", "iou50", "labels", "n_rem", "is_multiple", "is_hard")}
    order = torch.from_numpy(GOLD[f"{name}/order"])
    want = C.restate_case(case, order=GOLD[f"{name}/order"], offsets=first)
    tgt = [r["tgt"] for r in case["rows"]]
    for ids, t, kw in ((sids, tgt, _kw(case)), (tabs, tgt_d, _kw(case, DEV))):  # described on the host / on the device
        got = _np(select_rows(packed, ids, M, tgt_obj=t, order=order, targets=True, **kw))
        for b in range(B):
            assert C.compare_with_reference(_positions(got, first), ref, b, M) == [], (name, b)
        _same(got, want, "restatement")
        plain = _np(select_rows(packed, ids, M, tgt_obj=t, order=order, **kw))   # without the target outputs: the same rows
        _same(plain, want, "no targets", targets=False)
        out = _buffers(B, O)
        ptrs = {k: v.data_ptr() for k, v in out.items()}
        res = select_rows(packed, ids, M, tgt_obj=t, order=order, targets=True, out=out, **kw)
        assert all(res[k].data_ptr() == ptrs[k] for k in out if k != "is_multiple") and res["is_multiple"].dtype == torch.bool
        _same(_np(res), want, "out")
        _same({k: v.astype(_np(res)[k].dtype) for k, v in _np(out).items()}, want, "out buffers")      # every element written
    if O == M + 1:
        kw = {k: v for k, v in _kw(case).items() if k != "O"}
        assert select_rows(packed, sids, M, tgt_obj=tgt, order=order, **kw)["row_obj"].shape == (B, M + 1)


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_and_fused_targets(case):
    """The device law equals the emulation bit for bit, `ref=False` rows included, and the four target outputs equal what
    refer_targets makes of the launch's own row table."""
    M = case["M"]
    packed = _packed()
    sids, tabs, tgt_d, first = _tables(case)      # device tables: the odd case's targets and its 1025 proposals would be refused
    kw = _kw(case, DEV)
    fills = []
    for seed in (0, 20240521, (1 << 63) + (7 << 32) + 5):
        res = select_rows(packed, tabs, M, tgt_obj=tgt_d, seed=seed, targets=True, **kw)
        got = _np(res)
        _same(got, C.restate_case(case, seed=seed, offsets=first), seed)
        two = _refer_targets_of(case, res["row_obj"], tabs, tgt_d)
        for k in TGT_KEYS:
            assert np.array_equal(got[k], two[k]), (seed, k)
        fills.append(got["row_obj"])
    assert not np.array_equal(fills[0], fills[1]) and not np.array_equal(fills[1], fills[2])
    seed_dev = torch.full((1,), (1 << 40) + 9, dtype=torch.int64, device=DEV)
    got = _np(select_rows(packed, tabs, M, tgt_obj=tgt_d, seed=77, seed_dev=seed_dev, targets=True, **kw))
    _same(got, C.restate_case(case, seed=77 + (1 << 40) + 9, offsets=first), "seed_dev")
    assert int(seed_dev.item()) == (1 << 40) + 9


def test_replay_of_the_rows_the_reference_cannot_run():
    """No hit with P > M, k > M, k = M, targets outside their scans, 1025 proposals; an order entry out of range writes -1
    and the target outputs follow the hole."""
    case = next(c for c in C.CASES if c["name"] == "pred_M5_odd")
    packed = _packed()
    sids, tabs, tgt_d, first = _tables(case)
    B, M = len(sids), case["M"]
    order = np.stack([np.random.default_rng(b).permutation(8)[:M] for b in range(B)]).astype(np.int32)
    order[0, 0], order[7, 1] = -1, 10 ** 6
    res = select_rows(packed, tabs, M, tgt_obj=tgt_d, order=torch.from_numpy(order), targets=True, **_kw(case, DEV))
    got = _np(res)
    _same(got, C.restate_case(case, order=order, offsets=first), "odd")
    two = _refer_targets_of(case, res["row_obj"], tabs, tgt_d)
    for k in TGT_KEYS:
        assert np.array_equal(got[k], two[k]), k
    assert got["n_sel"].tolist() == [5, 5, 5, 0, 0, 0, 5, 5] and got["tgt_slot"].tolist() == [-1, 4, 4, -1, -1, -1, -1, 0]
    assert (got["row_obj"][3:6] == -1).all() and (got["obj_labels"][3:6] == -100).all()
    assert got["tgt_object_id"].reshape(-1).tolist() == [4, 4, 4, 0, 0, 0, 5, 0]      # the hole of row 0 is no real slot
    assert got["row_obj"][0, 0] == -1 and got["row_obj"][7, 2] == -1 and (got["is_multiple"][[3, 4, 5, 7]] == 0).all()


def test_a_1024_proposal_scan_and_a_scan_over_the_cap():
    case = next(c for c in C.CASES if c["name"] == "pred_M5_odd")
    packed = _packed()
    sids, tabs, tgt_d, first = _tables(case)
    at = [len(r["props"]) for r in case["rows"]]
    b1024, b1025 = at.index(1024), at.index(1025)
    kw = dict(pc_type="pred", tgt_obj=[C.T], seed=3)
    got = _np(select_rows(packed, [sids[b1024]], 79, **kw))                     # no hit, no class-mate missing: the fill of 1024
    rest = [p for p, q in enumerate(case["rows"][b1024]["props"]) if C.matched_label(*q) != C.ANN_LABELS[C.T]]
    mates = [p for p in range(1024) if p not in set(rest)]
    assert got["n_sel"].tolist() == [79] and got["n_rem"].tolist() == [len(rest)] and got["tgt_slot"].tolist() == [-1]
    want = mates + [rest[i] for i in C.device_order(3, 0, len(rest))[:79 - len(mates)]]
    assert np.array_equal(got["row_obj"][0, :79], first[b1024] + np.asarray(want))
    with pytest.raises(ValueError, match="1025 proposals > 1024"):              # host ids are refused ...
        select_rows(packed, [sids[b1025]], 79, **kw)
    one = (tabs[0][b1025:b1025 + 1], tabs[1][b1025:b1025 + 1])                  # ... a device table gives the empty row
    got = _np(select_rows(packed, one, 79, targets=True, **dict(kw, tgt_obj=tgt_d[b1025:b1025 + 1])))
    assert got["n_sel"].tolist() == [0] and (got["row_obj"] == -1).all() and got["tgt_slot"].tolist() == [-1]
    assert not got["tgt_object_id_iou25"].any() and (got["obj_labels"] == -100).all() and got["tgt_object_id"].tolist() == [[0]]
    # the same proposals without the first one: 1024, a full row; ranges that leave the packed arrays are clamped
    n_obj = packed.n_objects
    cut = (torch.cat([tabs[0][b1025:b1025 + 1]] * 3), torch.tensor([[int(first[b1025]) + 1, int(first[b1025]) + 1025],
                                                                    [n_obj - 3, n_obj + 1000], [7, 2]], dtype=torch.int32, device=DEV))
    got = _np(select_rows(packed, cut, 79, **dict(kw, tgt_obj=[C.T] * 3)))
    assert got["n_sel"].tolist() == [79, 3, 0] and got["row_obj"][1, :3].tolist() == [n_obj - 3, n_obj - 2, n_obj - 1]
    assert got["tgt_slot"][0] == 1 and got["row_obj"][0, :2].tolist() == [int(first[b1025]) + 3, int(first[b1025]) + 700]


def test_pretrain_mode_selects_among_the_proposals_by_their_raw_labels():
    """_getitem_pretrain on inst_labels_pred (base.py:227-246): the 'gt' launch over the proposals' ranges."""
    import rows_cases
    case = next(c for c in C.CASES if c["name"] == "pred_M5")
    packed = _packed()
    sids, tabs, _, first = _tables(case)
    keep = G.keep_table(C.INT2CAT)
    got = _np(select_rows(packed, sids, 5, mode="pretrain", pc_type="pred", keep=keep, seed=11))
    dev = _np(select_rows(packed, tabs[1], 5, mode="pretrain", pc_type="pred", keep=keep.to(DEV), seed=11))
    scans = dict(name="raw", mode="pretrain", M=5, O=5, keep="fg", label_map=None,
                 scans=[np.asarray([q[2] for q in r["props"]], dtype=np.int32) for r in case["rows"]], tgt=[-1] * len(sids))
    want = rows_cases.restate_case(scans, seed=11, offsets=first)
    for k in ROW_KEYS:
        assert np.array_equal(got[k], want[k]) and np.array_equal(dev[k], want[k]), k


def test_wrapper_refusals_on_the_device():
    case = next(c for c in C.CASES if c["name"] == "pred_M5")
    packed = _packed()
    sids, tabs, tgt_d, _ = _tables(case)
    B, M, O = len(sids), 5, 6
    kw = dict(tgt_obj=tgt_d, pc_type="pred", targets=True)
    good = _buffers(B, O)
    select_rows(packed, tabs, M, out=good, **kw)
    for bad in (dict(good, row_obj=good["row_obj"].long()), dict(good, obj_labels=good["obj_labels"].int()),
                dict(good, tgt_object_id=good["tgt_object_id"].reshape(-1)), dict(good, tgt_object_id_iou25=good["tgt_object_id_iou25"][:, :5]),
                {k: v for k, v in good.items() if k != "tgt_object_id_iou50"}, dict(good, obj_labels=good["obj_labels"].cpu())):
        with pytest.raises(ValueError, match="out"):
            select_rows(packed, tabs, M, out=bad, **kw)
    select_rows(packed, tabs, M, out={k: good[k] for k in ROW_KEYS}, tgt_obj=tgt_d, pc_type="pred")     # no targets: six suffice
    for seed_dev in (torch.zeros(1, dtype=torch.int64), torch.zeros(2, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="seed_dev"):
            select_rows(packed, tabs, M, seed_dev=seed_dev, **kw)
    with pytest.raises(ValueError, match="label_map"):
        select_rows(packed, tabs, M, label_map=torch.zeros((2, 6), dtype=torch.int32), **kw)
    with pytest.raises(ValueError, match="one row per batch row"):
        select_rows(packed, (tabs[0], tabs[1][:3]), M, **kw)
    empty = select_rows(packed, [], M, tgt_obj=[], pc_type="pred", targets=True)
    assert empty["row_obj"].shape == (0, O) and empty["tgt_object_id"].shape == (0, 1)


def test_one_capture_with_obj_processing_post_fresh_fill_per_replay():
    """A single chain: advance the seed word on the device, select rows and targets in one launch, build the object
    tensors from the rows.  Three replays: the pinned and class blocks stay, the fill is each time the emulation's at the
    advanced seed and differs between replays."""
    case = next(c for c in C.CASES if c["name"] == "pred_M79")
    packed = _packed()
    sids, tabs, tgt_d, first = _tables(case)
    M, O, B = case["M"], case["O"], len(sids)
    seed, start = 1000, 41
    seed_dev = torch.full((1,), start, dtype=torch.int64, device=DEV)
    kw = dict(O=O, tgt_obj=tgt_d, pc_type="pred", targets=True, seed=seed, seed_dev=seed_dev)
    out = select_rows(packed, tabs, M, **kw)                  # the buffers, and the library loaded ahead of the capture
    post = G.obj_processing_post(packed, out["row_obj"], num_points=8)
    _same(_np(out), C.restate_case(case, seed=seed + start, offsets=first), "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seed_dev.add_(1)
        select_rows(packed, tabs, M, out=out, **kw)
        G.obj_processing_post(packed, out["row_obj"], num_points=8, out=post)
    seen = []
    for k in range(1, 4):
        graph.replay()
        got = _np(out)
        want = C.restate_case(case, seed=seed + start + k, offsets=first)
        _same(got, want, k)
        assert np.array_equal(post["obj_masks"].cpu().numpy(), want["row_obj"] >= 0)
        assert bool(torch.isfinite(post["obj_fts"]).all())
        seen.append(got["row_obj"])
    assert int(seed_dev.item()) == start + 3
    assert not any(np.array_equal(seen[a], seen[b]) for a, b in ((0, 1), (0, 2), (1, 2)))
    plain = C.restate_case(case, seed=0, offsets=first)
    for b in range(B):                                        # what is not drawn does not move
        head = _fixed_prefix(case, b)
        assert all(np.array_equal(s[b, :head], plain["row_obj"][b, :head]) for s in seen), b


def _fixed_prefix(case, b):
    """How many leading slots of row b no draw decides: the pinned block and the class-mates (the whole row without a fill)."""
    row = case["rows"][b]
    r = C.restate_row(row, case["M"], case["O"], case["label_map"], lambda n: np.arange(n))
    if not r["n_rem"]:
        return len(r["row"])
    l_t = C.ANN_LABELS[row["tgt"]] if row["tgt_label"] is None else row["tgt_label"]
    return int(r["iou25"].sum()) + sum(1 for s, p in enumerate(r["row"]) if not r["iou25"][s] and r["labels"][s] == l_t)


def test_end_to_end_a_batch_batch_rows_refuses():
    """select_rows(pc_type='pred') -> obj_processing_post -> ScanReferCounter on logits that are a function of the
    PROPOSAL, placed into slots by this library's own rows: the reference's ScanReferEval.batch_metrics counts, which the
    fixture holds for the same scores placed by the reference's rows."""
    from sceneverse_amd.engine import ScanReferCounter
    case = next(c for c in C.CASES if c["name"] == C.E2E_CASE)
    packed = _packed()
    rows = C.e2e_rows()
    sids = [C.scene_id(case, b) for b in rows]
    first = np.asarray([packed.scan_proposals(s).start for s in sids], dtype=np.int64)
    M, O = case["M"], case["O"]
    with pytest.raises(ValueError, match=r'select_rows\(pc_type="pred"\)'):
        G.batch_rows(packed, sids, O, proposals=True)
    order = torch.from_numpy(GOLD[f"{case['name']}/order"][rows])
    sel = select_rows(packed, sids, M, tgt_obj=[case["rows"][b]["tgt"] for b in rows], order=order, pc_type="pred", targets=True)
    assert (sel["n_sel"] == M).all() and bool((sel["n_rem"] > 0).any())
    post = G.obj_processing_post(packed, sel["row_obj"], num_points=16)
    assert post["obj_fts"].shape == (len(rows), O, 16, 6) and bool(torch.isfinite(post["obj_fts"]).all())
    assert torch.equal(post["obj_masks"].sum(1).int(), sel["n_sel"])
    pos = np.where(sel["row_obj"].cpu().numpy() >= 0, sel["row_obj"].cpu().numpy() - first[:, None], -1)
    logits = torch.from_numpy(C.slot_logits(case, rows, pos)).to(DEV)
    counter = ScanReferCounter(DEV)
    counter.update(logits, sel)
    got = counter.result(include_count=True)
    ref = GOLD["e2e/metrics"]
    for i, key in enumerate(refer_cases.METRIC_KEYS):
        assert tuple(got[key]) == tuple(ref[i].tolist()), key
    assert 0 < ref[1, 0] < ref[0, 0] < len(rows) and 0 < ref[2, 1] < len(rows)   # hits at 0.5 < at 0.25 < all; unique rows exist
