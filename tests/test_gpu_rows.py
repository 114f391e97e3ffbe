"""The device-side object selection on the GPU (csrc/gps_obj_select.hip through sceneverse_amd/data/gpu_objects.py:
select_rows): replays of the reference's shuffles against the reference's own outputs (tests/golden/rows_ref.npz), the
device fill law against its numpy emulation (tests/rows_cases.py), in-place outputs, one graph capture together with
refer_targets, and one run through obj_processing_post.  Every comparison is exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import rows_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_objects import select_rows  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "rows_ref.npz"))
OUT_KEYS = ("row_obj", "tgt_slot", "n_sel", "n_rem", "is_multiple", "is_hard")
_CACHE = {}


def _pack(case, points=1):
    """The case's scans as one PackedScans, `points` points per object -> (packed, scan ids, first global id per row)."""
    key = (case["name"], points)
    if key not in _CACHE:
        rng = np.random.default_rng(len(case["scans"]))
        packed, sids = G.PackedScans(DEV), []
        for b, labels in enumerate(case["scans"]):
            n = len(labels)
            inst = np.repeat(np.arange(n), points)
            packed.add_scan(f"scan{b}", rng.random((n * points, 3)).astype(np.float32),
                            rng.integers(0, 256, size=(n * points, 3)).astype(np.uint8), inst, list(range(n)),
                            inst_labels=[int(l) for l in labels])
            sids.append(f"scan{b}")
        packed.finalize()
        _CACHE[key] = (packed, sids, np.asarray([packed.scan_objects(s).start for s in sids], dtype=np.int64))
    return _CACHE[key]


def _kw(case):
    kw = {"keep": torch.from_numpy(C.keep_of(case))}
    if case["label_map"] is not None:
        kw["label_map"] = torch.from_numpy(case["label_map"])
    return kw


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


def _same(got, want, what):
    assert set(got) == set(OUT_KEYS)
    for k in OUT_KEYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), (what, k)


def _buffers(B, O):
    """Static buffers holding values no launch writes."""
    out = {k: torch.full((B, O) if k == "row_obj" else (B,), -7, dtype=torch.int32, device=DEV) for k in OUT_KEYS[:4]}
    out["is_multiple"] = torch.full((B,), 7, dtype=torch.uint8, device=DEV)
    out["is_hard"] = torch.ones((B,), dtype=torch.bool, device=DEV)
    return out


def _device_args(packed, sids, case):
    return G.scan_ranges(packed, sids), torch.tensor(case["tgt"], dtype=torch.int64, device=DEV)


@pytest.mark.parametrize("case", C.REF_CASES, ids=C.REF_IDS)
def test_replay_equals_the_reference(case):
    name, M, O, mode = case["name"], case["M"], case["O"], case["mode"]
    packed, sids, first = _pack(case)
    B = len(sids)
    sel = GOLD[f"{name}/sel"]
    want = {k: GOLD[f"{name}/{k}"] for k in OUT_KEYS[1:]}
    want["row_obj"] = np.where(sel >= 0, sel + first[:, None], -1).astype(np.int32)
    order = torch.from_numpy(GOLD[f"{name}/order"])
    tgt = case["tgt"] if mode == "refer" else None
    kw = dict(_kw(case), mode=mode, O=O, order=order)
    res = select_rows(packed, sids, M, tgt_obj=tgt, **kw)                    # the batch described on the host
    assert all(res[k].dtype == torch.int32 for k in OUT_KEYS[:4]) and res["is_hard"].dtype == torch.bool
    _same(_np(res), want, "host")
    ranges, tgt_d = _device_args(packed, sids, case)
    kw_d = {k: v.to(DEV) for k, v in kw.items() if torch.is_tensor(v)}
    kw_d.update(mode=mode, O=O)
    res = select_rows(packed, ranges, M, tgt_obj=tgt_d if mode == "refer" else None, **kw_d)     # ... on the device
    _same(_np(res), want, "device")
    for args in ((sids, tgt, kw), (ranges, tgt_d if mode == "refer" else None, kw_d)):
        out = _buffers(B, O)
        ptrs = {k: v.data_ptr() for k, v in out.items()}
        res = select_rows(packed, args[0], M, tgt_obj=args[1], out=out, **args[2])
        assert all(out[k].data_ptr() == ptrs[k] for k in out) and res["row_obj"].data_ptr() == ptrs["row_obj"]
        assert res["is_hard"].data_ptr() == ptrs["is_hard"] and res["is_multiple"].dtype == torch.bool
        _same(_np(res), want, "out")
        _same({k: v.astype(want[k].dtype) for k, v in _np(out).items()}, want, "out buffers")   # every element written
    if mode == "refer" and O > M:                            # the default O of 'refer' mode is M + 1
        assert select_rows(packed, sids, M, tgt_obj=tgt, **{k: v for k, v in kw.items() if k != "O"})["row_obj"].shape == (B, M + 1)


@pytest.mark.parametrize("case", C.CASES, ids=C.CASE_IDS)
def test_device_law_equals_the_emulation(case):
    M, O, mode = case["M"], case["O"], case["mode"]
    packed, sids, first = _pack(case)
    ranges, tgt_d = _device_args(packed, sids, case)         # device tables: the odd cases' targets would be refused on the host
    kw = {k: v.to(DEV) for k, v in _kw(case).items()}
    kw.update(mode=mode, O=O, tgt_obj=tgt_d if mode == "refer" else None)
    fills = []
    for seed in (0, 20240521, (1 << 63) + (7 << 32) + 5):
        got = _np(select_rows(packed, ranges, M, seed=seed, **kw))
        _same(got, C.restate_case(case, seed=seed, offsets=first), seed)
        fills.append(got["row_obj"])
    if case["ref"]:
        assert not np.array_equal(fills[0], fills[1]) and not np.array_equal(fills[1], fills[2])
    seed_dev = torch.full((1,), (1 << 40) + 9, dtype=torch.int64, device=DEV)
    got = _np(select_rows(packed, ranges, M, seed=77, seed_dev=seed_dev, **kw))
    _same(got, C.restate_case(case, seed=77 + (1 << 40) + 9, offsets=first), "seed_dev")
    assert int(seed_dev.item()) == (1 << 40) + 9


MAXR = 8                                                     # the odd rows' orders: prefixes of permutations of range(8)


def test_replay_of_the_rows_the_reference_cannot_run():
    """Labels outside the table, targets outside their scans; an order entry out of range writes -1."""
    for name in ("refer_M5_odd", "pretrain_M5_odd"):
        case = next(c for c in C.CASES if c["name"] == name)
        packed, sids, first = _pack(case)
        ranges, tgt_d = _device_args(packed, sids, case)
        B, M = len(sids), case["M"]
        order = np.stack([np.random.default_rng(b).permutation(MAXR)[:M] for b in range(B)]).astype(np.int32)
        order[0, 0], order[1, 1] = -1, 10 ** 6
        kw = {k: v.to(DEV) for k, v in _kw(case).items()}
        got = _np(select_rows(packed, ranges, M, O=case["O"], mode=case["mode"], order=torch.from_numpy(order),
                              tgt_obj=tgt_d if case["mode"] == "refer" else None, **kw))
        want = C.restate_case(case, order=order, offsets=first)
        _same(got, want, name)
        if case["mode"] == "refer":
            assert got["n_sel"][-3:].tolist() == [0, 0, 0] and got["tgt_slot"][-3:].tolist() == [-1, -1, -1]
            assert (got["row_obj"][-3:] == -1).all()
        assert (got["n_rem"] > 0).any()


def test_a_1024_position_scan_and_a_scan_over_the_cap():
    case = next(c for c in C.CASES if c["name"] == "pretrain_M79")
    packed, sids, first = _pack(case)
    b = [len(s) for s in case["scans"]].index(1024)
    ranges = G.scan_ranges(packed, sids)
    keep = torch.ones(C.N_LABELS, dtype=torch.bool, device=DEV)            # everything kept: n_rem = 1024
    got = _np(select_rows(packed, ranges[b:b + 1], 79, mode="pretrain", keep=keep, seed=3))
    assert got["n_rem"].tolist() == [1024] and got["n_sel"].tolist() == [79]
    want = first[b] + C.device_order(3, 0, 1024)[:79]
    assert np.array_equal(got["row_obj"][0], want)
    # the same objects seen as the tail of a range of 1025: over the cap, an empty row; host ids are refused instead
    over = torch.tensor([[int(first[b]) - 1, int(first[b]) + 1024], [int(first[b]), int(first[b]) + 1024]],
                        dtype=torch.int32, device=DEV)
    got = _np(select_rows(packed, over, 79, mode="pretrain", keep=keep, seed=3))
    assert got["n_sel"].tolist() == [0, 79] and (got["row_obj"][0] == -1).all() and got["n_rem"].tolist() == [0, 1024]
    # a range that leaves the packed arrays is clamped, never followed
    n_obj = packed.n_objects
    wild = torch.tensor([[-5, 3], [n_obj - 2, n_obj + 1000], [7, 2]], dtype=torch.int32, device=DEV)
    got = _np(select_rows(packed, wild, 79, mode="pretrain", keep=keep, seed=3))
    assert got["n_sel"].tolist() == [3, 2, 0]
    assert got["row_obj"][0, :3].tolist() == [0, 1, 2] and got["row_obj"][1, :2].tolist() == [n_obj - 2, n_obj - 1]


def test_wrapper_refusals_on_the_device():
    case = next(c for c in C.CASES if c["name"] == "refer_M5")
    packed, sids, _ = _pack(case)
    B, M, O = len(sids), 5, 6
    kw = dict(tgt_obj=case["tgt"], keep=torch.from_numpy(C.keep_fg()))
    good = _buffers(B, O)
    select_rows(packed, sids, M, out=good, **kw)
    for bad in (dict(good, row_obj=good["row_obj"].long()), dict(good, row_obj=good["row_obj"][:, :5]),
                dict(good, n_sel=good["n_sel"][:3]), dict(good, is_hard=good["is_hard"].int()),
                {k: v for k, v in good.items() if k != "n_rem"}, dict(good, tgt_slot=good["tgt_slot"].cpu())):
        with pytest.raises(ValueError, match="out"):
            select_rows(packed, sids, M, out=bad, **kw)
    for order in (torch.zeros((B, M - 1), dtype=torch.int32), torch.zeros((B + 1, M), dtype=torch.int32),
                  torch.zeros((B, M)), torch.zeros(B * M, dtype=torch.int32)):
        with pytest.raises(ValueError, match="order"):
            select_rows(packed, sids, M, order=order, **kw)
    for seed_dev in (torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32, device=DEV),
                     torch.zeros(2, dtype=torch.int64, device=DEV)):
        with pytest.raises(ValueError, match="seed_dev"):
            select_rows(packed, sids, M, seed_dev=seed_dev, **kw)
    with pytest.raises(ValueError, match="keep"):
        select_rows(packed, sids, M, tgt_obj=case["tgt"], keep=torch.ones((B + 1, C.N_LABELS), dtype=torch.bool))
    with pytest.raises(ValueError, match="label_map"):
        select_rows(packed, sids, M, label_map=torch.zeros(C.N_LABELS + 1, dtype=torch.int32), **kw)
    empty = select_rows(packed, [], M, tgt_obj=[], keep=kw["keep"])
    assert empty["row_obj"].shape == (0, O) and empty["n_sel"].shape == (0,)


def test_one_capture_with_refer_targets_fresh_fill_per_replay():
    """A single chain: advance the seed word on the device, select the rows, derive the targets from them.  Three
    replays, three different fills, each the emulation's at the advanced seed."""
    case = next(c for c in C.CASES if c["name"] == "refer_M79")
    packed, sids, first = _pack(case)
    M, O = case["M"], case["O"]
    ranges, tgt_d = _device_args(packed, sids, case)
    keep = torch.from_numpy(C.keep_fg()).to(DEV)
    seed, start = 1000, 41
    seed_dev = torch.full((1,), start, dtype=torch.int64, device=DEV)
    kw = dict(O=O, tgt_obj=tgt_d, keep=keep, seed=seed, seed_dev=seed_dev)
    out = select_rows(packed, ranges, M, **kw)               # the buffers, and the library loaded ahead of the capture
    tout = G.refer_targets(packed, out["row_obj"], tgt_d, ranges, "gt")
    _same(_np(out), C.restate_case(case, seed=seed + start, offsets=first), "eager")
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seed_dev.add_(1)
        select_rows(packed, ranges, M, out=out, **kw)
        G.refer_targets(packed, out["row_obj"], tgt_d, ranges, "gt", out=tout)
    labels = packed.labels.cpu().numpy()
    seen = []
    for k in range(1, 4):
        graph.replay()
        got, tg = _np(out), _np(tout)
        want = C.restate_case(case, seed=seed + start + k, offsets=first)
        _same(got, want, k)
        assert np.array_equal(tg["tgt_object_id"].reshape(-1), want["tgt_slot"])
        onehot = np.arange(O)[None, :] == want["tgt_slot"][:, None]
        assert np.array_equal(tg["tgt_object_id_iou25"], onehot) and np.array_equal(tg["tgt_object_id_iou50"], onehot)
        assert np.array_equal(tg["obj_labels"], np.where(want["row_obj"] >= 0, labels[want["row_obj"]], -100))
        seen.append(got["row_obj"])
    assert int(seed_dev.item()) == start + 3
    assert not any(np.array_equal(seen[a], seen[b]) for a, b in ((0, 1), (0, 2), (1, 2)))


def test_end_to_end_a_scan_batch_rows_refuses():
    """select_rows -> obj_processing_post -> refer_targets on scans with more than M foreground objects."""
    full = next(c for c in C.CASES if c["name"] == "refer_M5")
    rows = [b for b, s in enumerate(full["scans"]) if 8 < len(s) < 40][:6]
    case = dict(full, name="refer_M5_e2e", scans=[full["scans"][b] for b in rows], tgt=[full["tgt"][b] for b in rows])
    packed, sids, first = _pack(case, points=5)
    M, O = 5, 6
    with pytest.raises(ValueError, match="> max_obj_len"):
        G.batch_rows(packed, sids, O)
    order = torch.from_numpy(GOLD["refer_M5/order"][rows])
    sel = select_rows(packed, sids, M, tgt_obj=case["tgt"], keep=torch.from_numpy(C.keep_fg()), order=order)
    gold_sel = GOLD["refer_M5/sel"][rows]
    assert np.array_equal(sel["n_sel"].cpu().numpy(), GOLD["refer_M5/n_sel"][rows]) and (GOLD["refer_M5/n_rem"][rows] > 0).any()
    post = G.obj_processing_post(packed, sel["row_obj"], num_points=16)
    assert post["obj_fts"].shape == (len(rows), O, 16, 6) and bool(torch.isfinite(post["obj_fts"]).all())
    assert torch.equal(post["obj_masks"].sum(1).int(), sel["n_sel"])
    tg = G.refer_targets(packed, sel["row_obj"], case["tgt"], sids, "gt")
    want_labels = np.stack([np.where(gold_sel[i] >= 0, case["scans"][i][np.maximum(gold_sel[i], 0)], -100)
                            for i in range(len(rows))]).astype(np.int64)
    assert np.array_equal(tg["obj_labels"].cpu().numpy(), want_labels)
    assert np.array_equal(tg["tgt_object_id"].cpu().numpy().reshape(-1), GOLD["refer_M5/tgt_slot"][rows])
    assert torch.equal(tg["tgt_object_id"].reshape(-1).int(), sel["tgt_slot"])
    assert np.array_equal(sel["is_multiple"].cpu().numpy(), GOLD["refer_M5/is_multiple"][rows])
