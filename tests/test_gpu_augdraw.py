"""The device-drawn loader on the GPU (sceneverse_amd/data/gpu_objects.py, gpu_items.py, gpu_batch.py -> libgps_hip.so):
  1. the seed-word entries of the two object launches against their by-value forms, bit for bit;
  2. gps_aug_draw's table (both modes) against the numpy / math mirror of tests/augdraw_cases.py;
  3. obj_processing_aug fed with the device-drawn table against the same launch fed with the mirror's table;
  4. gps_item_rows against its restatement, and select_rows / text_batch fed with its outputs;
  5. pretrain_batch captured once and replayed with an advancing seed word.

The tolerance of 2.: the integer part of the law (flags, flips, jitter scales, the axis-aligned table and its products,
the build_rotate_mat table) and the scale (one multiply, one add) must be EQUAL.  The free-angle rotations, the
translations and the colour deltas pass through sin / cos / log / sqrt / cospi, where the device's libm and the
host's differ: the largest distance measured over the cases below is FREE_ULPS float64 ulps (a translation or colour
delta in ulps of its own value, a rotation entry in ulps of 1.0, the scale of a rotation matrix), and the test allows
twice that, since the three-matrix product adds a few roundings on top of libm's.  A bound above 2^-40 relative would be
a defect, not a tolerance (asserted).
"""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from oracle import obj_processing as OP  # noqa: E402
import augdraw_cases as A  # noqa: E402
import objaug_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_batch import pretrain_batch  # noqa: E402
from sceneverse_amd.data.gpu_items import PackedItems, item_rows  # noqa: E402
from sceneverse_amd.data.gpu_text import PackedTexts, text_batch  # noqa: E402

DEV = "cuda"
FREE_ULPS = 2.0                                  # measured on the MI355X over the cases of test 2
assert 2 * FREE_ULPS * 2.0 ** -52 <= 2.0 ** -40

# three scans, KS-style sizes: a 1-point object, objects below / at / above both num_points (256, 300), a 3000-point one
SCANS = (("s0", [1, 7, 255, 256, 257, 900, 3000]), ("s1", [299, 300, 301, 40]), ("s2", [120, 512, 5, 64, 33, 700]))
N_LABELS = 10
POINTS = (256, 300)                              # the register-slot boundary: one full slot, a second partly filled
W = (0, 1, 1 << 40)


def _scans(records=True):
    """The three resident scans; every annotated object is a proposal too (IoU 1 with itself), plus the union of the
    first two objects."""
    packed = G.PackedScans(DEV, records=records)
    for n, (sid, ks) in enumerate(SCANS):
        objs = OP.synth_scene(np.random.default_rng(40 + n), len(ks), np.uint8, ks)
        pts = np.concatenate([p for p, _ in objs], 0)
        col = np.concatenate([c for _, c in objs], 0)
        lab = np.concatenate([np.full(len(p), 100 + i) for i, (p, _) in enumerate(objs)])
        order = np.random.default_rng(n).permutation(len(lab))      # interleaved across instances, as on disk
        pts, col, lab = pts[order], col[order], lab[order]
        inst = [100 + i for i in range(len(ks))]
        labels = [1 + (i % 4) for i in range(len(ks))]
        packed.add_scan(sid, pts, col, lab, inst, inst_labels=labels)
        masks = np.stack([lab == i for i in inst] + [(lab == inst[0]) | (lab == inst[1])], 0)
        packed.add_proposals(sid, pts, col, masks, labels + [labels[0]])
    return packed.finalize()


@pytest.fixture(scope="module")
def scans():
    return {True: _scans(True), False: _scans(False)}


def _texts():
    rng = np.random.default_rng(5)
    texts = PackedTexts(DEV)
    for n in (20, 31, 3, 45, 17, 26, 60, 9, 12, 38):
        texts.add_text(rng.integers(1000, 30000, n))
    return texts.finalize()


# (scan, target instance, tgt_label, sentence): 7 items over the 3 scans
ITEMS = (("s0", 103, 4, 0), ("s1", 100, 1, 1), ("s2", 105, 2, 2), ("s0", 106, 3, 3), ("s2", 101, 2, 4), ("s1", 103, 4, 5),
         ("s0", 100, 1, 6))
CAPS = {"s0": [7, 8, 9], "s1": [9, 7]}            # s2 has no caption: the default
DEFAULT_CAP = 8


def _items(packed):
    items = PackedItems(packed, default_caption=DEFAULT_CAP)
    for it in ITEMS:
        items.add_item(*it)
    for sid, caps in CAPS.items():
        items.set_captions(sid, caps)
    return items.finalize()


def _item_table(packed):
    sids = [s for s, _ in SCANS]
    return dict(item_scan=[sids.index(s) for s, *_ in ITEMS], item_tgt=[t - 100 for _, t, _, _ in ITEMS],
                item_label=[l for *_, l, _ in ITEMS], item_sent=[x for *_, x in ITEMS],
                scan_range=[[packed.scan_objects(s).start, packed.scan_objects(s).stop] for s in sids],
                prop_range=[[packed.scan_proposals(s).start, packed.scan_proposals(s).stop] for s in sids],
                caps=[CAPS.get(s, []) for s in sids], default_caption=DEFAULT_CAP)


def _word(w):
    return torch.tensor([w], dtype=torch.int64, device=DEV)


# ---- 1. the seed-word contract ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("records", [True, False], ids=["rec16", "two_arrays"])
@pytest.mark.parametrize("P", POINTS)
def test_seed_word_equals_seed_by_value(scans, records, P):
    packed = scans[records]
    assert packed.records == records
    rows = G.batch_rows(packed, [s for s, _ in SCANS], 8).to(DEV)             # padding slots in every scene
    aug = G.draw_aug_table(C.ALL_KNOBS, "train", 3, 8, seed=11, device=DEV)     # scale, jitter: every stream is read
    rot = G.draw_rot_table("train", True, 3, 8, seed=3, device=DEV)          # the mirror's indices at this seed: 0, 1, 3
    assert (rot[1].reshape(3, 8)[:, 0] >= 0).tolist() == [False, True, True]
    s = 5
    calls = {"post": lambda **kw: G.obj_processing_post(packed, rows, P, rot=rot, need_boxes=True, **kw),
             "aug": lambda **kw: G.obj_processing_aug(packed, rows, P, aug=aug, need_boxes=True, **kw)}
    for name, call in calls.items():
        plain = call(seed=s)
        none = call(seed=s, seed_dev=None)
        fts = []
        for w in W:
            got, want = call(seed=s, seed_dev=_word(w)), call(seed=s + w)
            for k in ("obj_fts", "obj_locs", "obj_boxes", "obj_masks"):
                assert torch.equal(got[k], want[k]), (name, w, k)
                if w == 0:
                    assert torch.equal(got[k], plain[k]) and torch.equal(none[k], plain[k]), (name, k)
            nxt = call(seed=s, seed_dev=_word(w + 1))
            assert not torch.equal(nxt["obj_fts"], got["obj_fts"]), (name, w)
            fts.append(got["obj_fts"])
        assert not torch.equal(fts[0], fts[2]) and not torch.equal(fts[1], fts[2])
        assert plain["obj_masks"].tolist() == [[True] * len(ks) + [False] * (8 - len(ks)) for _, ks in SCANS]
    # the word wraps like the seed does
    a = calls["aug"](seed=(1 << 64) - 1, seed_dev=_word(3))
    b = calls["aug"](seed=2)
    assert torch.equal(a["obj_fts"], b["obj_fts"])


# ---- 2. the device table against the mirror ---------------------------------------------------------------------------------
EXACT = [0, 1, 2, 3, 4] + list(range(14, 23)) + list(range(41, 48))            # flags, scale, jitter scale, flip, reserved
FREE = {"scene_trans": range(5, 8), "obj_trans": range(8, 11), "rgb": range(11, 14)}
ROTS = {"scene": range(23, 32), "obj": range(32, 41)}


def _free_ulps(dev_rows, mir_rows, table_rot):
    """Largest distance device - mirror over the libm entries, in float64 ulps (see the module docstring); the exact
    entries are asserted equal on the way."""
    worst = 0.0
    for r, (d, m) in enumerate(zip(dev_rows, mir_rows)):
        assert (d is None) == (m is None), r
        if m is None:
            continue
        assert np.array_equal(d[EXACT], m[EXACT]), (r, d[EXACT], m[EXACT])
        for name, at in ROTS.items():
            at = list(at)
            if table_rot[name]:
                assert np.array_equal(d[at], m[at]), (r, name, d[at], m[at])
            else:
                worst = max(worst, float(np.abs(d[at] - m[at]).max() / np.spacing(1.0)))
        for name, at in FREE.items():
            at = list(at)
            live = m[at] != 0.0
            assert np.array_equal(d[at] == 0.0, ~live)
            if live.any():
                worst = max(worst, float((np.abs(d[at] - m[at])[live] / np.spacing(np.abs(m[at][live]))).max()))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_device_table_equals_the_mirror(name):
    cfg, B, O = A.CONFIGS[name], 5, 4
    table_rot = A.table_rotations(cfg)
    assert table_rot == {"published": {"scene": True, "obj": False}, "all": {"scene": False, "obj": False},
                         "half_axis": {"scene": False, "obj": False}, "half_axis_table": {"scene": True, "obj": True},
                         "published_half": {"scene": True, "obj": False}}[name]
    worst, silent = 0.0, 0
    for seed, w in ((3, None), (1 << 33, 12345)):
        tab = G.draw_aug_table(cfg, "train", B, O, seed=seed, seed_dev=None if w is None else _word(w), device=DEV)
        ent, row_aug = tab.entries.cpu().numpy(), tab.row_aug.cpu().numpy()
        m_ent, m_row = A.mirror_table(cfg, "train", B, O, seed + (w or 0))
        assert ent.shape == m_ent.shape == (B * O if A.per_object(cfg) else B, A.STRIDE)
        assert np.array_equal(row_aug, m_row), (row_aug, m_row)
        assert tab.has_scale == (not name.startswith("published"))
        assert not ent[np.setdiff1d(np.arange(len(ent)), row_aug[row_aug >= 0])].any()      # a silent entry is zeros
        silent += int((row_aug < 0).sum())
        worst = max(worst, _free_ulps(A.resolve(ent, row_aug), A.resolve(m_ent, m_row), table_rot))
    print(f"{name}: largest libm distance to the mirror {worst:.2f} float64 ulps, {silent} silent rows")
    assert worst <= 2 * FREE_ULPS
    if name.startswith("published"):             # nothing passes through libm; p = 1.0: every scene fires, 0.5: some do
        assert worst == 0.0 and (silent == 0) == (name == "published") and silent < 2 * B * O


@pytest.mark.gpu
def test_rotation_table_equals_the_mirror_and_out_is_written_in_place():
    B, O = 37, 3
    seed, w = 21, 1 << 40
    out = {"rot": torch.zeros((B, 3, 3), device=DEV), "row_rot": torch.zeros(B * O, dtype=torch.int32, device=DEV)}
    mats, row_rot = G.draw_rot_table("train", True, B, O, seed=seed, seed_dev=_word(w), out=out)
    assert mats is out["rot"] and row_rot is out["row_rot"]
    idx, m_mats, m_rows = A.mirror_rot("train", True, B, O, seed + w)
    assert set(idx.tolist()) == {0, 1, 2, 3}
    assert np.array_equal(row_rot.cpu().numpy(), m_rows)
    got = mats.cpu().numpy()
    assert np.array_equal(got[idx != 0], m_mats[idx != 0]) and np.array_equal(got[idx == 0], np.tile(np.eye(3, dtype=np.float32), (int((idx == 0).sum()), 1, 1)))
    # the reference's own matrices (oracle/obj_processing.py restates build_rotate_mat)
    for a in (1, 2, 3):
        th = OP.ROTATE_ANGLES[a]
        ref = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], dtype=np.float32)
        assert np.array_equal(m_mats[idx == a][0], ref)
    tab_out = {"entries": torch.zeros((B, 48), dtype=torch.float64, device=DEV), "row_aug": torch.zeros(B * O, dtype=torch.int32, device=DEV)}
    tab = G.draw_aug_table(C.PUBLISHED, "train", B, O, seed=1, out=tab_out)
    assert tab.entries is tab_out["entries"] and tab.row_aug is tab_out["row_aug"] and (tab.row_aug >= 0).all()
    with pytest.raises(ValueError, match="entries"):
        G.draw_aug_table(C.ALL_KNOBS, "train", B, O, out=tab_out)             # per-object: B * O entries


# ---- 3. end to end ------------------------------------------------------------------------------------------------------------
def _scale_ulp(ref, axes):
    """One float32 ulp of each object's quantity scale: spacing(max |ref| over the object's entries)."""
    return np.spacing(np.abs(ref).max(axes, keepdims=True).astype(np.float32)).astype(np.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["published", "all"])
@pytest.mark.parametrize("P", POINTS)
def test_device_table_end_to_end(scans, name, P):
    cfg, packed = A.CONFIGS[name], scans[True]
    B, O, seed = 3, 8, 77
    rows = G.batch_rows(packed, [s for s, _ in SCANS], O).to(DEV)
    dev_tab = G.draw_aug_table(cfg, "train", B, O, seed=seed, device=DEV)
    ent, row_aug = A.mirror_table(cfg, "train", B, O, seed)
    mir_tab = G.AugTable(torch.from_numpy(ent).to(DEV), torch.from_numpy(row_aug).to(DEV), dev_tab.has_scale)
    a = G.obj_processing_aug(packed, rows, P, aug=dev_tab, seed=seed, need_boxes=True)
    b = G.obj_processing_aug(packed, rows, P, aug=mir_tab, seed=seed, need_boxes=True)
    assert torch.equal(a["obj_masks"], b["obj_masks"])
    if name == "published":
        for k in ("obj_fts", "obj_locs", "obj_boxes"):
            assert torch.equal(a[k], b[k]), k
        return
    fa, fb = (x["obj_fts"].cpu().numpy().astype(np.float64) for x in (a, b))
    for what, got, ref, axes in (("xyz", fa[..., :3], fb[..., :3], (2, 3)), ("rgb", fa[..., 3:], fb[..., 3:], (2, 3)),
                                 ("locs", *(x["obj_locs"].cpu().numpy().astype(np.float64) for x in (a, b)), (2,)),
                                 ("boxes", *(x["obj_boxes"].cpu().numpy().astype(np.float64) for x in (a, b)), (2,))):
        err, unit = np.abs(got - ref), _scale_ulp(ref, axes)
        print(f"{what}: max err {err.max():.3e}, max err / unit {np.max(err / np.maximum(unit, 1e-300)):.3f}, "
              f"equal {np.mean(got == ref):.4f}")
        assert np.all(err <= unit), what


# ---- 4. item_rows --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_item_rows_against_the_restatement_and_downstream(scans):
    packed = scans[True]
    items, texts, table = _items(packed), _texts(), _item_table(packed)
    ids = [3, 1, 2, 6, 4, 0, 5, -1, len(ITEMS)]                                # one id -1, one past the end
    pick = [2, 1, 0, 5, 0, 1, 0, 0, 0]                                         # 5: outside its scan's captions -> 0
    got = item_rows(items, ids, pick=pick)
    want = A.restate_item_rows(table, ids, pick=pick)
    for k, v in want.items():
        assert got[k].dtype == torch.int32 and np.array_equal(got[k].cpu().numpy(), v), (k, got[k], v)
    assert want["cap_idx"].tolist() == [9, 7, DEFAULT_CAP, 7, DEFAULT_CAP, 8, 9, -1, -1]
    seed, w = 9, 1 << 35
    ids_d = torch.tensor(ids, dtype=torch.int64, device=DEV)
    drawn = item_rows(items, ids_d, seed=seed, seed_dev=_word(w))
    want = A.restate_item_rows(table, ids, seed=seed + w)
    for k, v in want.items():
        assert np.array_equal(drawn[k].cpu().numpy(), v), k
    caps = {tuple(item_rows(items, ids_d, seed=s)["cap_idx"].tolist()) for s in range(6)}
    assert len(caps) > 1
    # downstream: the launches fed with the device tables give the rows the host-built tables give (the defined rows
    # come first, so a row has the same number -- which the fill's key carries -- in both batches)
    good = ids[:len(ITEMS)]
    sids, tgt = [ITEMS[i][0] for i in good], [ITEMS[i][1] - 100 for i in good]
    keep = torch.ones(N_LABELS, dtype=torch.bool)
    live = torch.tensor([0 <= i < len(ITEMS) for i in ids])
    assert live.tolist() == [True] * len(good) + [False, False]
    for pc_type in ("gt", "pred"):
        dev_ranges = (got["scan_range"], got["prop_range"]) if pc_type == "pred" else got["scan_range"]
        kw = dict(mode="refer", keep=keep, seed=4, pc_type=pc_type, targets=pc_type == "pred")
        a = G.select_rows(packed, dev_ranges, 5, tgt_obj=got["tgt_obj"], **kw)
        b = G.select_rows(packed, sids, 5, tgt_obj=tgt, **kw)
        assert len(b) >= 6 and (b["n_rem"] > 0).any()
        for k in b:
            assert torch.equal(a[k][:len(good)], b[k]), (pc_type, k)
        assert (a["n_sel"].cpu()[~live] == 0).all() and (a["row_obj"].cpu()[~live] == -1).all()      # the undefined rows: empty
        assert (a["n_sel"].cpu()[live] > 0).all()
    ta = text_batch(texts, got["sent_idx"], got["cap_idx"], mask=False)
    tb = text_batch(texts, [ITEMS[i][3] for i in good], want_caps(good, pick, ids), mask=False)
    for k in ("txt_ids", "txt_masks", "scene_txt_ids", "scene_txt_masks"):
        assert torch.equal(ta[k][live.to(DEV)], tb[k]), k
        dead = ta[k][~live.to(DEV)]
        assert (dead[:, 2:] == 0).all()                                        # an empty text: [CLS] [SEP] and padding
    with pytest.raises(ValueError, match="out"):
        item_rows(items, ids, out={"scan_range": torch.zeros((9, 2), dtype=torch.int32, device=DEV)})


def want_caps(good, pick, ids):
    """The caption text ids of the defined rows under the replayed picks, built on the host."""
    caps = []
    for j, i in enumerate(ids):
        if not 0 <= i < len(ITEMS):
            continue
        c = CAPS.get(ITEMS[i][0], [])
        caps.append(DEFAULT_CAP if not c else c[pick[j] if 0 <= pick[j] < len(c) else 0])
    return caps


# ---- 5. capture ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("pc_type", ["gt", "pred"])
def test_pretrain_batch_replays_redraw_from_the_seed_word(scans, pc_type):
    packed = scans[True]
    items, texts = _items(packed), _texts()
    B, O, M, P, seed = 4, 6, 5, 256, 1000
    ids = torch.tensor([0, 1, 2, 6], dtype=torch.int32, device=DEV)             # s0 (7 objects) is cropped to 5
    keep = torch.ones(N_LABELS, dtype=torch.bool, device=DEV)
    kw = dict(O=O, num_points=P, pc_type=pc_type, aug_cfg=C.ALL_KNOBS, keep=keep, max_seq_len=24, max_scene_cap_len=64)
    seed_dev = _word(3)
    out = pretrain_batch(packed, texts, items, ids, M, seed=seed, seed_dev=seed_dev, **kw)     # the buffers; library loaded
    for k in ("obj_fts", "obj_locs", "obj_masks", "obj_labels", "obj_sem_masks", "txt_ids", "txt_masks", "masked_lm_labels",
              "scene_txt_ids", "scene_txt_masks", "tgt_object_id", "tgt_object_id_iou25", "tgt_object_id_iou50",
              "is_multiple", "is_hard"):
        assert k in out, k
    assert out["obj_fts"].shape == (B, O, P, 6) and out["tgt_object_id"].shape == (B, 1) and out["txt_ids"].shape == (B, 24)
    assert out["n_sel"].tolist()[0] == M and out["n_rem"].tolist()[0] > 0 and out["n_sel"].tolist()[1] < O
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    torch.cuda.synchronize()
    side, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(graph, stream=side):
        res = pretrain_batch(packed, texts, items, ids, M, seed=seed, seed_dev=seed_dev, out=out, **kw)
    assert {k: v.data_ptr() for k, v in res.items()} == ptrs
    seen = []
    for w in (3, 4):
        graph.replay()
        torch.cuda.synchronize()
        got = {k: v.clone() for k, v in out.items()}
        want = pretrain_batch(packed, texts, items, ids, M, seed=seed + w, **kw)
        assert set(want) == set(got)
        for k in want:
            assert torch.equal(got[k], want[k]), (pc_type, w, k)
        seen.append(got)
        seed_dev.add_(1)
    assert int(seed_dev.item()) == 5
    assert not torch.equal(seen[0]["obj_fts"], seen[1]["obj_fts"])
    assert not torch.equal(seen[0]["masked_lm_labels"], seen[1]["masked_lm_labels"])
    assert torch.equal(seen[0]["txt_masks"], seen[1]["txt_masks"]) and torch.equal(seen[0]["obj_masks"], seen[1]["obj_masks"])
    # the wrapper without masking: ScanFamilyDatasetWrapperOld's dict
    plain = pretrain_batch(packed, texts, items, ids, M, seed=seed, mask=False, **kw)
    assert "masked_lm_labels" not in plain and torch.equal(plain["obj_sem_masks"], plain["obj_masks"])
    val = pretrain_batch(packed, texts, items, ids, M, seed=seed, split="val", **kw)
    assert "aug_entries" not in val and val["obj_fts"].shape == (B, O, P, 6)
