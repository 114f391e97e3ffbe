"""The resident text path on the GPU (csrc/gps_text.hip through sceneverse_amd/data/gpu_text.py): replays of the
reference's draws against the reference's own outputs (tests/golden/text_ref.npz), the device draw law against its
numpy emulation (tests/text_cases.py), the gather-only form, in-place outputs and one graph capture.  Every comparison
is exact equality."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import text_cases as C  # noqa: E402
from sceneverse_amd.data import gpu_text as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "text_ref.npz"))
SHAPE_IDS = [C.shape_key(L, Ls) for L, Ls in C.SHAPES]
_CACHE = {}


def _pack(tok, off):
    p = T.PackedTexts(DEV)
    for i in range(len(off) - 1):
        p.add_text(C.text_of(tok, off, i))
    return p.finalize()


def _golden_texts(L, Ls):
    key = C.shape_key(L, Ls)
    if key not in _CACHE:
        _CACHE[key] = _pack(GOLD[f"{key}/tok"], GOLD[f"{key}/off"])
    return _CACHE[key]


def _synth():
    """64 sentences + 16 captions with the synthetic batch's length laws, and their host copy for the emulation."""
    if "synth" not in _CACHE:
        from sceneverse_amd.data.synthetic import synth_packed_texts
        p = synth_packed_texts(64, 16, seed=11, device=DEV)
        _CACHE["synth"] = (p, p.tok.cpu().numpy(), p.off.cpu().numpy())
    return _CACHE["synth"]


def _obj_masks(n_rows, O, seed=2):
    n_real = np.random.default_rng(seed).integers(0, O + 1, size=n_rows)
    n_real[0], n_real[-1] = 0, O                             # an empty row and a full one
    return np.arange(O)[None, :] < n_real[:, None]


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.mark.parametrize("ratio", C.RATIOS, ids=[f"r{r:g}" for r in C.RATIOS])
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_replay_equals_the_reference(shape, ratio):
    L, Ls = shape
    key, rk = C.shape_key(L, Ls), C.ratio_key(L, Ls, ratio)
    texts = _golden_texts(L, Ls)
    draws = T.TextDraws(torch.from_numpy(GOLD[f"{rk}/u_tok"]), torch.from_numpy(GOLD[f"{rk}/rand_tok"]),
                        torch.from_numpy(GOLD[f"{rk}/u_obj"]))
    obj_masks = torch.from_numpy(GOLD[f"{key}/obj_masks"]).to(DEV)
    res = T.text_batch(texts, GOLD[f"{key}/sent_idx"], GOLD[f"{key}/cap_idx"], max_seq_len=L, max_scene_cap_len=Ls,
                       txt_mask_ratio=ratio, pc_mask_ratio=ratio, obj_masks=obj_masks, draws=draws)
    assert all(res[k].dtype == torch.int64 for k in res if k != "obj_sem_masks") and res["obj_sem_masks"].dtype == torch.bool
    got = _np(res)
    assert np.array_equal(got["txt_ids"], GOLD[f"{rk}/masked_ids"])
    assert np.array_equal(got["masked_lm_labels"], GOLD[f"{rk}/labels"])
    assert np.array_equal(got["txt_masks"], GOLD[f"{key}/txt_masks"])
    assert np.array_equal(got["scene_txt_ids"], GOLD[f"{key}/scene_ids_str"])            # the scene text is never masked
    assert np.array_equal(got["scene_txt_masks"], GOLD[f"{key}/scene_masks_str"])
    assert np.array_equal(got["obj_sem_masks"], GOLD[f"{rk}/obj_sem_masks"])
    if Ls > L:                                               # merge_tokens: the sentence enters already truncated
        got = _np(T.text_batch(texts, GOLD[f"{key}/sent_idx"], GOLD[f"{key}/cap_idx"], max_seq_len=L,
                               max_scene_cap_len=Ls, scene_sent_cap=L - 2, mask=False))
        assert np.array_equal(got["scene_txt_ids"], GOLD[f"{key}/scene_ids_merge"])
        assert np.array_equal(got["scene_txt_masks"], GOLD[f"{key}/scene_masks_merge"])


def _device_case(name):
    """-> texts, host tok / off, sent_idx, cap_idx, L, Ls, obj_masks (host bool)."""
    if name == "1x2":
        g = {k: GOLD[f"L2_Ls2/{k}"] for k in ("tok", "off", "sent_idx", "cap_idx")}
        return _golden_texts(2, 2), g["tok"], g["off"], g["sent_idx"][[30]], g["cap_idx"][[30]], 2, 2, _obj_masks(1, 3)
    if name == "3x5":
        g = {k: GOLD[f"L5_Ls8/{k}"] for k in ("tok", "off", "sent_idx", "cap_idx")}
        rows = [18, 31, 10]                                  # sentence of L - 2, 2 L and 1 tokens
        return _golden_texts(5, 8), g["tok"], g["off"], g["sent_idx"][rows], g["cap_idx"][rows], 5, 8, _obj_masks(3, 5)
    texts, tok, off = _synth()
    if name == "64x50":
        return texts, tok, off, np.arange(64, dtype=np.int32), (64 + np.arange(64) % 16).astype(np.int32), 50, 300, _obj_masks(64, 80)
    assert name == "7x3"                                     # a per-scene batch: 7 scenes x 3 sentences, 7 object rows
    sent = np.random.default_rng(4).permutation(64)[:21].reshape(7, 3).astype(np.int32)
    cap = np.repeat(64 + np.arange(7, dtype=np.int32), 3).reshape(7, 3)
    return texts, tok, off, sent, cap, 50, 300, _obj_masks(7, 80)


def _emulate(tok, off, sent, cap, L, Ls, obj_masks, seed, txt_ratio, pc_ratio):
    ids, masks, s_ids, s_masks = C.gather(tok, off, sent, cap, L, Ls)
    m_ids, labels = C.mask_device(ids, masks, seed, txt_ratio)
    return {"txt_ids": m_ids, "txt_masks": masks, "masked_lm_labels": labels, "scene_txt_ids": s_ids,
            "scene_txt_masks": s_masks, "obj_sem_masks": C.obj_device(obj_masks, seed, pc_ratio)}


@pytest.mark.parametrize("name", ["1x2", "3x5", "64x50", "7x3"])
def test_device_law_equals_the_emulation(name):
    texts, tok, off, sent, cap, L, Ls, obj_masks = _device_case(name)
    seed = (3 << 32) + 12345
    for txt_ratio, pc_ratio in ((0.15, 0.1), (1.0, 0.9)):
        res = T.text_batch(texts, sent, cap, max_seq_len=L, max_scene_cap_len=Ls, txt_mask_ratio=txt_ratio,
                           pc_mask_ratio=pc_ratio, obj_masks=torch.from_numpy(obj_masks).to(DEV), seed=seed)
        want = _emulate(tok, off, sent, cap, L, Ls, obj_masks, seed, txt_ratio, pc_ratio)
        assert set(res) == set(want)
        for k, v in _np(res).items():
            assert v.shape == want[k].shape and np.array_equal(v, want[k]), (name, txt_ratio, k)
    if name == "64x50":                                      # the case is not vacuous: all three outcomes occur
        want = _emulate(tok, off, sent, cap, L, Ls, obj_masks, seed, 0.15, 0.1)
        hit = want["masked_lm_labels"] != -1
        changed = want["txt_ids"][hit] != want["masked_lm_labels"][hit]
        assert (want["txt_ids"][hit] == 103).sum() > 100 and (~changed).sum() > 5
        assert (changed & (want["txt_ids"][hit] != 103)).sum() > 5
        assert 0 < (obj_masks & ~want["obj_sem_masks"]).sum() < obj_masks.sum()


def test_gather_only():
    texts, tok, off, sent, cap, L, Ls, obj_masks = _device_case("7x3")
    om = torch.from_numpy(obj_masks).to(DEV)
    res = T.text_batch(texts, sent, cap, max_seq_len=L, max_scene_cap_len=Ls, mask=False, obj_masks=om)
    ids, masks, s_ids, s_masks = C.gather(tok, off, sent, cap, L, Ls)
    assert set(res) == {"txt_ids", "txt_masks", "scene_txt_ids", "scene_txt_masks", "obj_sem_masks"}
    got = _np(res)
    assert np.array_equal(got["txt_ids"], ids) and np.array_equal(got["txt_masks"], masks)
    assert np.array_equal(got["scene_txt_ids"], s_ids) and np.array_equal(got["scene_txt_masks"], s_masks)
    assert torch.equal(res["obj_sem_masks"], om)
    # without captions or objects, labels on request: all -1
    out = {"txt_ids": torch.empty((7, 3, L), dtype=torch.int64, device=DEV),
           "txt_masks": torch.empty((7, 3, L), dtype=torch.int64, device=DEV),
           "masked_lm_labels": torch.zeros((7, 3, L), dtype=torch.int64, device=DEV)}
    res = T.text_batch(texts, torch.from_numpy(sent).to(DEV), max_seq_len=L, mask=False, out=out)
    assert set(res) == set(out) and np.array_equal(res["txt_ids"].cpu().numpy(), ids)
    assert bool((out["masked_lm_labels"] == -1).all())
    # a text id out of range: refused on the host, an empty text on the device
    with pytest.raises(ValueError):
        T.text_batch(texts, [0, texts.n_texts], max_seq_len=L, mask=False)
    with pytest.raises(ValueError):
        T.text_batch(texts, [0, 1], [-1, 64], max_seq_len=L, mask=False)
    res = T.text_batch(texts, torch.tensor([texts.n_texts, -1, 0], device=DEV), torch.tensor([64, 10 ** 6, -5], device=DEV),
                       max_seq_len=L, max_scene_cap_len=Ls, mask=False)
    want = C.gather(tok, off, [-1, -1, 0], [64, -1, -1], L, Ls)
    assert np.array_equal(res["txt_ids"].cpu().numpy(), want[0]) and np.array_equal(res["scene_txt_ids"].cpu().numpy(), want[2])
    assert res["txt_masks"][:2].sum(1).tolist() == [2, 2] and np.array_equal(res["scene_txt_masks"].cpu().numpy(), want[3])
    empty = T.text_batch(texts, np.zeros((0,), np.int32), np.zeros((0,), np.int32), max_seq_len=L, max_scene_cap_len=Ls)
    assert empty["txt_ids"].shape == (0, L) and empty["scene_txt_ids"].shape == (0, Ls)


def test_out_is_written_in_place():
    texts, tok, off, sent, cap, L, Ls, obj_masks = _device_case("64x50")
    om = torch.from_numpy(obj_masks).to(DEV)
    kw = dict(max_seq_len=L, max_scene_cap_len=Ls, obj_masks=om, seed=99)
    ref = T.text_batch(texts, sent, cap, **kw)
    SENT = -7
    out = {k: torch.full(tuple(v.shape), SENT, dtype=torch.int64, device=DEV) for k, v in ref.items() if k != "obj_sem_masks"}
    out["obj_sem_masks"] = torch.full(tuple(om.shape), 7, dtype=torch.uint8, device=DEV)
    ptrs = {k: v.data_ptr() for k, v in out.items()}
    res = T.text_batch(texts, sent, cap, out=out, **kw)
    for k in out:
        assert out[k].data_ptr() == ptrs[k]
        if k != "obj_sem_masks":
            assert res[k].data_ptr() == ptrs[k], k
        assert torch.equal(out[k].to(ref[k].dtype), ref[k]), k
        assert not bool((out[k] == (7 if k == "obj_sem_masks" else SENT)).any()), k     # no element left untouched
    # a bool buffer is returned as it is
    out["obj_sem_masks"] = torch.ones(tuple(om.shape), dtype=torch.bool, device=DEV)
    res = T.text_batch(texts, sent, cap, out=out, **kw)
    assert res["obj_sem_masks"].data_ptr() == out["obj_sem_masks"].data_ptr() and torch.equal(res["obj_sem_masks"], ref["obj_sem_masks"])
    with pytest.raises(ValueError):
        T.text_batch(texts, sent, cap, out=dict(out, txt_ids=out["txt_ids"].int()), **kw)
    with pytest.raises(ValueError):
        T.text_batch(texts, sent, cap, out={k: v for k, v in out.items() if k != "scene_txt_masks"}, **kw)
    with pytest.raises(ValueError):
        T.text_batch(texts, sent, cap, out=dict(out, txt_masks=out["txt_masks"][:32]), **kw)


def test_one_capture_fresh_draws_per_replay():
    """A single chain: advance the seed word on the device, then the launch.  Three replays, three different batches,
    each the emulation's at the advanced seed."""
    texts, tok, off, sent, cap, L, Ls, obj_masks = _device_case("64x50")
    om = torch.from_numpy(obj_masks).to(DEV)
    sent_d, cap_d = torch.from_numpy(sent).to(DEV), torch.from_numpy(cap).to(DEV)
    seed, start = 1000, 41
    seed_dev = torch.full((1,), start, dtype=torch.int64, device=DEV)
    kw = dict(max_seq_len=L, max_scene_cap_len=Ls, obj_masks=om, seed=seed, seed_dev=seed_dev)
    out = T.text_batch(texts, sent_d, cap_d, **kw)           # the buffers, and the library loaded ahead of the capture
    want = _emulate(tok, off, sent, cap, L, Ls, obj_masks, seed + start, 0.15, 0.1)
    assert all(np.array_equal(v, want[k]) for k, v in _np(out).items())
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seed_dev.add_(1)
        T.text_batch(texts, sent_d, cap_d, out=out, **kw)
    seen = []
    for k in range(1, 4):
        graph.replay()
        got = _np(out)
        want = _emulate(tok, off, sent, cap, L, Ls, obj_masks, seed + start + k, 0.15, 0.1)
        for name, v in got.items():
            assert np.array_equal(v, want[name]), (k, name)
        seen.append(got)
    assert int(seed_dev.item()) == start + 3
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert not np.array_equal(seen[a]["txt_ids"], seen[b]["txt_ids"])
        assert not np.array_equal(seen[a]["masked_lm_labels"], seen[b]["masked_lm_labels"])
        assert not np.array_equal(seen[a]["obj_sem_masks"], seen[b]["obj_sem_masks"])
