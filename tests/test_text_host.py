"""The resident text path on the host: the numpy restatement of tests/text_cases.py against the reference's own outputs
(tests/golden/text_ref.npz, written by tests/golden/make_golden_text.py) -- exact; `PackedTexts` table building on the
CPU; the argument checks of gps_text_batch, which come before any launch; and the statistics of the device draw law on
its numpy emulation.  No GPU."""
import math
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import text_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_text as T  # noqa: E402

GOLD = np.load(os.path.join(HERE, "golden", "text_ref.npz"))
SHAPE_IDS = [C.shape_key(L, Ls) for L, Ls in C.SHAPES]


def test_entry_is_declared_bound_and_built():
    lib = _native.load()
    assert "gps_text_batch" in _native.declared_symbols() and "gps_text_batch" in _native.SIGNATURES
    assert hasattr(lib, "gps_text_batch") and lib.gps_abi_version() == 11       # additive: the ABI number does not move
    from sceneverse_amd.csrc import build
    assert ("gps_text.hip", []) in build.SOURCES
    text = open(_native.HEADER_PATH).read()
    for cite in ("dataset_wrapper.py:38-111", "data_utils.py:50-60", "data_utils.py:76-104", "data_utils.py:107-121"):
        assert cite in text, cite


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_fixture_inputs_are_the_builders(shape):
    L, Ls = shape
    for name, v in C.build_inputs(L, Ls).items():
        assert np.array_equal(GOLD[f"{C.shape_key(L, Ls)}/{name}"], v), name


@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_gather_restatement_equals_the_reference(shape):
    L, Ls = shape
    key = C.shape_key(L, Ls)
    g = {k: GOLD[f"{key}/{k}"] for k in ("tok", "off", "sent_idx", "cap_idx")}
    ids, masks, s_ids, s_masks = C.gather(g["tok"], g["off"], g["sent_idx"], g["cap_idx"], L, Ls)
    assert np.array_equal(ids, GOLD[f"{key}/txt_ids"]) and np.array_equal(masks, GOLD[f"{key}/txt_masks"])
    assert np.array_equal(s_ids, GOLD[f"{key}/scene_ids_str"]) and np.array_equal(s_masks, GOLD[f"{key}/scene_masks_str"])
    if Ls > L:                                   # merge_tokens runs only there
        _, _, m_ids, m_masks = C.gather(g["tok"], g["off"], g["sent_idx"], g["cap_idx"], L, Ls, scene_sent_cap=L - 2)
        assert np.array_equal(m_ids, GOLD[f"{key}/scene_ids_merge"])
        assert np.array_equal(m_masks, GOLD[f"{key}/scene_masks_merge"])
        assert not np.array_equal(m_ids, s_ids)  # the 2 L sentence is cut differently by the two forms
    without = C.gather(g["tok"], g["off"], g["sent_idx"], None, L, Ls)
    assert without[2] is None and np.array_equal(without[0], ids)


def test_fixture_covers_the_cases_it_claims():
    L, Ls = 50, 300
    key = C.shape_key(L, Ls)
    off, sent, cap = GOLD[f"{key}/off"], GOLD[f"{key}/sent_idx"], GOLD[f"{key}/cap_idx"]
    ls, lc = (off[sent + 1] - off[sent]), (off[cap + 1] - off[cap])
    assert sorted(set(ls.tolist())) == [0, 1, L - 3, L - 2, L - 1, 2 * L]
    assert sorted(set(GOLD[f"{key}/txt_masks"].sum(1).tolist())) == [2, 3, L - 1, L]
    total = ls + lc
    assert (total == Ls - 2).any() and (total == Ls - 1).any() and (lc > Ls - 2).any() and (lc == 0).any()
    # a caption alone past Ls - 2: no sentence token in the scene text, [SEP] in the last slot
    r = int(np.flatnonzero((lc > Ls - 2) & (ls > 0))[0])
    tok = GOLD[f"{key}/tok"]
    assert np.array_equal(GOLD[f"{key}/scene_ids_str"][r, 1:Ls - 1], tok[off[cap[r]]:off[cap[r]] + Ls - 2])
    assert GOLD[f"{key}/scene_ids_str"][r, Ls - 1] == 102 and GOLD[f"{key}/scene_masks_str"][r].all()
    # [CLS] and [SEP] take part in the masking: at ratio 1 every valid position carries a label
    labels = GOLD[f"{C.ratio_key(L, Ls, 1.0)}/labels"]
    assert np.array_equal(labels != -1, GOLD[f"{key}/txt_masks"] == 1) and (labels[:, 0] == 101).all()
    assert (GOLD[f"{C.ratio_key(L, Ls, 0.0)}/labels"] == -1).all()
    m = GOLD[f"{key}/obj_masks"]
    assert not m[0].any() and m[1].all() and 0 < m[2].sum() < m.shape[1]
    sem = GOLD[f"{C.ratio_key(L, Ls, 0.15)}/obj_sem_masks"]
    assert not sem[0].any() and 0 < sem.sum() < m.sum() and not (sem & ~m).any()


@pytest.mark.parametrize("ratio", C.RATIOS, ids=[f"r{r:g}" for r in C.RATIOS])
@pytest.mark.parametrize("shape", C.SHAPES, ids=SHAPE_IDS)
def test_replay_restatement_equals_the_reference(shape, ratio):
    L, Ls = shape
    key, rk = C.shape_key(L, Ls), C.ratio_key(L, Ls, ratio)
    ids, labels = C.mask_replay(GOLD[f"{key}/txt_ids"], GOLD[f"{key}/txt_masks"], GOLD[f"{rk}/u_tok"],
                                GOLD[f"{rk}/rand_tok"], ratio)
    assert np.array_equal(ids, GOLD[f"{rk}/masked_ids"]) and np.array_equal(labels, GOLD[f"{rk}/labels"])
    sem = C.obj_replay(GOLD[f"{key}/obj_masks"], GOLD[f"{rk}/u_obj"], ratio)
    assert np.array_equal(sem, GOLD[f"{rk}/obj_sem_masks"])


def test_packed_texts_on_the_cpu():
    p = T.PackedTexts("cpu")
    assert p.n_texts == 0
    ids = [p.add_text(t) for t in ([5, 6, 7], [], np.array([9], dtype=np.int64), torch.tensor([1, 2]).tolist())]
    assert ids == [0, 1, 2, 3] and p.n_texts == 4
    with pytest.raises(ValueError):
        p.add_text([3, -1])
    with pytest.raises(ValueError):
        p.add_text([1 << 31])
    assert p.finalize() is p and p.n_texts == 4
    assert p.off.dtype == torch.int64 and p.off.tolist() == [0, 3, 3, 4, 6]
    assert p.tok.dtype == torch.int32 and p.tok.tolist() == [5, 6, 7, 9, 1, 2] and p.lens_host.tolist() == [3, 0, 1, 2]
    with pytest.raises(AssertionError):
        p.add_text([1])
    empty = T.PackedTexts("cpu").finalize()
    assert empty.n_texts == 0 and empty.off.tolist() == [0] and empty.tok.numel() == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        T.text_batch(p, [0, 1])
    with pytest.raises(RuntimeError, match="finalize"):
        T.text_batch(T.PackedTexts("cpu"), [0])


def test_synth_packed_texts_follows_the_length_laws():
    from sceneverse_amd.data.synthetic import synth_packed_texts
    p = synth_packed_texts(200, 50, seed=3, device="cpu")
    assert p.n_texts == 250
    ls, lc = p.lens_host[:200], p.lens_host[200:]
    assert ls.min() >= 4 and ls.max() <= 48 and lc.min() >= 28 and lc.max() <= 298 and lc.max() > 48
    assert int(p.tok.min()) >= 1000 and int(p.tok.max()) < C.VOCAB
    q = synth_packed_texts(200, 50, seed=3, device="cpu")
    assert torch.equal(p.tok, q.tok) and torch.equal(p.off, q.off)


def _call(lib, **kw):
    """gps_text_batch with a valid argument set (non-NULL stand-in addresses: nothing is launched when a check fails
    first) in which the named arguments are replaced."""
    a = dict(n_texts=4, n_tok=10, tok=16, off=16, n_rows=2, sent_idx=16, cap_idx=16, L=50, Ls=300, scene_sent_cap=48,
             cls_id=101, sep_id=102, mask_id=103, pad_id=0, vocab_size=30522, do_mask=1, txt_mask_ratio=0.15,
             pc_mask_ratio=0.1, n_obj_rows=2, O=80, obj_masks=16, u_tok=None, rand_tok=None, u_obj=None, seed=0,
             seed_dev=None, txt_ids=16, txt_masks=16, masked_lm_labels=16, scene_txt_ids=16, scene_txt_masks=16,
             obj_sem_masks=16, stream=None)
    assert set(kw) <= set(a), set(kw) - set(a)
    a.update(kw)
    return lib.gps_text_batch(*a.values())


def test_argument_checks_come_before_any_launch():
    lib = _native.load()
    OK, INVALID = _native.GPS_OK, _native.GPS_ERR_INVALID_ARGUMENT
    for bad in (dict(L=1), dict(Ls=1), dict(L=0), dict(n_rows=-1), dict(n_texts=-1), dict(n_tok=-1), dict(n_obj_rows=-1),
                dict(O=-1), dict(scene_sent_cap=-1), dict(txt_mask_ratio=-0.01), dict(txt_mask_ratio=1.01),
                dict(pc_mask_ratio=-1.0), dict(pc_mask_ratio=2.0), dict(txt_mask_ratio=float("nan")), dict(vocab_size=0),
                dict(tok=None), dict(off=None), dict(sent_idx=None), dict(txt_ids=None), dict(txt_masks=None),
                dict(masked_lm_labels=None), dict(obj_masks=None), dict(obj_sem_masks=None),
                dict(scene_txt_ids=None), dict(scene_txt_masks=None), dict(cap_idx=None),
                dict(u_tok=16), dict(rand_tok=16), dict(u_obj=16), dict(u_tok=16, rand_tok=16),
                dict(u_tok=16, u_obj=16), dict(rand_tok=16, u_obj=16)):
        assert _call(lib, **bad) == INVALID, bad
    # empty work is fine whatever the pointers are, but its scalars are still checked
    none = dict(tok=None, off=None, sent_idx=None, cap_idx=None, obj_masks=None, txt_ids=None, txt_masks=None,
                masked_lm_labels=None, scene_txt_ids=None, scene_txt_masks=None, obj_sem_masks=None)
    assert _call(lib, n_rows=0, n_obj_rows=0, **none) == OK
    assert _call(lib, n_rows=0, n_obj_rows=0, O=0, n_texts=0, n_tok=0, **none) == OK
    assert _call(lib, n_rows=0, n_obj_rows=0, L=1, **none) == INVALID
    assert _call(lib, n_rows=0, n_obj_rows=0, txt_mask_ratio=1.5, **none) == INVALID
    assert _call(lib, L=(1 << 20) + 1) == _native.GPS_ERR_UNSUPPORTED


# ---- the device law on its emulation ----------------------------------------------------------------------------------
N_TOK = 65536
SEEDS = (0, 20240521, (7 << 32) + 5)


def _within(share, p, n, sigmas=5.0):
    """`share` of n Bernoulli(p) draws lies within `sigmas` binomial standard deviations of p.  Derived, not tuned: a
    fair stream leaves this band with probability 5.7e-7 per check."""
    return abs(share - p) <= sigmas * math.sqrt(p * (1.0 - p) / n)


@pytest.mark.parametrize("seed", SEEDS)
def test_device_law_statistics(seed):
    ratio, pc_ratio = 0.15, 0.1
    masked, to_mask, to_rand, rand_id = C.token_decisions(seed, N_TOK, ratio)
    n_masked = int(masked.sum())
    assert _within(n_masked / N_TOK, ratio, N_TOK)
    kept = masked & ~to_mask & ~to_rand
    assert not (to_mask & to_rand).any() and int(to_mask.sum() + to_rand.sum() + kept.sum()) == n_masked
    assert _within(to_mask.sum() / n_masked, 0.8, n_masked)
    assert _within(to_rand.sum() / n_masked, 0.1, n_masked)
    assert _within(kept.sum() / n_masked, 0.1, n_masked)
    assert rand_id.min() >= 0 and rand_id.max() < C.VOCAB
    assert rand_id.max() > C.VOCAB * 0.99 and rand_id.min() < C.VOCAB * 0.01      # and they span the vocabulary
    dropped = C.obj_dropped(seed, N_TOK, pc_ratio)
    assert _within(dropped.mean(), pc_ratio, N_TOK)
    # the token and the object stream are different streams: equal indices do not share their decision
    both = C.obj_dropped(seed, N_TOK, ratio)                 # the object stream at the TOKEN ratio
    assert not np.array_equal(both, masked)
    assert _within((both & masked).mean(), ratio * ratio, N_TOK)                   # independent, not merely different


def test_device_law_edges():
    for seed in SEEDS:
        masked, to_mask, to_rand, _ = C.token_decisions(seed, 4096, 1.0)            # T = 2^32: every position
        assert masked.all() and _within(to_mask.mean(), 0.8, 4096)
        masked, _, _, _ = C.token_decisions(seed, 4096, 0.0)
        assert not masked.any()
        assert C.obj_dropped(seed, 4096, 1.0).all() and not C.obj_dropped(seed, 4096, 0.0).any()
    assert C.threshold(1.0) == 1 << 32 and C.threshold(0.0) == 0 and C.threshold(0.5) == 1 << 31
    # an index past 2^32 folds its high word in; the seed's high word matters
    a = C.rng_u32(1, np.array([5, 5 + (1 << 32)], dtype=np.uint64))
    assert a[0] != a[1]
    assert C.rng_u32(1, np.arange(8))[3] != C.rng_u32(1 + (1 << 32), np.arange(8))[3]
    # the wrap of S + 1 / S + 2 at 2^64
    assert np.array_equal(C.obj_dropped((1 << 64) - 2, 64, 0.5), C.rng_u32(0, np.arange(64)) < np.uint64(1 << 31))
