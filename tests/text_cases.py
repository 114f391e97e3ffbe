"""Shared by tests/golden/make_golden_text.py, tests/test_text_host.py and tests/test_gpu_text.py: the cases of the
resident text path (sceneverse_amd/data/gpu_text.py, csrc/gps_text.hip) and a numpy restatement of its rules, written
from the statement in include/gps_hip.h:

  * gather        [cls] s[:n] [sep] pad, and the scene text [cls] (c ++ s')[:Ls - 2] [sep] pad;
  * replay law    random_word / random_point_cloud on recorded draws, in double arithmetic;
  * device law    integers only, on the numpy `mix32` / `seed_fold` of tests/test_dropout_hash.py.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from test_dropout_hash import M32, mix32, seed_fold  # noqa: E402

SPECIAL = (101, 102, 103, 0)                     # [CLS], [SEP], [MASK], [PAD]
VOCAB = 30522
NO_CAP = (1 << 31) - 1
M64 = (1 << 64) - 1

SHAPES = ((2, 2), (5, 8), (50, 300))             # (L, Ls)
RATIOS = (0.0, 0.15, 0.9, 1.0)
CAP_KINDS = ("fit", "over1", "fit_t", "over1_t", "long", "empty")


def shape_key(L, Ls):
    return f"L{L}_Ls{Ls}"


def ratio_key(L, Ls, ratio):
    return f"{shape_key(L, Ls)}/r{ratio:g}"


def sentence_lengths(L):
    """Token counts against L: 0, 1, L - 3, L - 2 (fills the row), L - 1 (one cut), 2 L."""
    return [max(x, 0) for x in (0, 1, L - 3, L - 2, L - 1, 2 * L)]


def caption_length(kind, ls, L, Ls):
    """The caption that puts caption + sentence at: exactly Ls - 2 tokens (the last sentence token is the last body
    token), Ls - 1 (one cut); the same two counted with the sentence already truncated to L - 2 (the pre-tokenised
    form); a caption alone longer than Ls - 2 (the sentence entirely cut); no caption at all."""
    lt = min(ls, L - 2)
    return {"fit": max(Ls - 2 - ls, 0), "over1": max(Ls - 1 - ls, 0), "fit_t": max(Ls - 2 - lt, 0),
            "over1_t": max(Ls - 1 - lt, 0), "long": Ls + 3, "empty": 0}[kind]


def obj_slots(L):
    return 80 if L == 50 else 5


def build_inputs(L, Ls, seed=0):
    """One batch per (L, Ls): a row per (sentence length, caption kind), each with texts of its own; the object rows are
    an empty one, a full one and a prefix.  -> dict of arrays (what the golden stores as the case's inputs)."""
    rng = np.random.default_rng(1000 * L + Ls + seed)
    toks, sent_idx, cap_idx = [], [], []
    for ls in sentence_lengths(L):
        for kind in CAP_KINDS:
            sent_idx.append(len(toks))
            toks.append(rng.integers(1000, VOCAB, size=ls))
            cap_idx.append(len(toks))
            toks.append(rng.integers(1000, VOCAB, size=caption_length(kind, ls, L, Ls)))
    lens = np.asarray([len(t) for t in toks], dtype=np.int64)
    off = np.zeros(len(toks) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    O = obj_slots(L)
    obj_masks = np.zeros((3, O), dtype=bool)
    obj_masks[1] = True
    obj_masks[2, :O // 2 + 1] = True
    return {"tok": np.concatenate(toks).astype(np.int32), "off": off, "sent_idx": np.asarray(sent_idx, np.int32),
            "cap_idx": np.asarray(cap_idx, np.int32), "obj_masks": obj_masks}


def text_of(tok, off, i):
    if i < 0 or i >= len(off) - 1:
        return np.zeros(0, np.int64)
    return np.asarray(tok[off[i]:off[i + 1]], dtype=np.int64)


# ---- the rules ------------------------------------------------------------------------------------------------------
def framed(body, max_len, special=SPECIAL):
    """[cls] body[:max_len - 2] [sep], padded to max_len -> (ids, masks) int64."""
    cls_id, sep_id, _, pad_id = special
    body = np.asarray(body, dtype=np.int64)[:max_len - 2]
    ids = np.full(max_len, pad_id, dtype=np.int64)
    ids[0] = cls_id
    ids[1:1 + len(body)] = body
    ids[1 + len(body)] = sep_id
    masks = (np.arange(max_len) < len(body) + 2).astype(np.int64)
    return ids, masks


def gather(tok, off, sent_idx, cap_idx, L, Ls, scene_sent_cap=NO_CAP, special=SPECIAL):
    """-> txt_ids, txt_masks (shape + (L,)), scene_txt_ids, scene_txt_masks (shape + (Ls,)) or None, None."""
    sent_idx = np.asarray(sent_idx)
    shape = sent_idx.shape
    flat = sent_idx.reshape(-1)
    txt = [framed(text_of(tok, off, int(i)), L, special) for i in flat]
    ids = np.stack([t[0] for t in txt], 0).reshape(shape + (L,)) if len(txt) else np.zeros(shape + (L,), np.int64)
    masks = np.stack([t[1] for t in txt], 0).reshape(shape + (L,)) if len(txt) else np.zeros(shape + (L,), np.int64)
    if cap_idx is None:
        return ids, masks, None, None
    caps = np.asarray(cap_idx).reshape(-1)
    sc = []
    for i, c in zip(flat, caps):
        s = text_of(tok, off, int(i))
        sc.append(framed(np.concatenate([text_of(tok, off, int(c)), s[:min(len(s), scene_sent_cap)]]), Ls, special))
    return (ids, masks, np.stack([t[0] for t in sc], 0).reshape(shape + (Ls,)),
            np.stack([t[1] for t in sc], 0).reshape(shape + (Ls,)))


def mask_replay(txt_ids, txt_masks, u_tok, rand_tok, ratio, special=SPECIAL):
    """random_word on recorded draws -> (masked ids, labels)."""
    ids, labels = txt_ids.copy(), np.full(txt_ids.shape, -1, dtype=np.int64)
    u = np.asarray(u_tok, dtype=np.float64)
    hit = (txt_masks == 1) & (u < ratio)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = u / np.float64(ratio)
    labels[hit] = txt_ids[hit]
    to_mask = hit & (q < 0.8)
    to_rand = hit & ~(q < 0.8) & (q < 0.9)
    ids[to_mask] = special[2]
    ids[to_rand] = np.asarray(rand_tok, dtype=np.int64)[to_rand]
    return ids, labels


def obj_replay(obj_masks, u_obj, ratio):
    return np.asarray(obj_masks, dtype=bool) & ~(np.asarray(u_obj, dtype=np.float64) < ratio)


def rng_u32(seed, idx):
    """gps_dropout::rng_u32 -> uint64 array holding 32-bit values."""
    idx = np.asarray(idx, dtype=np.uint64)
    folded = ((idx & M32) + ((idx >> np.uint64(32)) * np.uint64(0x85EBCA6B) & M32)) & M32
    return mix32(folded ^ seed_fold(int(seed) & M64))


def threshold(ratio):
    """T(x) = floor(x * 2^32): 2^32 at x = 1."""
    return int(float(ratio) * 4294967296.0)


def token_decisions(seed, n, ratio):
    """The device law's decision of flat token index 0 .. n - 1 -> (masked, to [MASK], to random, random id)."""
    idx = np.arange(n, dtype=np.uint64)
    u = rng_u32(seed, idx)
    T = np.uint64(threshold(ratio))
    masked = u < T
    ten_u = np.uint64(10) * u
    to_mask = masked & (ten_u < np.uint64(8) * T)
    to_rand = masked & ~to_mask & (ten_u < np.uint64(9) * T)
    rand_id = ((rng_u32((int(seed) + 1) & M64, idx) * np.uint64(VOCAB)) >> np.uint64(32)).astype(np.int64)
    return masked, to_mask, to_rand, rand_id


def mask_device(txt_ids, txt_masks, seed, ratio, special=SPECIAL, vocab=VOCAB):
    """The integer law over rows of length L = txt_ids.shape[-1] -> (masked ids, labels)."""
    assert vocab == VOCAB
    shape = txt_ids.shape
    masked, to_mask, to_rand, rand_id = (a.reshape(shape) for a in token_decisions(seed, txt_ids.size, ratio))
    valid = txt_masks == 1
    ids, labels = txt_ids.copy(), np.full(shape, -1, dtype=np.int64)
    labels[valid & masked] = txt_ids[valid & masked]
    ids[valid & to_mask] = special[2]
    ids[valid & to_rand] = rand_id[valid & to_rand]
    return ids, labels


def obj_dropped(seed, n, ratio):
    return rng_u32((int(seed) + 2) & M64, np.arange(n, dtype=np.uint64)) < np.uint64(threshold(ratio))


def obj_device(obj_masks, seed, ratio):
    obj_masks = np.asarray(obj_masks, dtype=bool)
    return obj_masks & ~obj_dropped(seed, obj_masks.size, ratio).reshape(obj_masks.shape)
