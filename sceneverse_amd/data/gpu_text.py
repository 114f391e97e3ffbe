"""HBM-resident token tables + the loader's per-sample text work as ONE launch of libgps_hip.so.

Reference (what this replaces on the data-loader workers, per sample):
    MaskDatasetWrapper.__getitem__  data/datasets/dataset_wrapper.py:38-111  tokenizer(sentence), tokenizer(scene_cap + " " +
                                                                             sentence), random_word, random_point_cloud
    merge_tokens                    data/data_utils.py:50-60                 caption + sentence, pre-tokenised
    random_word                     data/data_utils.py:76-104                a Python loop with `.item()` per token
    random_point_cloud              data/data_utils.py:107-121               a Python loop per object slot

MI355X form: the corpus (sentences and scene captions) is tokenised ONCE with whatever tokenizer the caller has, WITHOUT
special tokens, and uploaded as one int32 array with a CSR offset table (`PackedTexts`, the text twin of
`gpu_objects.PackedScans`).  A batch is then two integers per row -- the sentence's text id and the caption's -- and
`text_batch` turns them into `txt_ids / txt_masks / masked_lm_labels / scene_txt_ids / scene_txt_masks / obj_sem_masks`
on the device: gather, [CLS] / [SEP] / padding, the caption ++ sentence merge and the masking draws, which are new
every epoch and so cannot be cached.  GPU only: there is no CPU path here (the reference's own loader IS the CPU path;
tests/text_cases.py restates the rules for the tests).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from .._launch import launch
from ._resident import as_bool, need_finalized, need_gpu, outputs, seed_word, u64

BERT_SPECIAL = (101, 102, 103, 0)                # [CLS], [SEP], [MASK], [PAD]
BERT_VOCAB = 30522
_NO_CAP = (1 << 31) - 1                          # scene_sent_cap of the wrapper's string form: the whole sentence


class PackedTexts:
    """Token ids of a corpus resident on one device.  Build with add_text(...) x n, then finalize()."""

    def __init__(self, device: torch.device | str = "cuda"):
        self.device = torch.device(device)
        self._tokens: List[np.ndarray] = []
        self.tok = self.off = None
        self.lens_host: Optional[np.ndarray] = None

    def add_text(self, tokens: Sequence[int]) -> int:
        """tokens: the ids of one text WITHOUT special tokens (`tokenizer(text, add_special_tokens=False)`), any length,
        empty included.  -> the text's id, the number a batch refers to it by."""
        assert self.tok is None, "finalize() was already called"
        t = np.asarray(tokens, dtype=np.int64).reshape(-1)
        if t.size and (t.min() < 0 or t.max() > np.iinfo(np.int32).max):
            raise ValueError("add_text: token ids must fit int32 and be non-negative")
        self._tokens.append(t.astype(np.int32))
        return len(self._tokens) - 1

    def finalize(self) -> "PackedTexts":
        lens = np.asarray([t.size for t in self._tokens], dtype=np.int64)
        off = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        tok = np.concatenate(self._tokens) if self._tokens else np.zeros(0, np.int32)
        self.lens_host = lens
        self.tok = torch.from_numpy(tok.astype(np.int32, copy=False)).to(self.device)
        self.off = torch.from_numpy(off).to(self.device)
        self._tokens = []
        return self

    @property
    def n_texts(self) -> int:
        return len(self._tokens) if self.lens_host is None else int(self.lens_host.shape[0])


@dataclass
class TextDraws:
    """The reference loader's draws of one batch, for bit-compatible replays: u_tok (..., L) float64 = `random.random()`
    of random_word at each position (unread where txt_masks == 0), rand_tok (..., L) int32 = the id `random.choice`
    picked there (unread elsewhere), u_obj (n_obj_rows..., O) float64 = random_point_cloud's draws (None without
    object slots)."""
    u_tok: torch.Tensor
    rand_tok: torch.Tensor
    u_obj: Optional[torch.Tensor] = None


def _index(name: str, idx, n_texts: int, dev) -> torch.Tensor:
    """An index array of the batch -> int32 on the device; one that arrives on the host is range-checked there."""
    t = idx if torch.is_tensor(idx) else torch.as_tensor(np.asarray(idx))
    if t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"text_batch: {name} must hold integer text ids")
    if t.device.type == "cpu" and t.numel() and (int(t.min()) < 0 or int(t.max()) >= n_texts):
        raise ValueError(f"text_batch: {name} holds a text id outside [0, {n_texts})")
    return t.to(device=dev, dtype=torch.int32).contiguous()


def text_batch(texts: PackedTexts, sent_idx, cap_idx=None, *, max_seq_len: int = 50, max_scene_cap_len: int = 300,
               scene_sent_cap: Optional[int] = None, mask: bool = True, txt_mask_ratio: float = 0.15,
               pc_mask_ratio: float = 0.1, obj_masks: Optional[torch.Tensor] = None, draws: Optional[TextDraws] = None,
               seed: int = 0, seed_dev: Optional[torch.Tensor] = None, special=BERT_SPECIAL, vocab_size: int = BERT_VOCAB,
               out: Optional[dict] = None) -> dict:
    """The text tensors of one batch, in one launch and without a host sync.

    sent_idx: text ids of the rows' sentences, any shape `S` (a per-scene batch is (B, n_sentences)); cap_idx: the
    scene captions' text ids in the same shape, or None = no scene text.  -> dict with txt_ids, txt_masks (S + (L,))
    int64 [, masked_lm_labels likewise, when mask] [, scene_txt_ids, scene_txt_masks (S + (Ls,)) int64, with cap_idx]
    [, obj_sem_masks, bool in the shape of obj_masks, with obj_masks].

    scene_sent_cap: how many sentence tokens may enter the scene text; None = all of them, the string form of
    MaskDatasetWrapper (dataset_wrapper.py:49-54); max_seq_len - 2 = merge_tokens over the truncated sentence.
    mask=False: gather only (ScanFamilyDatasetWrapperOld): no draw, obj_sem_masks = obj_masks.
    obj_masks (..., O) bool / uint8 on the texts' GPU: which object slots hold an object (`obj_processing_post`'s).
    draws: a TextDraws for a replay of the reference's draws; None = drawn on the device from seed + *seed_dev by the
    integer law of include/gps_hip.h (seed_dev: one int64 word on the device, advanced there between graph replays).
    special = ([CLS], [SEP], [MASK], [PAD]) ids.
    out: optional dict of preallocated contiguous tensors under the names above (int64; obj_sem_masks bool or uint8),
    written IN PLACE -- the static input buffers of a captured training step (`GPSTrainStep.static_inputs()`), exactly as
    `obj_processing_post(out=)`.  Text ids that arrive on the host are range-checked there (ValueError); on the device,
    an id out of range reads as an empty text."""
    need_finalized(texts.tok, "PackedTexts")
    dev = texts.tok.device
    need_gpu(dev, "text_batch", "texts")
    L, Ls = int(max_seq_len), int(max_scene_cap_len)
    sent = _index("sent_idx", sent_idx, texts.n_texts, dev)
    shape = tuple(sent.shape)
    n_rows = sent.numel()
    cap = None
    if cap_idx is not None:
        cap = _index("cap_idx", cap_idx, texts.n_texts, dev)
        if tuple(cap.shape) != shape:
            raise ValueError(f"text_batch: cap_idx has shape {tuple(cap.shape)}, sent_idx {shape}")
    n_obj_rows = O = 0
    if obj_masks is not None:
        if obj_masks.device != dev or obj_masks.dim() < 1:
            raise ValueError("text_batch: obj_masks must be a (..., O) tensor on the texts' GPU")
        if obj_masks.dtype not in (torch.bool, torch.uint8):
            obj_masks = obj_masks != 0
        obj_masks = obj_masks.contiguous()
        O = int(obj_masks.shape[-1])
        n_obj_rows = obj_masks.numel() // O if O else 0
    u_tok = rand_tok = u_obj = None
    if draws is not None and mask:
        u_tok = draws.u_tok.to(device=dev, dtype=torch.float64).contiguous()
        rand_tok = draws.rand_tok.to(device=dev, dtype=torch.int32).contiguous()
        if tuple(u_tok.shape) != shape + (L,) or tuple(rand_tok.shape) != shape + (L,):
            raise ValueError(f"text_batch: the token draws must have shape {shape + (L,)}")
        if obj_masks is not None:
            if draws.u_obj is None or tuple(draws.u_obj.shape) != tuple(obj_masks.shape):
                raise ValueError("text_batch: draws.u_obj must have the shape of obj_masks")
            u_obj = draws.u_obj.to(device=dev, dtype=torch.float64).contiguous()
    seed_word("text_batch", seed_dev, dev, "texts")

    spec = [("txt_ids", torch.int64, shape + (L,)), ("txt_masks", torch.int64, shape + (L,))]
    if mask or (out is not None and "masked_lm_labels" in out):
        spec.append(("masked_lm_labels", torch.int64, shape + (L,)))
    if cap is not None:
        spec += [("scene_txt_ids", torch.int64, shape + (Ls,)), ("scene_txt_masks", torch.int64, shape + (Ls,))]
    if obj_masks is not None:
        spec.append(("obj_sem_masks", torch.bool, tuple(obj_masks.shape)))
    res = outputs("text_batch", spec, out, dev, "texts")
    cls_id, sep_id, mask_id, pad_id = (int(x) for x in special)
    # every output written once + at most one token read per position + the object flags read
    nbytes = (sum(t.numel() * t.element_size() for t in res.values()) + 4 * n_rows * (L + (Ls if cap is not None else 0))
              + n_obj_rows * O)
    launch("gps_text_batch", texts.n_texts, int(texts.tok.numel()), texts.tok, texts.off, n_rows, sent, cap, L, Ls,
           _NO_CAP if scene_sent_cap is None else int(scene_sent_cap), cls_id, sep_id, mask_id, pad_id, int(vocab_size),
           int(bool(mask)), float(txt_mask_ratio), float(pc_mask_ratio), n_obj_rows, O, obj_masks, u_tok, rand_tok, u_obj,
           u64(seed), seed_dev, res["txt_ids"], res["txt_masks"], res.get("masked_lm_labels"),
           res.get("scene_txt_ids"), res.get("scene_txt_masks"), res.get("obj_sem_masks"), device=dev,
           label=f"text_batch(rows={n_rows},L={L},Ls={Ls if cap is not None else 0})", nbytes=nbytes, what="text_batch")
    return as_bool(res, ("obj_sem_masks",))
