"""A pre-train / grounding batch from one item id per row: the resident loader's launches as one capturable chain.

Reference (what the chain replaces on the data-loader workers, per sample): ScanBase._getitem_refer / _getitem_finalrefer
(data/datasets/base.py:348-457, :851-957), DataAugmentor (data/datasets/data_augmentor.py), ScanBase._obj_processing_aug
(base.py:742-776) and MaskDatasetWrapper / ScanFamilyDatasetWrapperOld (data/datasets/dataset_wrapper.py:38-111, :164-191).

    item_rows -> select_rows(mode="refer") [-> refer_targets("gt")] -> draw_aug_table -> obj_processing_aug -> text_batch

Every launch draws from the same `seed` and the same device word `seed_dev` (streams seed .. seed + 6 and the object
path's own key, include/gps_hip.h), no launch waits for the host and no table is built there, so the chain can be
captured once in a `torch.cuda.graph` next to the captured training step and write into `GPSTrainStep.static_inputs()`;
the caller advances the word with `seed_dev.add_(1)`, inside or outside the capture.
"""
from __future__ import annotations

from typing import Optional

import torch

from .gpu_items import PackedItems, item_rows
from .gpu_objects import PackedScans, draw_aug_table, obj_processing_aug, refer_targets, select_rows
from .gpu_text import PackedTexts, text_batch


def pretrain_batch(packed: PackedScans, texts: PackedTexts, items: PackedItems, item_ids, max_keep: int,
                   O: Optional[int] = None, num_points: int = 1024, pc_type: str = "gt", aug_cfg=None, split: str = "train",
                   mask: bool = True, keep: Optional[torch.Tensor] = None, label_map: Optional[torch.Tensor] = None,
                   pick=None, seed: int = 0, seed_dev: Optional[torch.Tensor] = None, out: Optional[dict] = None,
                   **text_kw) -> dict:
    """item_ids (B) -> the data_dict of MaskDatasetWrapper (mask=True) or ScanFamilyDatasetWrapperOld (mask=False) on the
    device: obj_fts (B,O,num_points,6) f32, obj_locs (B,O,6) f32, obj_masks, obj_sem_masks (B,O) bool, obj_labels (B,O)
    int64, txt_ids, txt_masks, masked_lm_labels (B,L) int64, scene_txt_ids, scene_txt_masks (B,Ls) int64, tgt_object_id
    (B,1), tgt_object_id_iou25 / _iou50 (B,O) int64, is_multiple, is_hard (B) bool -- plus what the launches on the way
    wrote (`item_rows`' and `select_rows`' outputs and the drawn table as aug_entries / aug_row).

    max_keep, O, keep, label_map: `select_rows`' arguments (keep is required for pc_type 'gt').  pc_type 'pred': rows of
    the scans' proposals, the targets from the selection launch itself; 'gt': `refer_targets(..., "gt")`.
    aug_cfg, split: the `data_aug:` block and the split, as `draw_aug_table` takes them (None or a split other than
    'train': nothing is drawn and nothing applied, the reference's validation path).  pick: a replay of the caption
    choice.  text_kw: `text_batch`'s max_seq_len, max_scene_cap_len, scene_sent_cap, txt_mask_ratio, pc_mask_ratio,
    special, vocab_size.  seed, seed_dev: one seed and one int64 device word for every launch.
    out: optional dict of preallocated tensors under ALL the names of the result, written IN PLACE (the result of an
    earlier call serves).  With item_ids, keep and label_map already on the device the call never waits for the host and
    uploads nothing: it is capturable."""
    if pc_type not in ("gt", "pred"):
        raise ValueError(f"pretrain_batch: pc_type {pc_type!r} is neither 'gt' nor 'pred'")
    pred = pc_type == "pred"
    rows = item_rows(items, item_ids, pick=pick, seed=seed, seed_dev=seed_dev, out=out)
    B = int(rows["tgt_obj"].shape[0])
    ranges = (rows["scan_range"], rows["prop_range"]) if pred else rows["scan_range"]
    sel = select_rows(packed, ranges, max_keep, O, tgt_obj=rows["tgt_obj"], mode="refer", keep=keep, label_map=label_map,
                      seed=seed, seed_dev=seed_dev, out=out, pc_type=pc_type, tgt_label=rows["tgt_label"] if pred else None,
                      targets=pred)
    n_slots = int(sel["row_obj"].shape[1])
    res = {**rows, **sel}
    if not pred:
        res.update(refer_targets(packed, sel["row_obj"], rows["tgt_obj"], rows["scan_range"], "gt", out=out))
    aug_out = None if out is None else {"entries": out.get("aug_entries"), "row_aug": out.get("aug_row")}
    aug = draw_aug_table(aug_cfg, split, B, n_slots, seed=seed, seed_dev=seed_dev, out=aug_out, device=packed.xyz.device)
    if aug is not None:
        res["aug_entries"], res["aug_row"] = aug.entries, aug.row_aug
    res.update(obj_processing_aug(packed, sel["row_obj"], num_points, aug=aug, seed=seed, seed_dev=seed_dev, out=out))
    res.update(text_batch(texts, rows["sent_idx"], rows["cap_idx"], mask=mask, obj_masks=res["obj_masks"], seed=seed,
                          seed_dev=seed_dev, out=out, **text_kw))
    return res
