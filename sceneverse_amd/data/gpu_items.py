"""HBM-resident items of a pre-train / grounding split + the row's facts as ONE launch of libgps_hip.so.

Reference (what this replaces on the data-loader workers, per sample):
    ScanBase._getitem_refer       data/datasets/base.py:348-417  the item's scan, `obj_ids.index(tgt_object_instance)`,
                                                                 cat2int[instance_type], the sentence
    ScanBase._getitem_finalrefer  data/datasets/base.py:851-957  the same + np.random.choice of a scene caption (:851-856)

MI355X form: the items are uploaded ONCE (`PackedItems`, the twin of `gpu_qa.PackedQuestions`): per item its scan, the
target's position, `tgt_label` and the sentence's text id; per scan its object and proposal ranges and a CSR of caption
text ids.  A batch is then ONE integer per row -- the item's number -- and `item_rows` turns it into the range tables
and target positions `select_rows` takes and the text ids `text_batch` takes, on the device.  The rule is stated in
include/gps_hip.h (gps_item_rows); tests/augdraw_cases.py restates it.  GPU only: there is no CPU path here.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from .. import _native
from .._launch import launch
from ._resident import need_finalized, need_gpu, outputs, seed_word, u64
from .gpu_objects import PackedScans

_ITEM_OUT = (("scan_range", 2), ("prop_range", 2), ("tgt_obj", None), ("tgt_label", None), ("sent_idx", None),
             ("cap_idx", None), ("scan_idx", None))


class PackedItems:
    """The items of a split resident on the scans' device.  Build with add_item(...) x n and set_captions(...) per scan,
    then finalize()."""

    def __init__(self, packed: PackedScans, default_caption: int = -1):
        """packed: the finalized scans the items are about (their ranges and instance ids are read here, on the host).
        default_caption: the text id a scan without captions gets (-1: an empty text)."""
        need_finalized(packed.xyz, "PackedScans")
        self.packed = packed
        self.device = packed.xyz.device
        self.default_caption = int(default_caption)
        self._scan_no: Dict[str, int] = {sid: n for n, sid in enumerate(packed._scan_objs)}
        self._scan: List[int] = []
        self._tgt: List[int] = []
        self._label: List[int] = []
        self._sent: List[int] = []
        self._caps: Dict[int, List[int]] = {}
        self.item_scan = self.item_tgt = self.item_label = self.item_sent = None
        self.scan_range = self.prop_range = self.cap_first = self.cap_text = None
        self.n_caps_host: Optional[np.ndarray] = None

    def _scan_of(self, what: str, scan_id) -> int:
        if scan_id not in self._scan_no:
            raise ValueError(f"{what}: scan {scan_id!r} is not among the packed scans")
        return self._scan_no[scan_id]

    def add_item(self, scan_id: str, target_instance: int, tgt_label: int, sent_idx: int) -> int:
        """scan_id: the item's scan.  target_instance: the instance id of the referred object; its position among the
        scan's annotated objects is resolved through `packed.scan_inst_ids` (`obj_ids.index(tgt_object_instance)`).
        tgt_label: the reference's `cat2int[instance_type]`.  sent_idx: the sentence's text id in a PackedTexts.
        -> the item's number, what a batch refers to it by."""
        if self.item_scan is not None:
            raise ValueError("PackedItems: finalize() was already called")
        s = self._scan_of("add_item", scan_id)
        inst = self.packed.scan_inst_ids(scan_id)
        if target_instance not in inst:
            raise ValueError(f"add_item: instance {target_instance} is not an object of scan {scan_id!r}")
        self._scan.append(s)
        self._tgt.append(inst.index(target_instance))
        self._label.append(int(tgt_label))
        self._sent.append(int(sent_idx))
        return len(self._scan) - 1

    def set_captions(self, scan_id: str, text_ids: Sequence[int]) -> None:
        """The scan's captions (`scene_caps`), as text ids of a PackedTexts; a scan never named here has none."""
        if self.item_scan is not None:
            raise ValueError("PackedItems: finalize() was already called")
        self._caps[self._scan_of("set_captions", scan_id)] = [int(t) for t in text_ids]

    def finalize(self) -> "PackedItems":
        """The device tables of gps_item_table."""
        if self.item_scan is not None:
            raise ValueError("PackedItems: finalize() was already called")
        packed, n_scans = self.packed, len(self._scan_no)
        ann, prop = np.zeros((n_scans, 2), np.int32), np.zeros((n_scans, 2), np.int32)
        for sid, s in self._scan_no.items():
            objs = packed.scan_objects(sid)
            ann[s] = (objs.start, objs.stop)
            if sid in packed._scan_props:
                props = packed.scan_proposals(sid)
                prop[s] = (props.start, props.stop)
        caps = [self._caps.get(s, []) for s in range(n_scans)]
        first = np.zeros(n_scans + 1, np.int64)
        np.cumsum([len(c) for c in caps], out=first[1:])

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

        self.item_scan, self.item_tgt, self.item_label, self.item_sent = (up(x) for x in (self._scan, self._tgt, self._label,
                                                                                           self._sent))
        self.scan_range, self.prop_range = up(ann), up(prop)
        self.cap_first, self.cap_text = up(first), up([t for c in caps for t in c])
        self.n_caps_host = np.diff(first)
        return self

    @property
    def n_items(self) -> int:
        return len(self._scan)

    def table(self) -> "_native.ItemTable":
        z = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        return _native.ItemTable(self.n_items, int(self.scan_range.shape[0]), int(self.cap_text.numel()),
                                 self.default_caption, z(self.item_scan), z(self.item_tgt), z(self.item_label),
                                 z(self.item_sent), z(self.scan_range), z(self.prop_range), self.cap_first.data_ptr(),
                                 z(self.cap_text))


def item_rows(items: PackedItems, item_ids, pick=None, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
              out: Optional[dict] = None) -> dict:
    """A pre-train / grounding batch's look-ups in one launch and without a host sync, from one item number per row; the
    rule and its undefined rows are stated in include/gps_hip.h.

    -> dict, all int32 on the scans' device: scan_range, prop_range (B, 2), the tables `select_rows` takes as `scan_ids`
    ('gt': scan_range; 'pred': the pair); tgt_obj (B) the target's position in its scan and tgt_label (B), `select_rows`'
    and `refer_targets`' arguments of those names; sent_idx, cap_idx (B) the text ids `text_batch` takes; scan_idx (B).

    item_ids: (B) item numbers (`add_item`'s), a sequence or a tensor on any device; a number outside the table gives an
    undefined row (empty ranges, text ids -1) -- `select_rows` makes an empty row of it and `text_batch` an empty text.
    pick: (B) a replay of `np.random.choice(len(scene_caps))`; None = drawn on the device from seed + *seed_dev (stream
    seed + 5, so `text_batch`, `select_rows` and `draw_aug_table` share the word).  A scan without captions gets the
    table's default_caption.  out: optional dict of preallocated contiguous tensors under the names above, IN PLACE."""
    need_finalized(items.item_scan, "PackedItems")
    dev = items.device
    ids = item_ids if torch.is_tensor(item_ids) else torch.as_tensor(np.asarray(item_ids))
    ids = ids.reshape(-1)
    B = int(ids.numel())
    if B == 0:
        ids = ids.to(torch.int32)
    if ids.dtype.is_floating_point or ids.dtype == torch.bool:
        raise ValueError(f"item_rows: item_ids must hold {B} integers")
    if pick is not None:
        pick = pick if torch.is_tensor(pick) else torch.as_tensor(np.asarray(pick))
        pick = pick.reshape(-1)
        if pick.numel() != B or pick.dtype.is_floating_point or pick.dtype == torch.bool:
            raise ValueError(f"item_rows: pick must hold {B} integers")
    need_gpu(dev, "item_rows", "scenes")
    seed_word("item_rows", seed_dev, dev, "scans")
    ids = ids.to(device=dev, dtype=torch.int32).contiguous()
    if pick is not None:
        pick = pick.to(device=dev, dtype=torch.int32).contiguous()
    spec = [(name, torch.int32, (B,) if w is None else (B, w)) for name, w in _ITEM_OUT]
    res = outputs("item_rows", spec, out, dev, "scans")
    table = items.table()
    launch("gps_item_rows", B, ctypes.byref(table), ids, pick, u64(seed), seed_dev, *[res[name] for name, _ in _ITEM_OUT],
           device=dev, label=f"item_rows(B={B})", nbytes=4 * B * (9 + 12), what="item_rows")
    return res
