"""HBM-resident scenes + the loader's per-object processing as ONE launch of libgps_hip.so.

Reference (what this replaces on the data-loader workers):
    ScanBase._load_scan            data/datasets/base.py:65-142   per scan: pcds = [points | colors/127.5-1],
                                                                  obj_pcds = [pcds[instance_labels == id] ...]
    ScanBase._obj_processing_post  data/datasets/base.py:697-740  rotate, obj_locs, box, subsample, normalise
    ScanBase._obj_processing_aug   data/datasets/base.py:742-776  the branch of every config with a `data_aug:` block
    DataAugmentor                  data/datasets/data_augmentor.py  its draws (:39-154) and their application (:156-215)
    dataset wrapper padding        data/datasets/dataset_wrapper.py:62-70  pad to max_obj_len, obj_masks
    ScanBase._getitem_refer        data/datasets/base.py:348-417  `pc_type: 'pred'`: predicted proposals (loaded at
                                                                  :115-141), labels / flags / target id by box IoU
    object selection, 'gt'         data/datasets/base.py:231-246, :275-289, :368-450, :877-957  background filter, target-
                                                                  first crop, random fill; :485-488 is_multiple / is_hard

MI355X form: every scan is uploaded ONCE in its raw on-disk precision (xyz f32 + rgb u8, packed as
16-byte records, instead of the loader's 48 B/point float64 rows), points regrouped so that each kept instance is
contiguous (same within-instance order as `pcds[mask]`), with a CSR offset table.  A training batch
is then described by a (B, max_obj_len) table of object ids; `obj_processing_post` turns it into the
model's `obj_fts / obj_locs / obj_masks` (+ boxes) on the device -- no per-object host work, no
126 MB/step host-to-device copy.  GPU only: there is no CPU path here (the reference's own loader IS
the CPU path; oracle/obj_processing.py restates it for the tests).
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, List, Mapping, Optional, Sequence

import numpy as np
import torch

from .. import _native
from .._launch import launch
from ._resident import as_bool, need_finalized, need_gpu, outputs, seed_word, u64


class PackedScans:
    """Raw scans resident on one device.  Build with add_scan(...) x n, then finalize()."""

    def __init__(self, device: torch.device | str = "cuda", records: bool = True):
        """records=True (default, uint8 colours only): store points as 16-byte records {x, y, z f32; r, g, b
        u8; pad} -- one aligned vector load per point, colours gathered with the coordinates.
        records=False: xyz (N,3) and rgb (N,3) as two arrays (also the layout for float32 colours)."""
        self.device = torch.device(device)
        self.records = records
        self._xyz: List[np.ndarray] = []
        self._rgb: List[np.ndarray] = []
        self._sizes: List[int] = []
        self._scan_objs: Dict[str, range] = {}
        self._scan_props: Dict[str, range] = {}
        self._inst_ids: Dict[str, list] = {}
        self._labels: List[int] = []
        self.xyz = self.rgb = self.obj_offsets = None
        self.labels = self.boxes = self.match_labels = None
        self.sizes_host: Optional[np.ndarray] = None

    def add_scan(self, scan_id: str, points: np.ndarray, colors: np.ndarray, instance_labels: np.ndarray,
                 inst_ids: Sequence[int], inst_labels: Optional[Sequence[int]] = None) -> None:
        """points (N,3) float32, colors (N,3) uint8 or float32 in 0..255 (the `.pth` contents of
        base.py:70-73), instance_labels (N,), inst_ids: the instances the loader keeps, in its order
        (base.py:82-89; instances without points are skipped exactly like `np.sum(mask) == 0`).
        inst_labels: optionally the class of each entry of inst_ids (base.py:90) -> the per-object `labels` array;
        objects of a scan added without it carry -100."""
        assert self.xyz is None, "finalize() was already called"
        if inst_labels is not None and len(inst_labels) != len(inst_ids):
            raise ValueError("inst_labels must give one label per entry of inst_ids")
        points, colors = self._arrays(points, colors)
        first = len(self._sizes)
        kept = [inst for n, inst in enumerate(inst_ids)
                if self._append(points, colors, instance_labels == inst, -100 if inst_labels is None else inst_labels[n])]
        self._scan_objs[scan_id] = range(first, len(self._sizes))
        self._inst_ids[scan_id] = kept

    def add_proposals(self, scan_id: str, points: np.ndarray, colors: np.ndarray, masks: np.ndarray,
                      labels: Sequence[int]) -> None:
        """The predicted instance masks of a scan (base.py:115-141 after its `[:50]` cut, which is the caller's): masks
        (n_prop, N) bool / 0-1 over the scan's points, labels (n_prop,).  Every proposal with at least one point becomes
        one more object of the packed arrays, its points in `pcds[mask == 1]` order; masks may overlap (a point is then
        stored once per proposal) and empty ones are skipped like `pcds[mask == 1].shape[0] > 0`.  Call it after
        add_scan for the same scan (same points and colors) and before finalize()."""
        assert self.xyz is None, "finalize() was already called"
        if scan_id not in self._scan_objs:
            raise KeyError(f"add_proposals: add_scan({scan_id!r}) comes first")
        if scan_id in self._scan_props:
            raise ValueError(f"add_proposals: scan {scan_id!r} already has its proposals")
        points, colors = self._arrays(points, colors)
        masks = np.asarray(masks).reshape(-1, points.shape[0])
        if len(labels) != masks.shape[0]:
            raise ValueError("add_proposals: one label per mask")
        first = len(self._sizes)
        for mask, label in zip(masks, labels):
            self._append(points, colors, mask == 1, label)
        self._scan_props[scan_id] = range(first, len(self._sizes))

    def _arrays(self, points: np.ndarray, colors: np.ndarray):
        """A scan's points as float32 and its colours as stored: uint8, or float32 for anything else; one dtype per store."""
        if colors.dtype != np.uint8:
            colors = np.ascontiguousarray(colors, dtype=np.float32)
        if self._rgb and self._rgb[0].dtype != colors.dtype:
            raise ValueError("all scans must store colours in the same dtype")
        return np.ascontiguousarray(points, dtype=np.float32), colors

    def _append(self, points: np.ndarray, colors: np.ndarray, mask: np.ndarray, label) -> bool:
        """The points under `mask` as one more object, in `pcds[mask]` order; False (nothing stored) when there are none."""
        sel = np.flatnonzero(mask)
        if sel.size == 0:
            return False
        self._xyz.append(points[sel])
        self._rgb.append(np.ascontiguousarray(colors[sel]))
        self._sizes.append(int(sel.size))
        self._labels.append(int(label))
        return True

    def finalize(self) -> "PackedScans":
        sizes = np.asarray(self._sizes, dtype=np.int64)
        off = np.zeros(len(sizes) + 1, dtype=np.int64)
        np.cumsum(sizes, out=off[1:])
        self.sizes_host = sizes
        xyz = np.concatenate(self._xyz, 0) if self._xyz else np.zeros((0, 3), np.float32)
        rgb = np.concatenate(self._rgb, 0) if self._rgb else np.zeros((0, 3), np.uint8)
        if self.records and rgb.dtype == np.uint8:
            rec = np.zeros((xyz.shape[0], 4), dtype=np.float32)
            rec[:, :3] = xyz
            rec.view(np.uint8).reshape(-1, 16)[:, 12:15] = rgb
            self.xyz, self.rgb = torch.from_numpy(rec).to(self.device), None
        else:
            self.records = False
            self.xyz, self.rgb = torch.from_numpy(xyz).to(self.device), torch.from_numpy(rgb).to(self.device)
        self.obj_offsets = torch.from_numpy(off).to(self.device)
        self.labels = torch.from_numpy(np.asarray(self._labels, dtype=np.int32)).to(self.device)
        self._xyz, self._rgb = [], []
        if self.device.type == "cuda":             # the boxes are a device product: no CPU path
            self.boxes = obj_boxes(self)
            self.match_labels = proposal_labels(self)
        return self

    def scan_objects(self, scan_id: str) -> range:
        """Global object ids of a scan's annotated objects, in the loader's object order."""
        return self._scan_objs[scan_id]

    def scan_proposals(self, scan_id: str) -> range:
        """Global object ids of a scan's proposals (add_proposals), in mask order without the empty ones."""
        return self._scan_props[scan_id]

    def scan_inst_ids(self, scan_id: str) -> list:
        return self._inst_ids[scan_id]

    @property
    def n_objects(self) -> int:
        return 0 if self.sizes_host is None else int(self.sizes_host.shape[0])


def batch_rows(packed: PackedScans, scan_ids: Sequence[str], max_obj_len: int,
               obj_select: Optional[Sequence[Sequence[int]]] = None, proposals: bool = False) -> torch.Tensor:
    """(B, max_obj_len) int32 table of global object ids, -1 = padding slot.  obj_select[b] optionally
    lists scene-local object positions (the loader's selected_obj_idxs, base.py:236-246).  proposals=True fills
    the rows from the scans' proposals (`pc_type: 'pred'`) instead of their annotated objects."""
    rows = np.full((len(scan_ids), max_obj_len), -1, dtype=np.int32)
    for b, sid in enumerate(scan_ids):
        objs = list(packed.scan_proposals(sid) if proposals else packed.scan_objects(sid))
        if obj_select is not None:
            objs = [objs[i] for i in obj_select[b]]
        if len(objs) > max_obj_len:
            hint = '; select_rows(pc_type="pred") crops such a scan' if proposals else ""
            raise ValueError(f"scan {sid}: {len(objs)} objects > max_obj_len {max_obj_len}{hint}")
        rows[b, :len(objs)] = objs
    return torch.from_numpy(rows)


def scan_ranges(packed: PackedScans, scan_ids, proposals: bool = False) -> torch.Tensor:
    """(B, 2) int32 [first, last) global ids of the scans' annotated objects, on the scans' device: what `select_rows`
    and `refer_targets` read.  A tensor of that form is passed through (after a shape / dtype / device check), so a
    loader builds the table once per batch, or once per epoch, outside any captured region.
    proposals=True: the ranges of the scans' proposals (`add_proposals`; KeyError for a scan without them), the second
    table `select_rows(pc_type="pred")` reads."""
    dev = packed.xyz.device
    if torch.is_tensor(scan_ids):
        if scan_ids.dim() != 2 or scan_ids.shape[1] != 2 or scan_ids.dtype != torch.int32 or scan_ids.device != dev:
            raise ValueError("scan_ranges: a range table must be (B, 2) int32 on the scans' device")
        return scan_ids.contiguous()
    of = packed.scan_proposals if proposals else packed.scan_objects
    ranges = np.asarray([[r.start, r.stop] for r in (of(s) for s in scan_ids)],
                        dtype=np.int32).reshape(len(scan_ids), 2)
    return torch.from_numpy(ranges).to(dev)


# ---- which objects enter the batch: filter, crop, random fill ------------------------------------------------
OBJ_SELECT_MAX_SCAN = 1024                       # GPS_OBJ_SELECT_MAX_SCAN of include/gps_hip.h
_SELECT_MODES = {"refer": 0, "pretrain": 1}      # GPS_OBJ_SELECT_REFER / _PRETRAIN
_SELECT_OUT = (("row_obj", torch.int32), ("tgt_slot", torch.int32), ("n_sel", torch.int32), ("n_rem", torch.int32),
               ("is_multiple", torch.bool), ("is_hard", torch.bool))
BACKGROUND = ("wall", "floor", "ceiling")


def keep_table(int2cat: Sequence[str], drop: Sequence[str] = BACKGROUND, only: Optional[Sequence[str]] = None) -> torch.Tensor:
    """(n_labels,) bool: label l is kept iff int2cat[l] is not in `drop` (the loader's wall / floor / ceiling filter,
    base.py:232-233, :380-381) and, with `only`, is one of those names (`only=CLASS_LABELS_200`: the filter of
    _getitem_obj_pretrain, base.py:276-277).  For `filter_lang` build a (B, n_labels) table: row b keeps label l iff
    this table does and `int2cat[l] in sentence_b` (base.py:371-373)."""
    drop = set(drop)
    only = None if only is None else set(only)
    return torch.tensor([(c not in drop) and (only is None or c in only) for c in int2cat], dtype=torch.bool)


def select_rows(packed: PackedScans, scan_ids, max_keep: int, O: Optional[int] = None, tgt_obj=None, mode: str = "refer",
                keep: Optional[torch.Tensor] = None, label_map: Optional[torch.Tensor] = None,
                order: Optional[torch.Tensor] = None, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
                out: Optional[dict] = None, pc_type: str = "gt", tgt_label=None, targets: bool = False) -> dict:
    """The loader's object selection for `pc_type: 'gt'` (base.py:231-246, :275-289, :368-450, :877-957) for a whole
    batch in one launch and without a host sync: drop the background (the referred object stays), and where more than
    `max_keep` objects remain put the target first, then its class, then a random choice of the rest -- redrawn every
    call.  `batch_rows` only copies ranges and raises on such a scan; the rule is stated in include/gps_hip.h.

    -> dict: row_obj (B, O) int32 global object ids, -1 = padding -- the table `obj_processing_post`, `obj_processing_aug`
    and `refer_targets(..., "gt")` take; tgt_slot (B) int32, the target's slot (the loader's tgt_object_id; -1 in
    'pretrain' mode); n_sel (B) int32 objects in the row; n_rem (B) int32, how many objects the random fill chose from
    (0 = no fill); is_multiple, is_hard (B) bool (base.py:485-488; both False in 'pretrain' mode).

    scan_ids: the rows' scans, or their `scan_ranges` table.  max_keep: objects a row may hold -- the loader's
    `max_obj_len`, which ScanNetSpatialRefer sets to the config's value - 1 (scannet.py:50).  O: slots per row,
    default max_keep + 1 in 'refer' mode (refer_targets' flag vectors need one spare slot) and max_keep in 'pretrain'.
    tgt_obj: per row the position of the referred object among its scan's annotated objects, as in `refer_targets`.
    keep: `keep_table(...)`, (n_labels,) or per row (B, n_labels), bool / uint8.  label_map: (n_labels,) the reference's
    id_to_scannetid for is_multiple (ScanNetSpatialRefer); None = identity, the _getitem_finalrefer form.
    order: (B, R >= max_keep) int32, per row what `random.shuffle` made of `list(range(n_rem))` -- a replay of the
    reference's draw; None = drawn on the device from seed + *seed_dev by the law of include/gps_hip.h (seed_dev: one
    int64 word on the device, advanced there between graph replays; the stream is seed + 3, so `text_batch` can share
    the word).  out: optional dict of preallocated contiguous tensors under the names above (int32; the flags bool or
    uint8), written IN PLACE.
    A scan of more than OBJ_SELECT_MAX_SCAN objects, max_keep > O and a target given on the host outside its scan are
    refused here (ValueError); in a device table such a row comes out empty (n_sel 0, tgt_slot -1).

    pc_type="pred": the rows are filled from the scans' PROPOSALS (`add_proposals`).
    'refer' mode is the crop of base.py:420-450 in one launch of gps_obj_select_pred (rule and its two differences from
    the reference: include/gps_hip.h): every proposal that overlaps the referred annotated object by IoU >= 0.25 first,
    in ascending order, then the proposals of the target's class by `packed.match_labels`, then the random fill.  `keep`
    is not read (the reference filters nothing there; given, only its width bounds the labels that count);
    tgt_label: (B,) the reference's `cat2int[instance_type]` where it differs from the target's own label, None = that
    label.  scan_ids: the scans, or the pair (scan_ranges(packed, ids), scan_ranges(packed, ids, proposals=True)) of
    device tables.  tgt_slot is the slot of the LAST overlapping proposal, -1 when there is none.  targets=True: the
    result also carries tgt_object_id_iou25 / _iou50 (B, O) int64, tgt_object_id (B, 1) int64 and obj_labels (B, O)
    int64 in `refer_targets`' layouts, bit-equal to `refer_targets(row_obj, ..., "pred")` -- a 'pred' batch is one
    launch; `out=` accepts them too.
    'pretrain' mode is _getitem_pretrain on inst_labels_pred (base.py:227-246): the 'gt' selection over the proposals'
    ranges with their raw labels (scan_ids: the scans or their proposals' range table)."""
    need_finalized(packed.xyz, "PackedScans")
    if mode not in _SELECT_MODES:
        raise ValueError(f"select_rows: mode {mode!r} is neither 'refer' nor 'pretrain'")
    if pc_type not in ("gt", "pred"):
        raise ValueError(f"select_rows: pc_type {pc_type!r} is neither 'gt' nor 'pred'")
    refer = mode == "refer"
    pred = pc_type == "pred"
    hits = pred and refer                        # the IoU-hit crop, gps_obj_select_pred: the one branch below
    if (tgt_label is not None or targets) and not hits:
        raise ValueError("select_rows: tgt_label and targets belong to pc_type='pred' in 'refer' mode")
    M = int(max_keep)
    O = (M + 1 if refer else M) if O is None else int(O)
    if M < 1 or M > O:
        raise ValueError(f"select_rows: max_keep {M} must lie in [1, O = {O}]")
    if refer and M < 2:
        raise ValueError("select_rows: 'refer' mode needs max_keep >= 2")
    if O > REFER_MAX_OBJ:
        raise ValueError(f"select_rows: {O} object slots > {REFER_MAX_OBJ}")
    if refer and tgt_obj is None:
        raise ValueError("select_rows: 'refer' mode needs tgt_obj")
    if keep is None and not hits:
        raise ValueError("select_rows: keep is required (see keep_table)")
    # the rows' scans: ids on the host, or ready-made range tables -- for the hits a pair, annotated objects and proposals
    if hits:
        host_ids = not (isinstance(scan_ids, (tuple, list)) and len(scan_ids) == 2 and all(torch.is_tensor(t) for t in scan_ids))
        if host_ids and torch.is_tensor(scan_ids):
            raise ValueError("select_rows: pc_type='pred' takes scan ids or the pair (scan_ranges(..), scan_ranges(.., proposals=True))")
        B = len(scan_ids) if host_ids else int(scan_ids[0].shape[0])
    else:
        host_ids = not torch.is_tensor(scan_ids)
        B = len(scan_ids)
    if host_ids:
        if refer:                                # what tgt_obj indexes: the annotated objects
            sizes = [len(packed.scan_objects(s)) for s in scan_ids]
        for sid in scan_ids:
            n = len(_scan_proposals(packed, sid) if pred else packed.scan_objects(sid))
            if n > OBJ_SELECT_MAX_SCAN:
                raise ValueError(f"select_rows: scan {sid} has {n} {'proposals' if pred else 'objects'} > {OBJ_SELECT_MAX_SCAN}")
    tgt = None
    if refer:
        tgt = torch.as_tensor(tgt_obj).reshape(-1)
        if tgt.numel() == 0:                     # an empty list has no integer dtype of its own
            tgt = tgt.to(torch.int32)
        if tgt.numel() != B or tgt.dtype.is_floating_point or tgt.dtype == torch.bool:
            raise ValueError(f"select_rows: tgt_obj must hold {B} integer positions")
        if host_ids and tgt.device.type == "cpu" and any(not 0 <= int(t) < n for t, n in zip(tgt.tolist(), sizes)):
            raise ValueError("select_rows: a target position outside its scan")
    if tgt_label is not None:
        tgt_label = torch.as_tensor(tgt_label).reshape(-1)
        if tgt_label.numel() != B or tgt_label.dtype.is_floating_point or tgt_label.dtype == torch.bool:
            raise ValueError(f"select_rows: tgt_label must hold {B} integer labels")
    R = 0
    if order is not None:
        if order.dim() != 2 or order.shape[0] != B or order.shape[1] < M or order.dtype.is_floating_point:
            raise ValueError(f"select_rows: order must be (B, R >= {M}) integers")
        R = int(order.shape[1])
    dev = packed.xyz.device
    need_gpu(dev, "select_rows", "scenes")
    if hits:
        ids, prop_ids = (scan_ids, scan_ids) if host_ids else scan_ids
        ranges, props = scan_ranges(packed, ids), scan_ranges(packed, prop_ids, proposals=True)
        if props.shape[0] != B:
            raise ValueError("select_rows: the two range tables must have one row per batch row")
    else:
        ranges = scan_ranges(packed, scan_ids, proposals=pred)
    if refer:
        tgt = tgt.to(device=dev, dtype=torch.int32) + ranges[:, 0]
    if tgt_label is not None:
        tgt_label = tgt_label.to(device=dev, dtype=torch.int32).contiguous()
    n_labels = (1 << 31) - 1                     # the hits without a table: every non-negative label counts
    if keep is not None:
        n_labels = int(keep.shape[-1])
    if not hits:                                 # the hits read no keep table: given, only its width counts
        if keep.dtype not in (torch.bool, torch.uint8) or keep.dim() not in (1, 2) or (keep.dim() == 2 and keep.shape[0] != B):
            raise ValueError("select_rows: keep must be (n_labels,) or (B, n_labels) bool / uint8")
        keep = keep.to(dev).contiguous()
    if label_map is not None:
        if label_map.dim() != 1 or label_map.dtype.is_floating_point or (keep is not None and label_map.shape[0] != n_labels):
            raise ValueError("select_rows: label_map must hold n_labels integers, as many as keep has columns")
        n_labels = int(label_map.shape[0])
        label_map = label_map.to(device=dev, dtype=torch.int32).contiguous()
    if order is not None:
        order = order.to(device=dev, dtype=torch.int32).contiguous()
    seed_word("select_rows", seed_dev, dev, "scans")
    spec = [(name, dt, (B, O) if name == "row_obj" else (B,)) for name, dt in _SELECT_OUT]
    if targets:
        spec += _refer_spec(B, O)
    res = outputs("select_rows", spec, out, dev, "scans")
    rows = [res[name] for name, _ in _SELECT_OUT]
    if hits:
        tout = [res[name] if targets else None for name, _ in _REFER_OUT]
        launch("gps_obj_select_pred", B, O, M, packed.n_objects, n_labels, packed.boxes, packed.labels, packed.match_labels,
               ranges, props, tgt, tgt_label, label_map, order, R, u64(seed), seed_dev, *rows, *tout,
               device=dev, label=f"obj_select_pred(B={B},O={O},M={M})",
               nbytes=4 * B * (O + 8) + 2 * B + (24 * B * O if targets else 0) + 52 * B * 256,
               what="select_rows")     # outputs + ranges and target + a box and a label per position (scans of some 256 proposals)
    else:
        launch("gps_obj_select", B, O, M, _SELECT_MODES[mode], packed.n_objects, n_labels, packed.labels, ranges, tgt, keep,
               n_labels if keep.dim() == 2 else 0, label_map, order, R, u64(seed), seed_dev, *rows, device=dev,
               label=f"obj_select(B={B},O={O},M={M})", nbytes=4 * B * (O + 6) + 2 * B + 4 * B * OBJ_SELECT_MAX_SCAN // 4,
               what="select_rows")     # outputs + ranges and target + a label per position (scans of some 256 objects)
    return as_bool(res, ("is_multiple", "is_hard"))


def _scan_proposals(packed: PackedScans, scan_id) -> range:
    try:
        return packed.scan_proposals(scan_id)
    except KeyError:
        raise ValueError(f"select_rows: scan {scan_id!r} has no proposals (add_proposals)") from None


def obj_processing_post(packed: PackedScans, row_obj: torch.Tensor, num_points: int = 1024,
                        rot: Optional[torch.Tensor] = None, sample_idx: Optional[torch.Tensor] = None,
                        seed: int = 0, need_boxes: bool = False, out: Optional[dict] = None,
                        seed_dev: Optional[torch.Tensor] = None) -> dict:
    """row_obj (B, O) int32 object ids (-1 = padding) -> dict with obj_fts (B,O,num_points,6) f32,
    obj_locs (B,O,6) f32, obj_masks (B,O) bool [, obj_boxes (B,O,6) f32].

    rot: per-scene rotations (build_rotate_mat's matrix): a (B,3,3) tensor/array, or a length-B list
    with None for the scenes it left unrotated; None = no rotation at all.  A ready pair (mats (n,3,3) f32,
    row_rot (B*O,) int32) of tensors on the scans' device -- `draw_rot_table`'s -- is passed through untouched.
    sample_idx: (B,O,num_points) int32 object-local indices (np.random.choice draws, for bit-compatible
    replays of the reference loader) or None = drawn on the device from `seed`.
    seed_dev: one int64 word on the scans' device: the samples are drawn from seed + *seed_dev, read on the device, so
    a captured launch redraws when the word is advanced between replays (gps_obj_processing_post_sw); None = `seed`.
    out: optional {"obj_fts", "obj_locs", "obj_masks"} of preallocated contiguous tensors of those shapes (obj_masks bool
    or uint8) the kernel writes IN PLACE -- the static input buffers of a captured training step
    (`GPSTrainStep.static_inputs()`), so that no per-step copy of the 126 MB of object points is needed."""
    dev = _obj_device(packed, "obj_processing_post")
    B, O = row_obj.shape
    n_rows = B * O
    nbytes = _algorithmic_bytes(packed, row_obj if row_obj.device.type == "cpu" else None, n_rows, num_points)
    row_obj, sample_idx, res = _obj_buffers("obj_processing_post", row_obj, num_points, sample_idx, need_boxes, out, dev)
    rot_t = row_rot = None
    if rot is not None:
        rot_t, row_rot = _rot_pair(rot, n_rows, dev) or rot_rows(rot, B, O, dev)
    seed_word("obj_processing_post", seed_dev, dev, "scans")
    word = () if seed_dev is None else (seed_dev,)
    launch("gps_obj_processing_post" + ("_sw" if word else ""), n_rows, num_points, packed.xyz, packed.rgb,
           int(packed.rgb is None or packed.rgb.dtype == torch.uint8), packed.obj_offsets, row_obj, sample_idx,
           u64(seed), *word, rot_t, row_rot, res["obj_fts"], res["obj_locs"], res.get("obj_boxes"), res["obj_masks"], device=dev,
           label=f"obj_processing_post(rows={n_rows},P={num_points})", nbytes=nbytes, what="obj_processing_post")
    return as_bool(res, ("obj_masks",))


def _rot_pair(rot, n_rows: int, dev):
    """`rot` when it is a ready (mats (n,3,3) f32, row_rot (B*O,) int32) pair of device tensors, else None."""
    if not (isinstance(rot, tuple) and len(rot) == 2 and all(torch.is_tensor(t) for t in rot)):
        return None
    mats, row_rot = rot
    if (mats.dim() != 3 or tuple(mats.shape[1:]) != (3, 3) or mats.dtype != torch.float32 or row_rot.dtype != torch.int32
            or tuple(row_rot.shape) != (n_rows,) or mats.device != dev or row_rot.device != dev
            or not mats.is_contiguous() or not row_rot.is_contiguous()):
        raise ValueError(f"obj_processing_post: a rotation pair is (mats (n,3,3) float32, row_rot ({n_rows},) int32), "
                         "contiguous, on the scans' GPU")
    return mats, row_rot


def _obj_device(packed: PackedScans, what: str) -> torch.device:
    """The two guards of a call that checks nothing on the host between them -> the scans' GPU."""
    need_finalized(packed.xyz, "PackedScans")
    need_gpu(packed.xyz.device, what, "scenes")
    return packed.xyz.device


def _obj_buffers(what: str, row_obj: torch.Tensor, num_points: int, sample_idx, need_boxes: bool, out, dev):
    """What obj_processing_post and obj_processing_aug share past their guards -> (the row table and the replayed sample
    indices as the launch reads them, the result dict: `out`'s tensors or new ones, obj_boxes always new)."""
    B, O = row_obj.shape
    row_obj = row_obj.to(device=dev, dtype=torch.int32).contiguous()
    if sample_idx is not None:
        sample_idx = sample_idx.to(device=dev, dtype=torch.int32).contiguous()
        assert sample_idx.shape == (B, O, num_points), sample_idx.shape
    res = outputs(what, (("obj_fts", torch.float32, (B, O, num_points, 6)), ("obj_locs", torch.float32, (B, O, 6)),
                         ("obj_masks", torch.uint8, (B, O))), out, dev, "scans")
    if need_boxes:
        res["obj_boxes"] = torch.empty((B, O, 6), dtype=torch.float32, device=dev)
    return row_obj, sample_idx, res


# ---- ScanRefer targets: boxes of every object, IoU flags per batch ---------------------------------------------
BOXES_CHUNK = 4096                               # GPS_OBJ_BOXES_CHUNK of include/gps_hip.h
REFER_MAX_OBJ = 512                              # GPS_REFER_MAX_OBJ
_REFER_OUT = (("tgt_object_id_iou25", None), ("tgt_object_id_iou50", None), ("tgt_object_id", 1), ("obj_labels", None))


def _refer_spec(B: int, O: int) -> list:
    """(name, dtype, shape) of the four target tensors, for `outputs`."""
    return [(name, torch.int64, (B, O if w is None else w)) for name, w in _REFER_OUT]


def boxes_work_list(sizes: np.ndarray, chunk: int = BOXES_CHUNK) -> np.ndarray:
    """(n_work, 3) int64 {object, first point, count <= chunk}: every object's CSR segment cut into bounded chunks, so
    that one launch is balanced whatever the largest object is (a floor has several hundred thousand points)."""
    sizes = np.asarray(sizes, dtype=np.int64)
    off = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(sizes, out=off[1:])
    n_chunks = (sizes + chunk - 1) // chunk
    obj = np.repeat(np.arange(len(sizes), dtype=np.int64), n_chunks)
    start = np.zeros(len(sizes) + 1, dtype=np.int64)
    np.cumsum(n_chunks, out=start[1:])
    k = np.arange(obj.shape[0], dtype=np.int64) - start[obj]
    work = np.empty((obj.shape[0], 3), dtype=np.int64)
    work[:, 0] = obj
    work[:, 1] = off[obj] + k * chunk
    work[:, 2] = np.minimum(sizes[obj] - k * chunk, chunk)
    return work


def obj_boxes(packed: PackedScans) -> torch.Tensor:
    """convert_pc_to_box (data/data_utils.py:63-72) of every packed object, annotated and proposal, in one pass:
    (n_objects, 6) float64 [centre, size], bit-equal to numpy on the loader's float64 rows.  finalize() calls it once
    and keeps the result as `packed.boxes`."""
    dev = _obj_device(packed, "obj_boxes")
    n = packed.n_objects
    boxes = torch.empty((n, 6), dtype=torch.float64, device=dev)
    if n == 0:
        return boxes
    work = torch.from_numpy(boxes_work_list(packed.sizes_host)).to(dev)
    ws = torch.empty(n * 6, dtype=torch.int32, device=dev)
    launch("gps_obj_boxes", n, int(packed.xyz.shape[0]), int(work.shape[0]), packed.xyz, int(packed.rgb is None), work, ws, boxes,
           device=dev)
    return boxes


def proposal_labels(packed: PackedScans) -> torch.Tensor:
    """(n_objects,) int32: an annotated object's own label; a proposal's label after the relabelling of base.py:353-366
    -- the label of the first annotated object of its scan whose box overlaps it by IoU >= 0.25, else its own.  It depends
    on the scan only, so finalize() computes it once (one launch over all proposals) and keeps it as
    `packed.match_labels`: what `select_rows(pc_type="pred")` reads, bit-equal to `refer_targets(..., "pred")`'s
    obj_labels for every proposal."""
    dev = _obj_device(packed, "proposal_labels")
    match = packed.labels.clone()
    ids, ann = [], []
    for sid, props in packed._scan_props.items():
        objs = packed._scan_objs[sid]
        ids.extend(props)
        ann.extend([[objs.start, objs.stop]] * len(props))
    if ids:
        prop_id = torch.from_numpy(np.asarray(ids, dtype=np.int32)).to(dev)
        ann_range = torch.from_numpy(np.asarray(ann, dtype=np.int32).reshape(-1, 2)).to(dev)
        launch("gps_proposal_labels", len(ids), packed.n_objects, packed.boxes, packed.labels, prop_id, ann_range, match,
               device=dev)
    return match


def refer_targets(packed: PackedScans, row_obj: torch.Tensor, tgt_obj, scan_ids: Sequence[str], pc_type: str = "pred",
                  out: Optional[dict] = None) -> dict:
    """The targets ScanBase._getitem_refer derives from box IoU (base.py:348-417, :453-454, :478-483) in the layouts the
    dataset wrapper hands to the model (dataset_wrapper.py:164-191), for a whole batch in one launch and without a host
    sync: tgt_object_id_iou25 / tgt_object_id_iou50 (B,O) int64, tgt_object_id (B,1) int64, obj_labels (B,O) int64 with
    -100 in the padding slots.

    row_obj (B,O) int32: batch_rows(..., proposals=True) for pc_type 'pred', batch_rows(...) for 'gt'.
    tgt_obj: per item the position of the referred object among its scan's annotated objects (`obj_ids.index(
    tgt_object_instance)`, base.py:398), a sequence or a tensor on any device.  scan_ids: the items' scans, or their
    `scan_ranges(packed, scan_ids)` table made ahead of the call (no upload inside a captured region then).
    out: optional dict of preallocated contiguous tensors of those four names, shapes and dtypes, written IN PLACE.
    The reference's flag vectors have n_b + 1 entries, so a scene that fills all O slots cannot be padded there
    (pad_tensors asserts); a row table on the host is checked for that here (ValueError), one on the device is not.
    Integer-stored colours: bit-equal flags; float32-stored colours: the float64 form still (the reference's float32
    boxes are no parity target).  `is_multiple` / `is_hard` are dictionary look-ups of the caller, or `select_rows`'."""
    need_finalized(packed.xyz, "PackedScans")
    if pc_type not in ("pred", "gt"):
        raise ValueError(f"refer_targets: pc_type {pc_type!r} is neither 'pred' nor 'gt'")
    B, O = row_obj.shape
    if len(scan_ids) != B:
        raise ValueError(f"refer_targets: {len(scan_ids)} scan ids for {B} rows")
    if O > REFER_MAX_OBJ:
        raise ValueError(f"refer_targets: {O} object slots > {REFER_MAX_OBJ}")
    if row_obj.device.type == "cpu" and B and bool((row_obj[:, -1] >= 0).any()):
        raise ValueError("refer_targets: a scene fills all object slots; the targets need max_obj_len >= n_objects + 1")
    dev = packed.xyz.device
    need_gpu(dev, "refer_targets", "scenes")
    row_obj = row_obj.to(device=dev, dtype=torch.int32).contiguous()
    ranges = scan_ranges(packed, scan_ids)
    tgt = torch.as_tensor(tgt_obj).reshape(B).to(device=dev, dtype=torch.int32) + ranges[:, 0]
    res = outputs("refer_targets", _refer_spec(B, O), out, dev, "scans")
    launch("gps_refer_targets", B, O, packed.n_objects, int(pc_type == "gt"), packed.boxes, packed.labels, row_obj, tgt, ranges,
           res["tgt_object_id_iou25"], res["tgt_object_id_iou50"], res["tgt_object_id"], res["obj_labels"], device=dev)
    return res


# ---- the augmented path: ScanBase._obj_processing_aug + DataAugmentor ---------------------------------
AUG_STRIDE = 48                                  # GPS_OBJ_AUG_STRIDE of include/gps_hip.h, and the offsets of its comment
AUG_FLIP, AUG_SCALE, AUG_SCENE_TRANS, AUG_SCENE_ROT, AUG_RGB, AUG_OBJ_TRANS, AUG_OBJ_ROT, AUG_JITTER = (
    1, 2, 4, 8, 16, 32, 64, 128)
# (AugParams field, presence bit, first double of the entry, doubles) of the per-scene knobs
_AUG_SCENE = (("scene_flip", AUG_FLIP, 14, 9), ("scene_scale", AUG_SCALE, 1, 1), ("scene_trans", AUG_SCENE_TRANS, 5, 3),
              ("scene_rot", AUG_SCENE_ROT, 23, 9), ("rgb_delta", AUG_RGB, 11, 3), ("obj_jitter", AUG_JITTER, 2, 3))
_AUG_OBJ_TRANS_AT, _AUG_OBJ_ROT_AT = 8, 32


@dataclass
class AugParams:
    """One batch's draws of DataAugmentor (the `aug_dict` of data_augmentor.py:218-223, per scene).  Every field is
    a length-B list (or None = absent for the whole batch); an entry None means "not applied" to that scene.

    scene_flip / scene_rot: (3,3) float64, applied as x @ M.  scene_scale: float.  scene_trans / rgb_delta: (3,).
    obj_trans / obj_rot: per scene a length-O list over the object SLOTS of `row_obj` (None = that object keeps
    its place) of (3,) / (3,3).  obj_jitter: the jitter scale, a float or (3,).  pts_shuffle: bool per scene -- kept
    for the record only: a permutation of the sample rows commutes with everything downstream, so it is realised by
    the order of the draws (device-drawn samples are in random order; a replay passes permuted sample_idx and
    jitter_noise), never by device work."""
    scene_flip: Optional[list] = None
    scene_scale: Optional[list] = None
    scene_trans: Optional[list] = None
    scene_rot: Optional[list] = None
    rgb_delta: Optional[list] = None
    obj_trans: Optional[list] = None
    obj_rot: Optional[list] = None
    obj_jitter: Optional[list] = None
    pts_shuffle: Optional[list] = None

    def _get(self, name: str, b: int):
        v = getattr(self, name)
        return None if v is None else v[b]

    def table(self, B: int, O: int):
        """-> (entries (n, AUG_STRIDE) float64, row_aug (B*O,) int32 with -1 = nothing applied).  A scene without
        per-object parameters is ONE entry shared by its O rows (the published configs: B entries per batch)."""
        entries, row_aug = [], np.full((B, O), -1, dtype=np.int32)
        for b in range(B):
            e, flags = np.zeros(AUG_STRIDE, dtype=np.float64), 0
            for name, bit, at, n in _AUG_SCENE:
                v = self._get(name, b)
                if v is not None:                 # a scalar jitter scale serves all three coordinates
                    e[at:at + n] = np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (n,))
                    flags |= bit
            ot, orot = self._get("obj_trans", b), self._get("obj_rot", b)
            per_obj = any(x is not None for x in (ot or [])) or any(x is not None for x in (orot or []))
            if not per_obj:
                if flags:
                    e[0] = flags
                    row_aug[b, :] = len(entries)
                    entries.append(e)
                continue
            for o in range(O):
                eo, fo = e.copy(), flags
                if ot is not None and o < len(ot) and ot[o] is not None:
                    eo[_AUG_OBJ_TRANS_AT:_AUG_OBJ_TRANS_AT + 3] = np.asarray(ot[o], dtype=np.float64).reshape(3)
                    fo |= AUG_OBJ_TRANS
                if orot is not None and o < len(orot) and orot[o] is not None:
                    eo[_AUG_OBJ_ROT_AT:_AUG_OBJ_ROT_AT + 9] = np.asarray(orot[o], dtype=np.float64).reshape(9)
                    fo |= AUG_OBJ_ROT
                if fo:
                    eo[0] = fo
                    row_aug[b, o] = len(entries)
                    entries.append(eo)
        tab = np.stack(entries, 0) if entries else np.zeros((0, AUG_STRIDE), dtype=np.float64)
        return tab, row_aug.reshape(-1)

    def to_device(self, B: int, O: int, dev) -> "AugTable":
        tab, row_aug = self.table(B, O)
        return AugTable(torch.from_numpy(tab).to(dev), torch.from_numpy(row_aug).to(dev),
                        bool((tab[:, 0].astype(np.int64) & AUG_SCALE).any()))


@dataclass
class AugTable:
    """AugParams.table() on the device: what the launch reads.  Build it ahead of the step (AugParams.to_device) to
    keep the upload out of a captured or timed region."""
    entries: torch.Tensor                        # (n, AUG_STRIDE) float64
    row_aug: torch.Tensor                        # (B*O,) int32, -1 = nothing applied
    has_scale: bool                              # some entry scales: those rows read all points of their object


def obj_processing_aug(packed: PackedScans, row_obj: torch.Tensor, num_points: int = 1024,
                       aug: "Optional[AugParams | AugTable]" = None, sample_idx: Optional[torch.Tensor] = None,
                       jitter_noise: Optional[torch.Tensor] = None, seed: int = 0, need_boxes: bool = False,
                       out: Optional[dict] = None, seed_dev: Optional[torch.Tensor] = None) -> dict:
    """ScanBase._obj_processing_aug (base.py:742-776) after DataAugmentor.update_data_dict (data_augmentor.py:156-215)
    for a whole batch in one launch; same return dict and the same in-place `out=` contract as obj_processing_post
    (so it fills `GPSTrainStep.static_inputs()` just the same).

    aug: the batch's AugParams (`draw_aug_params`) or their AugTable already on the device, or None = nothing applied -- the reference's validation path under
    a `data_aug` config (an empty augmentor queue still takes this branch: subsample, sizes / centres from the sample,
    max_dist clamped at 1e-6).
    sample_idx (B,O,num_points) int32 / jitter_noise (B,O,num_points,3) float32 or float64: the reference's
    np.random.choice / np.random.randn draws for a replay -- already in the order the point shuffle left them; None =
    drawn on the device from `seed` (the noise only for scenes whose obj_jitter is set).
    seed_dev: one int64 word on the scans' device, as in obj_processing_post: samples and noise are drawn from
    seed + *seed_dev (gps_obj_processing_aug_sw); None = `seed`."""
    dev = _obj_device(packed, "obj_processing_aug")
    B, O = row_obj.shape
    n_rows = B * O
    if isinstance(aug, AugParams):
        aug = aug.to_device(B, O, dev)
    tab, row_aug, scaled = (aug.entries, aug.row_aug, aug.has_scale) if aug is not None else (None, None, False)
    if tab is not None and (tab.shape[0] == 0 or row_aug.shape[0] != n_rows):
        if tab.shape[0]:
            raise ValueError(f"obj_processing_aug: the parameter table indexes {row_aug.shape[0]} rows, the batch has {n_rows}")
        tab = row_aug = None
    nbytes = _algorithmic_bytes(packed, row_obj if row_obj.device.type == "cpu" else None, n_rows, num_points,
                                stream_all=scaled)
    row_obj, sample_idx, res = _obj_buffers("obj_processing_aug", row_obj, num_points, sample_idx, need_boxes, out, dev)
    if jitter_noise is not None:
        if jitter_noise.dtype not in (torch.float32, torch.float64):
            raise ValueError("obj_processing_aug: jitter_noise must be float32 or float64")
        jitter_noise = jitter_noise.to(device=dev).contiguous()
        assert jitter_noise.shape == (B, O, num_points, 3), jitter_noise.shape
    seed_word("obj_processing_aug", seed_dev, dev, "scans")
    word = () if seed_dev is None else (seed_dev,)
    launch("gps_obj_processing_aug" + ("_sw" if word else ""), n_rows, num_points, packed.xyz, packed.rgb,
           int(packed.rgb is None or packed.rgb.dtype == torch.uint8), packed.obj_offsets, row_obj, sample_idx, jitter_noise,
           int(jitter_noise is not None and jitter_noise.dtype == torch.float64), u64(seed), *word,
           tab, row_aug, tab.shape[0] if tab is not None else 0, res["obj_fts"], res["obj_locs"], res.get("obj_boxes"),
           res["obj_masks"], device=dev, label=f"obj_processing_aug(rows={n_rows},P={num_points})", nbytes=nbytes,
           what="obj_processing_aug")
    return as_bool(res, ("obj_masks",))


def _check_key(key) -> bool:
    """DataAugmentor.check_key (data_augmentor.py:225-238): absent -> off, a bool is itself, a mapping is its
    `enabled` (default on), anything else is on."""
    if key is None:
        return False
    if isinstance(key, bool):
        return key
    if isinstance(key, Mapping):
        return bool(key.get("enabled", True))
    return True


def _check_p(key, rng: np.random.Generator) -> bool:
    """DataAugmentor.check_p (data_augmentor.py:241-242): a mapping with a `p` fires with that probability, and the
    draw is consumed only then.  (The reference tests `isinstance(key, dict)`, so a config node that is not a dict
    subclass always fires there; every `p` of an enabled knob in the published configs is 1.0.)"""
    return (not isinstance(key, Mapping)) or ("p" not in key) or bool(rng.random() < key["p"])


_R_ANGLES = (0.0, math.pi / 2, math.pi, math.pi * 3 / 2)


def _draw_rotation(cfg, rng: np.random.Generator) -> np.ndarray:
    """data_augmentor.py:69-93 / :120-144: axis-aligned or uniform angles times `value`, the reference's rx, ry, rz
    (its rz is the transpose of build_rotate_mat's), optionally multiplied in a shuffled order."""
    if cfg["axis_align"]:
        th = [_R_ANGLES[int(rng.integers(4))] * cfg["value"][i] for i in range(3)]
    else:
        th = [(rng.random() * 2 * math.pi - math.pi) * cfg["value"][i] for i in range(3)]
    rx = np.array([[1, 0, 0], [0, math.cos(th[0]), -math.sin(th[0])], [0, math.sin(th[0]), math.cos(th[0])]])
    ry = np.array([[math.cos(th[1]), 0, math.sin(th[1])], [0, 1, 0], [-math.sin(th[1]), 0, math.cos(th[1])]])
    rz = np.array([[math.cos(th[2]), math.sin(th[2]), 0], [-math.sin(th[2]), math.cos(th[2]), 0], [0, 0, 1]])
    mats = [rx, ry, rz]
    if cfg.get("shuffle", False):
        mats = [mats[i] for i in rng.permutation(3)]
    return mats[0].dot(mats[1]).dot(mats[2])


def _draw_translation(cfg, rng: np.random.Generator) -> np.ndarray:
    return np.array([rng.standard_normal() * cfg["value"][i] for i in range(3)])


def draw_aug_params(aug_cfg, split: str, B: int, O: int, rng: np.random.Generator) -> AugParams:
    """One batch's draws under the reference's `data_aug` schema (any mapping: a dict, an OmegaConf node), with the laws
    of DataAugmentor.scene_aug / obj_aug (data_augmentor.py:39-154) on `rng`; the reference's global-RNG stream is
    not reproduced.  Only the augmentors named in `aug_list` run, and none at all on a split other than 'train'.
    Like the reference, `random_jitter.p` and `accord_to_size` are not read, and `order_shuffle` is not drawn (it
    only fills obj_order, which _obj_processing_aug never reads)."""
    a = AugParams()
    if aug_cfg is None or split != "train":
        return a
    for name in aug_cfg["aug_list"]:
        if name not in aug_cfg:
            continue
        cfg = aug_cfg[name]
        if name == "scene_aug":
            a.scene_trans, a.scene_scale, a.scene_flip = [None] * B, [None] * B, [None] * B
            a.scene_rot, a.rgb_delta = [None] * B, [None] * B
            for b in range(B):
                c = cfg.get("translation")
                if _check_key(c) and _check_p(c, rng):
                    a.scene_trans[b] = _draw_translation(c, rng)
                c = cfg.get("scaling")
                if _check_key(c) and _check_p(c, rng):
                    a.scene_scale[b] = rng.random() * (c["value"][1] - c["value"][0]) + c["value"][0]
                c = cfg.get("flip")
                if _check_key(c) and _check_p(c, rng):
                    m, kind = np.eye(3), int(rng.integers(4))     # x, y, x + y, or none at all
                    if kind in (0, 2):
                        m[0][0] *= -1
                    if kind in (1, 2):
                        m[1][1] *= -1
                    a.scene_flip[b] = m
                c = cfg.get("rotation")
                if _check_key(c) and _check_p(c, rng):
                    a.scene_rot[b] = _draw_rotation(c, rng)
                if _check_key(cfg.get("color_jitter")):
                    a.rgb_delta[b] = rng.standard_normal(3) * 0.1
        elif name == "obj_aug":
            a.obj_trans, a.obj_rot = [[None] * O for _ in range(B)], [[None] * O for _ in range(B)]
            for b in range(B):
                for o in range(O):
                    c = cfg.get("translation")
                    if _check_key(c) and _check_p(c, rng):
                        a.obj_trans[b][o] = _draw_translation(c, rng)
                    c = cfg.get("rotation")
                    if _check_key(c) and _check_p(c, rng):
                        a.obj_rot[b][o] = _draw_rotation(c, rng)
            if _check_key(cfg.get("random_jitter")):
                a.obj_jitter = [cfg["random_jitter"]["value"]] * B
            if _check_key(cfg.get("pts_shuffle")):
                a.pts_shuffle = [True] * B
        else:
            raise ValueError(f"draw_aug_params: unknown augmentor {name!r} in aug_list")
    return a


def _knob(key, n_values: int = 3):
    """One knob of the `data_aug:` schema as the plain numbers of struct gps_aug_knob: enabled by `_check_key`, p = 1.0
    where the config gives none (check_p always fires then), the first n_values of `value`."""
    k = _native.AugKnob()
    k.enabled = int(_check_key(key))
    k.p = 1.0
    if k.enabled and isinstance(key, Mapping):
        k.p = float(key.get("p", 1.0))
        if not 0.0 <= k.p <= 1.0:
            raise ValueError(f"draw_aug_table: p = {k.p} outside [0, 1]")
        k.axis_align, k.shuffle = int(bool(key.get("axis_align", False))), int(bool(key.get("shuffle", False)))
        for i in range(n_values):
            k.value[i] = float(key["value"][i])
    return k


def aug_draw_args(aug_cfg, B: int, O: int, seed: int = 0, seed_dev: Optional[torch.Tensor] = None):
    """The `data_aug:` block (any mapping) as struct gps_aug_draw_args -> (args, per_obj, has_scale): per_obj = some
    per-object knob is on (the table then has B * O entries, else B), has_scale = the scaling knob is on."""
    a = _native.AugDrawArgs()
    a.mode, a.B, a.O, a.seed = _native.AUG_DRAW_TABLE, int(B), int(O), u64(seed)
    a.seed_dev = None if seed_dev is None else seed_dev.data_ptr()
    for name in aug_cfg["aug_list"]:
        if name not in aug_cfg:
            continue
        cfg = aug_cfg[name]
        if name == "scene_aug":
            a.scene_on = 1
            a.scene_trans, a.scene_scale = _knob(cfg.get("translation")), _knob(cfg.get("scaling"), 2)
            a.scene_flip, a.scene_rot = _knob(cfg.get("flip"), 0), _knob(cfg.get("rotation"))
            a.color_jitter = int(_check_key(cfg.get("color_jitter")))
        elif name == "obj_aug":
            a.obj_on = 1
            a.obj_trans, a.obj_rot = _knob(cfg.get("translation")), _knob(cfg.get("rotation"))
            a.jitter_on = int(_check_key(cfg.get("random_jitter")))
            if a.jitter_on:
                v = np.broadcast_to(np.asarray(cfg["random_jitter"]["value"], dtype=np.float64).reshape(-1), (3,))
                a.jitter_value[0], a.jitter_value[1], a.jitter_value[2] = (float(x) for x in v)
        else:
            raise ValueError(f"draw_aug_table: unknown augmentor {name!r} in aug_list")
    per_obj = bool(a.obj_on and (a.obj_trans.enabled or a.obj_rot.enabled))
    return a, per_obj, bool(a.scene_on and a.scene_scale.enabled)


def draw_aug_table(aug_cfg, split: str, B: int, O: int, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
                   out: Optional[dict] = None, device=None) -> "Optional[AugTable]":
    """`draw_aug_params` + `AugParams.to_device` as ONE launch (gps_aug_draw) and without a host loop, a host table or an
    upload: the AugTable `obj_processing_aug` takes, drawn on the device from seed + *seed_dev by the law of
    include/gps_hip.h (stream seed + 6; seed_dev: one int64 word on the device, advanced there between graph replays).
    None -- nothing launched -- without a config and on a split other than 'train', like `draw_aug_params`.
    The table's shape follows from the config alone: B entries, or B * O when a per-object knob is on; `has_scale` comes
    from the config too.  out: optional {"entries" (n, AUG_STRIDE) float64, "row_aug" (B*O,) int32}, written IN PLACE.
    device: where to draw, default the seed word's, else the current GPU.  The draws differ from `draw_aug_params`'
    (another generator); that function stays the host and replay path."""
    if aug_cfg is None or split != "train":
        return None
    args, per_obj, has_scale = aug_draw_args(aug_cfg, B, O, seed, seed_dev)
    dev = _draw_device("draw_aug_table", seed_dev, out, device)
    res = outputs("draw_aug_table", (("entries", torch.float64, (B * O if per_obj else B, AUG_STRIDE)),
                                     ("row_aug", torch.int32, (B * O,))), out, dev, "scans")
    launch("gps_aug_draw", ctypes.byref(args), res["entries"], res["row_aug"], None, None, device=dev,
           label=f"aug_draw(B={B},O={O})", nbytes=res["entries"].numel() * 8 + 4 * B * O, what="draw_aug_table")
    return AugTable(res["entries"], res["row_aug"], has_scale)


def draw_rot_table(split: str, rot_aug: bool, B: int, O: int, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
                   out: Optional[dict] = None, device=None):
    """build_rotate_mat (data/data_utils.py:163-178, rand_angle 'axis') for a whole batch in one launch: the pair
    (mats (B,3,3) f32, row_rot (B*O,) int32) `obj_processing_post(rot=...)` passes through, drawn on the device from
    seed + *seed_dev (stream seed + 7 of include/gps_hip.h).  None -- nothing launched -- on a split other than 'train'
    or with rot_aug off, where build_rotate_mat returns None for every scene.
    out: optional {"rot" (B,3,3) float32, "row_rot" (B*O,) int32}, written IN PLACE."""
    if split != "train" or not rot_aug:
        return None
    a = _native.AugDrawArgs()
    a.mode, a.B, a.O, a.seed = _native.AUG_DRAW_ROT, int(B), int(O), u64(seed)
    a.seed_dev = None if seed_dev is None else seed_dev.data_ptr()
    dev = _draw_device("draw_rot_table", seed_dev, out, device)
    res = outputs("draw_rot_table", (("rot", torch.float32, (B, 3, 3)), ("row_rot", torch.int32, (B * O,))), out, dev, "scans")
    launch("gps_aug_draw", ctypes.byref(a), None, None, res["rot"], res["row_rot"], device=dev,
           label=f"rot_draw(B={B},O={O})", nbytes=36 * B + 4 * B * O, what="draw_rot_table")
    return res["rot"], res["row_rot"]


def _draw_device(what: str, seed_dev, out, device) -> torch.device:
    """Where a draw runs: `device`, else the seed word's, else the out buffers', else the current GPU."""
    if device is not None:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
    elif seed_dev is not None:
        dev = seed_dev.device
    elif out:
        dev = next(iter(out.values())).device
    else:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
    need_gpu(dev, what, "tables")
    seed_word(what, seed_dev, dev, "tables")
    return dev


def rot_rows(rot, B: int, O: int, dev):
    """Per-scene rotations -> (matrices (n,3,3) f32 on dev, row_rot (B*O) int32 with -1 = unrotated).
    `rot` is a (B,3,3) tensor/array, or a list with None for scenes build_rotate_mat left unrotated."""
    mats, row_rot = [], np.full((B, O), -1, dtype=np.int32)
    for b in range(B):
        r = rot[b]
        if r is None:
            continue
        row_rot[b, :] = len(mats)
        mats.append(np.asarray(r.cpu() if torch.is_tensor(r) else r, dtype=np.float32).reshape(3, 3))
    if not mats:
        mats = [np.eye(3, dtype=np.float32)]
    return (torch.from_numpy(np.stack(mats, 0)).to(dev).contiguous(),
            torch.from_numpy(row_rot.reshape(-1)).to(dev))


def _algorithmic_bytes(packed: PackedScans, row_obj_host, n_rows: int, num_points: int, stream_all: bool = True) -> int:
    """Each object's raw points read once (16-byte records; 15 or 24 B/point as two arrays) + the sampled
    points gathered + the f32 feature rows written.  With the row table already on the device the object
    sizes of THIS batch are not known on the host without a sync: the mean object size stands in.
    stream_all=False: the augmented path without scaling, which reads the gathered records only."""
    per_pt = 16 if packed.rgb is None else 12 + 3 * packed.rgb.element_size()
    if not stream_all:
        k_total = 0
    elif row_obj_host is not None:
        ids = row_obj_host.reshape(-1).numpy()
        k_total = int(packed.sizes_host[ids[ids >= 0]].sum())
    else:
        k_total = int(packed.sizes_host.mean() * n_rows) if packed.n_objects else 0
    return k_total * per_pt + n_rows * num_points * (per_pt + 24) + n_rows * (4 + 24 + 1)
