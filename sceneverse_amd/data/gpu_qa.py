"""HBM-resident questions + the ScanQA / SQA3D loaders' per-sample selection as ONE launch of libgps_hip.so.

Reference (what this replaces on the data-loader workers, per sample):
    ScanNetScanQAOld.__getitem__  data/datasets/scannet_old.py:326-484  filter, target list ('gt', or 'pred' by IoU >= 0.25),
                                                                        crop with ALL targets first, the three multi-hots
    ScanNetSQA3D.__getitem__      data/datasets/scannet_old.py:94-232   the same + random.choice of a situation, sqa_type

MI355X form: the questions are uploaded ONCE (`PackedQuestions`, the twin of `gpu_objects.PackedScans` and
`gpu_text.PackedTexts`): per question its scan's object ranges, a CSR of target objects with their labels, a CSR of
answer ids, the question type and a CSR of text ids (one per situation variant).  A batch is then ONE integer per row --
the question's number -- and `qa_rows` turns it into the row table `obj_processing_post` takes, the text ids
`text_batch(mask=False)` takes, and `tgt_object_id / tgt_object_label / answer_label / sqa_type` on the device.  The rule
is stated in include/gps_hip.h (gps_obj_select_qa); tests/qa_rows_cases.py restates it.  GPU only: there is no CPU path
here (the reference's own loader IS the CPU path).
"""
from __future__ import annotations

import ctypes
from typing import List, Optional, Sequence

import numpy as np
import torch

from .. import _native
from .._launch import launch
from ._resident import need_finalized, need_gpu, outputs, seed_word, u64
from .gpu_objects import OBJ_SELECT_MAX_SCAN, REFER_MAX_OBJ, PackedScans

QA_MAX_TGT = _native.QA_MAX_TGT                  # GPS_QA_MAX_TGT of include/gps_hip.h
N_LABELS_607 = 607                               # sem_type '607' (scannet_old.py:462-463)


class PackedQuestions:
    """The questions of a split resident on the scans' device.  Build with add_question(...) x n, then
    finalize(packed_scans)."""

    def __init__(self, device: torch.device | str = "cuda"):
        self.device = torch.device(device)
        self._scan: List[str] = []
        self._tgt: List[List[int]] = []
        self._tgt_label: List[Optional[List[int]]] = []
        self._ans: List[List[int]] = []
        self._type: List[int] = []
        self._texts: List[List[int]] = []
        self.ann_range = self.prop_range = self.tgt_first = self.tgt_id = self.tgt_label = None
        self.ans_first = self.ans_id = self.sqa_type = self.var_first = self.var_text = None
        self.n_var_host: Optional[np.ndarray] = None
        self.n_sel_host: Optional[np.ndarray] = None   # (nq, 2) positions of the annotated / the proposal range
        self.has_props_host: Optional[np.ndarray] = None

    def add_question(self, scan_id: str, targets: Sequence[int] = (), answers: Sequence[int] = (), texts=0,
                     tgt_labels: Optional[Sequence[int]] = None, sqa_type: int = 0) -> int:
        """scan_id: the question's scan.  targets: the positions of its target objects among the scan's ANNOTATED objects
        (`obj_ids.index(object_id)`; the reference's `object_ids`), none to GPS_QA_MAX_TGT of them.  tgt_labels: per
        target the reference's `cat2int[object_name]` (read in 'pred' mode, scannet_old.py:421), None = the object's own
        label.  answers: answer ids in the caller's vocabulary; ids < 0 are dropped, as `stoi(answer) >= 0` does
        (scannet_old.py:341-342; SQA3DAnswer.stoi never returns one).  sqa_type: get_sqa_question_type, 0 .. 5.
        texts: one text id of a PackedTexts or several -- the strings `situation_i + question`, tokenised whole by the
        caller; the first is the evaluation variant.  -> the question's number, what a batch refers to it by."""
        assert self.ann_range is None, "finalize() was already called"
        targets = [int(t) for t in targets]
        if len(targets) > QA_MAX_TGT:
            raise ValueError(f"add_question: {len(targets)} targets > {QA_MAX_TGT}")
        if tgt_labels is not None and len(tgt_labels) != len(targets):
            raise ValueError("add_question: tgt_labels must give one label per target")
        texts = [int(texts)] if np.isscalar(texts) else [int(t) for t in texts]
        if not texts or min(texts) < 0:
            raise ValueError("add_question: a question needs at least one text id, none negative")
        if not 0 <= int(sqa_type) <= 5:
            raise ValueError("add_question: sqa_type must lie in 0 .. 5")
        self._scan.append(scan_id)
        self._tgt.append(targets)
        self._tgt_label.append(None if tgt_labels is None else [int(l) for l in tgt_labels])
        self._ans.append([int(a) for a in answers if int(a) >= 0])
        self._type.append(int(sqa_type))
        self._texts.append(texts)
        return len(self._scan) - 1

    def finalize(self, packed: PackedScans) -> "PackedQuestions":
        """The device tables of gps_qa_questions.  packed: the finalized scans the questions are about (their ranges and
        labels are read here, on the host); a target position outside its scan is refused (ValueError)."""
        need_finalized(packed.xyz, "PackedScans")
        nq = len(self._scan)
        ann, prop = np.zeros((nq, 2), np.int32), np.zeros((nq, 2), np.int32)
        has = np.zeros(nq, bool)
        tgt_id, tgt_label = [], []
        for i, sid in enumerate(self._scan):
            objs = packed.scan_objects(sid)
            ann[i] = (objs.start, objs.stop)
            if sid in packed._scan_props:
                props = packed.scan_proposals(sid)
                prop[i], has[i] = (props.start, props.stop), True
            for j, t in enumerate(self._tgt[i]):
                if not 0 <= t < len(objs):
                    raise ValueError(f"PackedQuestions: question {i} has a target position {t} outside scan {sid!r}")
                tgt_id.append(objs.start + t)
                tgt_label.append(packed._labels[objs.start + t] if self._tgt_label[i] is None else self._tgt_label[i][j])

        def csr(lists):
            first = np.zeros(nq + 1, np.int64)
            np.cumsum([len(l) for l in lists], out=first[1:])
            return first.astype(np.int32)

        def up(a):
            return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(self.device)

        self.ann_range, self.prop_range = up(ann), up(prop)
        self.tgt_first, self.tgt_id, self.tgt_label = up(csr(self._tgt)), up(tgt_id), up(tgt_label)
        self.ans_first, self.ans_id = up(csr(self._ans)), up([a for l in self._ans for a in l])
        self.sqa_type = up(self._type)
        self.var_first, self.var_text = up(csr(self._texts)), up([t for l in self._texts for t in l])
        self.n_var_host = np.asarray([len(l) for l in self._texts], dtype=np.int64)
        self.n_sel_host = np.stack([ann[:, 1] - ann[:, 0], prop[:, 1] - prop[:, 0]], 1).astype(np.int64)
        self.has_props_host = has
        return self

    @property
    def n_questions(self) -> int:
        return len(self._scan)

    @property
    def n_variants(self) -> int:
        """All questions' variants; variant v of the whole table is text `var_text[v]` (a per-variant keep table has one
        row per v)."""
        return 0 if self.n_var_host is None else int(self.n_var_host.sum())

    def table(self) -> "_native.QAQuestions":
        z = lambda t: t.data_ptr() if t.numel() else None     # noqa: E731
        return _native.QAQuestions(self.n_questions, int(self.tgt_id.numel()), int(self.ans_id.numel()),
                                   int(self.var_text.numel()), z(self.ann_range), z(self.prop_range),
                                   self.tgt_first.data_ptr(), z(self.tgt_id), z(self.tgt_label), self.ans_first.data_ptr(),
                                   z(self.ans_id), z(self.sqa_type), self.var_first.data_ptr(), z(self.var_text))


def _ints(name: str, x, B: int) -> torch.Tensor:
    t = x if torch.is_tensor(x) else torch.as_tensor(np.asarray(x))
    t = t.reshape(-1)
    if t.numel() == 0:
        t = t.to(torch.int32)
    if t.numel() != B or t.dtype.is_floating_point or t.dtype == torch.bool:
        raise ValueError(f"qa_rows: {name} must hold {B} integers")
    return t


def qa_rows(packed: PackedScans, questions: PackedQuestions, q_idx, max_keep: int, O: Optional[int] = None,
            n_answers: int = 8864, keep: Optional[torch.Tensor] = None, n_labels: Optional[int] = None,
            pc_type: str = "gt", matched: bool = True, train: bool = True, long: bool = False,
            order: Optional[torch.Tensor] = None, pick=None, seed: int = 0, seed_dev: Optional[torch.Tensor] = None,
            out: Optional[dict] = None) -> dict:
    """The ScanQA / SQA3D loaders' selection (scannet_old.py:326-484, :94-232) for a whole batch in one launch and without
    a host sync, from one question number per row; the rule and its four definitions are stated in include/gps_hip.h.

    -> dict: row_obj (B, O) int32 global object ids, -1 = padding -- the table `obj_processing_post(..., need_boxes=True)`
    takes; n_sel, n_rem, n_tgt (B) int32: objects in the row, how many the random fill chose from (0 = no fill), targets
    in the row; sent_idx (B) int32: the text id of the row's variant, what `text_batch(..., mask=False)` takes; sqa_type
    (B) int64; obj_labels (B, O) int64, the loaders' obj_labels, -100 = padding; tgt_object_id (B, O), tgt_object_label (B, n_labels), answer_label (B, n_answers): multi-hot, float32
    (ScanQA's `.float()`) or, long=True, int64 (SQA3D's `.long()`).

    q_idx: (B) question numbers (`add_question`'s), a sequence or a tensor on any device.  max_keep: objects a row may
    hold, the loaders' `max_obj_len - 1`; O: slots per row, default max_keep + 1 (what ScanFamilyDatasetWrapperOld pads
    to; tgt_object_id keeps its pad slot).  keep: `keep_table(...)`, (n_labels,), or per VARIANT (questions.n_variants,
    n_labels) for `filter_lang` -- row v keeps label l iff the table does and `int2cat[l] in text_v`; required for
    pc_type 'gt', not read for 'pred'.  n_labels: width of tgt_object_label, default keep's, else 607.
    pc_type 'pred': rows of the scans' proposals (`add_proposals`), targets by IoU >= 0.25.  matched: class comparisons
    read `packed.match_labels` (ScanQA relabels its proposals) or the raw labels (False: SQA3D).
    train: the variant is drawn (SQA3D's random.choice); False: the first.  pick: (B) a replay of that choice.
    order: (B, R >= max_keep) int32, per row what `random.shuffle` made of `list(range(n_rem))`; None = drawn on the
    device from seed + *seed_dev (stream seed + 3, the fill of `select_rows`; the pick is stream seed + 4, so `text_batch`
    shares the word).  out: optional dict of preallocated contiguous tensors under the names above, written IN PLACE.
    Refused here (ValueError): max_keep outside [1, O], O above 512, a question number, a pick or a scan size that
    arrives on the host and is out of range; in a device table such a row comes out empty."""
    need_finalized(packed.xyz, "PackedScans")
    need_finalized(questions.ann_range, "PackedQuestions")
    if pc_type not in ("gt", "pred"):
        raise ValueError(f"qa_rows: pc_type {pc_type!r} is neither 'gt' nor 'pred'")
    pred = pc_type == "pred"
    M = int(max_keep)
    O = M + 1 if O is None else int(O)
    A = int(n_answers)
    if M < 1 or M > O:
        raise ValueError(f"qa_rows: max_keep {M} must lie in [1, O = {O}]")
    if O > REFER_MAX_OBJ:
        raise ValueError(f"qa_rows: {O} object slots > {REFER_MAX_OBJ}")
    if A < 0:
        raise ValueError("qa_rows: n_answers must not be negative")
    if keep is None and not pred:
        raise ValueError("qa_rows: keep is required for pc_type='gt' (see keep_table)")
    q = torch.as_tensor(q_idx) if not torch.is_tensor(q_idx) else q_idx
    B = int(q.numel())
    q = _ints("q_idx", q, B)
    nq = questions.n_questions
    q_host = q.numpy() if q.device.type == "cpu" else None
    if q_host is not None and B:
        if int(q_host.min()) < 0 or int(q_host.max()) >= nq:
            raise ValueError(f"qa_rows: q_idx holds a question number outside [0, {nq})")
        if pred and not questions.has_props_host[q_host].all():
            raise ValueError("qa_rows: pc_type='pred' for a question whose scan has no proposals (add_proposals)")
        n_pos = questions.n_sel_host[q_host, 1 if pred else 0]
        if int(n_pos.max()) > OBJ_SELECT_MAX_SCAN:
            raise ValueError(f"qa_rows: a scan of {int(n_pos.max())} {'proposals' if pred else 'objects'} > {OBJ_SELECT_MAX_SCAN}")
    keep_rows = 0
    if keep is not None:
        if keep.dtype not in (torch.bool, torch.uint8) or keep.dim() not in (1, 2):
            raise ValueError("qa_rows: keep must be (n_labels,) or (n_variants, n_labels) bool / uint8")
        if keep.dim() == 2:
            keep_rows = int(keep.shape[0])
            if keep_rows != questions.n_variants:
                raise ValueError(f"qa_rows: a per-variant keep has {questions.n_variants} rows, one per variant")
        if n_labels is not None and int(n_labels) != int(keep.shape[-1]):
            raise ValueError("qa_rows: n_labels is the width of keep")
        n_labels = int(keep.shape[-1])
    n_labels = N_LABELS_607 if n_labels is None else int(n_labels)
    if n_labels < 0:
        raise ValueError("qa_rows: n_labels must not be negative")
    R = 0
    if order is not None:
        if order.dim() != 2 or order.shape[0] != B or order.shape[1] < M or order.dtype.is_floating_point:
            raise ValueError(f"qa_rows: order must be (B, R >= {M}) integers")
        R = int(order.shape[1])
    if pick is not None:
        pick = _ints("pick", pick, B)
        if q_host is not None and pick.device.type == "cpu" and B:
            pk = pick.numpy()
            if (pk < 0).any() or (pk >= questions.n_var_host[q_host]).any():
                raise ValueError("qa_rows: a pick outside its question's variants")
    dev = packed.xyz.device
    need_gpu(dev, "qa_rows", "scenes")
    if questions.ann_range.device != dev:
        raise ValueError("qa_rows: the questions must live on the scans' GPU")
    q = q.to(device=dev, dtype=torch.int32).contiguous()
    if keep is not None:
        keep = keep.to(dev).contiguous()
    if order is not None:
        order = order.to(device=dev, dtype=torch.int32).contiguous()
    if pick is not None:
        pick = pick.to(device=dev, dtype=torch.int32).contiguous()
    seed_word("qa_rows", seed_dev, dev, "scans")
    hot = torch.int64 if long else torch.float32
    spec = [("row_obj", torch.int32, (B, O)), ("n_sel", torch.int32, (B,)), ("n_rem", torch.int32, (B,)),
            ("n_tgt", torch.int32, (B,)), ("sent_idx", torch.int32, (B,)), ("sqa_type", torch.int64, (B,)),
            ("obj_labels", torch.int64, (B, O)), ("tgt_object_id", hot, (B, O)), ("tgt_object_label", hot, (B, n_labels)), ("answer_label", hot, (B, A))]
    res = outputs("qa_rows", spec, out, dev, "scans")
    flags = ((_native.QA_PRED if pred else 0) | (_native.QA_MATCHED if matched else 0) | (_native.QA_TRAIN if train else 0)
             | (_native.QA_INT64 if long else 0))
    table = questions.table()
    # every output written once + the question's tables + a label (and, 'pred', a box) per position (scans of some 256)
    nbytes = sum(t.numel() * t.element_size() for t in res.values()) + 64 * B + (52 if pred else 5) * B * 256
    launch("gps_obj_select_qa", B, O, M, A, packed.n_objects, n_labels, flags, ctypes.byref(table), q, packed.boxes,
           packed.labels, packed.match_labels, keep, keep_rows, order, R, pick, u64(seed), seed_dev,
           *[res[name] for name, _, _ in spec], device=dev, label=f"obj_select_qa(B={B},O={O},M={M},A={A})", nbytes=nbytes,
           what="qa_rows")
    return res
