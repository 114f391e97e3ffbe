"""Seeded inputs of the answer-accuracy checks (ScanQACounter, SQA3DCounter, gps_answer_hits), shared by
tests/golden/make_golden_answers.py (which runs the reference's evaluators on them) and the tests (which regenerate
them: they are not stored), and a pure-torch ORACLE of the ranking law of include/gps_hip.h:

    NaN above every number; then the value, descending, -0.0 == +0.0; among equals the lower column first

as a stable sort on the three keys (is-NaN, value, index) -- not "NaN -> +inf", which would tie NaN with +inf."""
import numpy as np
import torch

K = 10
SIZES = (16, 7, 33)                       # three batches of different B: the weighting of record() shows
V = {"scanqa": 8864, "sqa3d": 706}
N_TYPES = 6
N_OBJ, N_CLS = 5, 9
N_TOP = 12                                # planted best values per row, spaced so that bf16 keeps them distinct
SQA_KEYS = ("target_metric", "obj_cls_raw_acc", "ans1_acc", "ans10_acc") + tuple(f"type{t}_acc" for t in range(N_TYPES))
SCANQA_KEYS = ("ans1_acc", "ans10_acc", "obj_cls_raw_acc", "obj_cls_post_acc")


# ---- the law ----------------------------------------------------------------------------------------------------------
def ranked(scores: torch.Tensor) -> torch.Tensor:
    """(rows, V) float -> (rows, V) int64: every row's columns in rank order.  Two stable sorts, least significant key
    first: by value descending (NaN taken as 0 here, -0.0 == +0.0 compare equal, equal values keep index order), then by
    is-NaN (NaN first)."""
    x = scores.detach().float().cpu()
    nan = torch.isnan(x)
    v = torch.where(nan, torch.zeros_like(x), x)
    by_value = torch.sort(v, dim=1, descending=True, stable=True)[1]
    flag = torch.gather(nan, 1, by_value).to(torch.int8)
    by_nan = torch.sort(flag, dim=1, descending=True, stable=True)[1]
    return torch.gather(by_value, 1, by_nan)


def topk_ids(scores: torch.Tensor, k: int = K) -> torch.Tensor:
    """(rows, k) int32: the k best ids in rank order, -1 past V."""
    r = ranked(scores)[:, :k]
    out = torch.full((scores.shape[0], k), -1, dtype=torch.int32)
    out[:, :r.shape[1]] = r.to(torch.int32)
    return out


def words(scores, label, types=None, n_types=0, k=K, rows=None):
    """The 19 integer words gps_answer_hits adds for a batch: hit1, hitk, count, type_hit1[8], type_count[8]."""
    ids = topk_ids(scores, k).long()
    lab = label.detach().cpu()
    n = scores.shape[0] if rows is None else min(int(rows), scores.shape[0])
    w = [0] * 19
    for r in range(n):
        ones = [bool(lab[r, j] == 1) for j in ids[r].tolist() if j >= 0]
        h1 = ones[0]
        w[0] += int(h1)
        w[1] += int(any(ones))
        w[2] += 1
        if types is not None:
            t = int(types[r])
            if 0 <= t < n_types:
                w[3 + t] += int(h1)
                w[11 + t] += 1
    return w


def tie_free(scores: torch.Tensor, places: int = K + 1) -> torch.Tensor:
    """(rows,) bool: no two of the row's `places` best values are equal (a condition on the inputs alone)."""
    x = scores.detach().float().cpu()
    top = torch.gather(x, 1, ranked(x)[:, :places])
    return (top[:, 1:] != top[:, :-1]).all(dim=1) & ~torch.isnan(top).any(dim=1)


# ---- the batches --------------------------------------------------------------------------------------------------------
def batch(task: str, i: int) -> dict:
    """Batch i (B = SIZES[i]) of `task`: fp32 continuous scores whose N_TOP best values per row sit at random columns,
    at least 0.09 apart in [4, 5.5) (so they stay distinct on the bf16 grid, spacing 2^-5 there) above a N(0,1) floor cut
    at 3.5; multi-hot labels by row kind (row % 4): the best answer / one of places 2..10 and place 41 / a place past
    10 only / unanswerable; for sqa3d question types where type 4 never occurs and type 3 is absent from batch 1 only."""
    B, Vt = SIZES[i], V[task]
    g = torch.Generator().manual_seed(1000 * (1 + sorted(V).index(task)) + i)
    scores = torch.randn(B, Vt, generator=g).clamp_(max=3.5)
    cols = torch.stack([torch.randperm(Vt, generator=g)[:N_TOP] for _ in range(B)])
    top = 4.0 + 0.125 * torch.arange(N_TOP, dtype=torch.float32)[None, :] + 0.03 * torch.rand(B, N_TOP, generator=g)
    scores.scatter_(1, cols, top)
    order = ranked(scores)
    label = torch.zeros(B, Vt, dtype=torch.int64)
    for r in range(B):
        kind = r % 4
        if kind == 0:
            label[r, order[r, 0]] = 1
        elif kind == 1:
            label[r, order[r, 1 + (r % 9)]] = 1
            label[r, order[r, 40]] = 1
        elif kind == 2:
            label[r, order[r, 10 + (r % 20)]] = 1
    d = {"answer_scores": scores, "answer_label": label,
         "obj_cls_raw_logits": torch.randn(B, N_OBJ, N_CLS, generator=g),
         "obj_labels": torch.randint(0, N_CLS, (B, N_OBJ), generator=g),
         "obj_masks": torch.rand(B, N_OBJ, generator=g) > 0.3}
    d["obj_masks"][:, 0] = True
    if task == "scanqa":
        d["obj_cls_post_logits"] = torch.randn(B, N_OBJ, N_CLS, generator=g)
    else:
        pool = torch.tensor([0, 1, 2, 5] if i == 1 else [0, 1, 2, 3, 5])
        d["sqa_type"] = pool[torch.randint(0, len(pool), (B,), generator=g)]
    return d


def to_device(d: dict, device, scores_dtype=None) -> dict:
    out = {k: v.to(device) for k, v in d.items()}
    if scores_dtype is not None:
        out["answer_scores"] = out["answer_scores"].to(scores_dtype)
    return out


# ---- the evaluators' arithmetic on top of the oracle --------------------------------------------------------------------
def _obj_pair(d, key):
    pred = torch.argmax(d[key], dim=2)
    m = d["obj_masks"]
    return int((pred[m] == d["obj_labels"][m]).sum()), int(m.sum())


def scanqa_pairs(d: dict, scores=None) -> dict:
    """ScanQAEval.batch_metrics(include_count=True) with the law in place of torch.topk."""
    s = d["answer_scores"] if scores is None else scores
    w = words(s, d["answer_label"])
    out = {"ans1_acc": (w[0], w[2]), "ans10_acc": (w[1], w[2])}
    for key in d:
        if key.endswith("logits") and d[key].dim() == 3 and d[key].shape[:2] == d["obj_labels"].shape:
            out[key.replace("logits", "acc")] = _obj_pair(d, key)
    return out


def scanqa_record(batches) -> dict:
    """BaseEvaluator.update / record: the pairs summed, hits / max(count, 1)."""
    tot = {}
    for d in batches:
        for k, (h, c) in scanqa_pairs(d).items():
            a = tot.setdefault(k, [0, 0])
            a[0] += h
            a[1] += c
    return {k: h / max(c, 1) for k, (h, c) in tot.items()}


def sqa3d_metrics(d: dict, scores=None) -> dict:
    """SQA3DEval.batch_metrics in Python floats, with the law in place of torch.topk."""
    s = d["answer_scores"] if scores is None else scores
    B = s.shape[0]
    w = words(s, d["answer_label"], d["sqa_type"], N_TYPES)
    m = {"ans1_acc": w[0] / float(B), "ans10_acc": w[1] / float(B)}
    h, c = _obj_pair(d, "obj_cls_raw_logits")
    m["obj_cls_raw_acc"] = h / float(c)
    for t in range(N_TYPES):
        ct = 1e-10
        for _ in range(w[11 + t]):
            ct += 1
        m[f"type{t}_acc"] = w[3 + t] / ct
        m[f"type{t}_count"] = ct
    m["target_metric"] = m["ans1_acc"]
    m["total_count"] = B
    return m


def sqa3d_record(batches) -> dict:
    """SQA3DEval.update / record: additions left to right from 0.0, one rounding per operation."""
    acc = {k: 0.0 for k in SQA_KEYS}
    type_count = {t: 1e-10 for t in range(N_TYPES)}
    total = 0
    for d in batches:
        m = sqa3d_metrics(d)
        total += m["total_count"]
        for t in range(N_TYPES):
            type_count[t] += m[f"type{t}_count"]
        for k in SQA_KEYS:
            if "type" in k:
                acc[k] = acc[k] + float(m[k]) * m["type" + k[4] + "_count"]
            else:
                acc[k] = acc[k] + float(m[k]) * m["total_count"]
    return {k: (acc[k] / type_count[int(k[4])] if "type" in k else acc[k] / total) for k in SQA_KEYS}


def as_array(m: dict, keys) -> np.ndarray:
    return np.asarray([m[k] for k in keys], dtype=np.float64)
