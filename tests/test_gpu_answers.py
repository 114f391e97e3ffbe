"""The answer-accuracy evaluators on the GPU (gps_answer_hits / gps_answer_fold, csrc/gps_metrics.hip): ranked ids and
integer words against the pure-torch oracle of the ranking law (tests/answers_cases.py; pinned to the reference by
tests/test_answers_host.py) with exact equality, ScanQACounter / SQA3DCounter against the reference's own results
(tests/golden/answers_ref.npz, bit-equal float64), a captured update, and `GPSTrainStep(train_metrics="scanqa")`."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import answers_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.common import answer_hits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "answers_ref.npz"))
NARROW = _native.ANSWER_WAVE_MAX_COLS
WIDTHS = [1, 7, 10, 11, NARROW, NARROW + 1, 706, 8864, 8867]
DTYPES = [torch.float32, torch.bfloat16]
IDS = ["fp32", "bf16"]
NAN = float("nan")


# ---- the kernel against the oracle on the same tensor -----------------------------------------------------------------
def _place(values: torch.Tensor, dtype, fill=NAN, behind=8):
    """(rows, V) fp32 values (already on `dtype`'s grid) -> a (rows, V) view with row pitch V + 3 that starts ONE element
    into its buffer, so row heads and tails are misaligned; the pitch padding, the first element and `behind` elements
    behind the last row hold `fill`."""
    rows, V = values.shape
    ld = V + 3
    body = torch.full((rows, ld), fill, dtype=torch.float32)
    body[:, :V] = values
    flat = torch.full((1 + rows * ld + behind,), fill, dtype=torch.float32)
    flat[1:1 + rows * ld] = body.reshape(-1)
    flat = flat.to(dtype).to(DEV)
    x = flat[1:1 + rows * ld].view(rows, ld)[:, :V]
    assert x.data_ptr() == flat.data_ptr() + flat.element_size() and x.stride(0) == ld
    return x


def _values(rows, V, seed):
    """bf16-exact values: even rows N(0,1) on the bf16 grid, odd rows on a grid of quarter steps (ties everywhere)."""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, V, generator=g).to(torch.bfloat16).float()
    v[1::2] = (v[1::2] * 4).round() / 4
    return v


def _labels(values, k, seed):
    """Multi-hot int64 labels: per row one entry at a ranked place that cycles through 0 .. k + 2 (so past k too) and
    one at a random column; every fourth row unanswerable."""
    g = torch.Generator().manual_seed(seed)
    rows, V = values.shape
    order = C.ranked(values)
    lab = torch.zeros(rows, V, dtype=torch.int64)
    for r in range(rows):
        if r % 4 == 3:
            continue
        lab[r, order[r, min((3 * r + seed) % (k + 3), V - 1)]] = 1
        lab[r, int(torch.randint(0, V, (1,), generator=g))] = 1
    return lab


def _run(x, label, k, types=None, n_types=0, rows_dev=None, words=None, topk=True):
    w = torch.zeros(answer_hits.WORDS, dtype=torch.int64, device=DEV) if words is None else words
    ids = torch.full((x.shape[0], k), -7, dtype=torch.int32, device=DEV) if topk else None
    answer_hits.hits(x, label.to(DEV), w, k=k, types=None if types is None else types.to(DEV), n_types=n_types,
                     rows_dev=rows_dev, topk=ids)
    return w.tolist(), None if ids is None else ids.cpu()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k", [1, 10, 16])
@pytest.mark.parametrize("rows", [1, 5])
@pytest.mark.parametrize("V", WIDTHS)
def test_ranked_ids_and_words_equal_the_oracle(V, rows, k, dtype):
    """Every width at which the kernel takes another path (one wave per row up to 64 columns, one workgroup above; rows
    shorter than k, shorter than a 16-byte granule, with and without a vector body), misaligned heads and tails, NaN in
    every element around the rows."""
    values = _values(rows, V, seed=V + rows + k)
    label = _labels(values, k, seed=V % 7)
    types = (torch.arange(rows) * 5 + V) % 6
    x = _place(values, dtype)
    words, ids = _run(x, label, k, types=types, n_types=6)
    want = C.topk_ids(values, k)
    assert torch.equal(ids, want), (ids, want)
    if V < k:
        assert bool((ids[:, V:] == -1).all()) and bool((ids[:, :V] >= 0).all())      # the hit is taken over the V present
    assert words == C.words(values, label, types, 6, k=k)
    assert words[2] == rows and sum(words[11:17]) == rows


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [NARROW, 8864])
def test_ties(V, dtype):
    """Row 0 all equal: ids 0 .. k-1.  Rows 1, 2: nine distinct best values, then the same value twice -- places 10 and
    11 -- at columns c < c'; the label on c' must miss (row 1), on c it must hit (row 2)."""
    k = 10
    g = torch.Generator().manual_seed(5)
    values = torch.randn(3, V, generator=g).to(torch.bfloat16).float().clamp_(max=2.0)
    values[0] = 0.5
    cols = torch.randperm(V, generator=g)[:11]
    c, c2 = sorted(cols[9:].tolist())
    for r in (1, 2):
        values[r, cols[:9]] = 16.0 + torch.arange(9, dtype=torch.float32)
        values[r, c] = values[r, c2] = 8.0
    label = torch.zeros(3, V, dtype=torch.int64)
    label[0, k] = 1                                            # the first column past the k best of the all-equal row
    label[1, c2] = 1
    label[2, c] = 1
    words, ids = _run(_place(values, dtype), label, k)
    assert ids[0].tolist() == list(range(k))
    assert ids[1, 9] == c and ids[2, 9] == c and torch.equal(ids, C.topk_ids(values, k))
    assert words[:3] == [0, 1, 3]                              # only row 2 hits, and not at place 0


def test_bf16_normal_rows_tie_at_place_ten():
    """N(0,1) scores rounded to bf16 at V = 8864: several rows hold equal values across places 10 / 11, where
    torch.topk's answer is an implementation detail; the kernel's is the law's."""
    rows, V = 32, 8864
    values = torch.randn(rows, V, generator=torch.Generator().manual_seed(77)).to(torch.bfloat16).float()
    order = C.ranked(values)
    top = torch.gather(values, 1, order[:, :11])
    assert int((top[:, 9] == top[:, 10]).sum()) >= 3           # not vacuous
    assert int((~C.tie_free(values)).sum()) >= rows // 3
    label = torch.zeros(rows, V, dtype=torch.int64)
    label[torch.arange(rows), order[:, 10]] = 1                # the first answer OUTSIDE the ten best: no hit by the law
    label[::2, order[::2, 9]] = 1                              # ... and on even rows the last one inside
    words, ids = _run(_place(values, torch.bfloat16), label, 10)
    assert torch.equal(ids, C.topk_ids(values, 10))
    assert words[:3] == [0, rows // 2, rows] == C.words(values, label)[:3]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [11, NARROW, 706])
def test_special_values(V, dtype):
    inf = float("inf")
    g = torch.Generator().manual_seed(3)
    values = torch.randn(6, V, generator=g).to(torch.bfloat16).float()
    values[0, 3], values[0, 7], values[0, 5] = NAN, NAN, inf   # NaN above +inf, the lower NaN first
    values[1, :] = -inf                                        # a row of -inf: ids 0 ..
    values[2, :] = -1.0
    values[2, 2], values[2, 6], values[2, 4] = 0.0, -0.0, 0.0  # -0.0 == +0.0: column order
    values[3, :] = NAN
    values[4, V - 1], values[4, 0] = inf, inf
    values[5, 1], values[5, V - 2] = -inf, NAN
    label = torch.zeros(6, V, dtype=torch.int64)
    label[0, 5] = label[1, 9] = label[2, 4] = label[3, 10] = label[4, V - 1] = label[5, 1] = 1
    words, ids = _run(_place(values, dtype, fill=1e30), label, 10)
    want = C.topk_ids(values, 10)
    assert torch.equal(ids, want)
    assert ids[0, :3].tolist() == [3, 7, 5] and ids[1].tolist() == list(range(10)) and ids[2, :3].tolist() == [2, 4, 6]
    assert ids[3].tolist() == list(range(10)) and ids[4, :2].tolist() == [0, V - 1] and ids[5, 0] == V - 2
    assert words == C.words(values, label)


def test_label_kinds_types_and_row_extent():
    rows, V, k = 9, 706, 10
    values = _values(rows, V, seed=12)
    label = _labels(values, k, seed=2)
    order = C.ranked(values)
    label[0] = 0
    label[0, order[0, 0]] = 2                                  # an entry of 2 does not count (the reference's `== 1`)
    label[1] = 0                                               # unanswerable: count only
    label[2] = 0
    label[2, order[2, 0]] = 1
    types = torch.tensor([0, 1, 7, 3, 5, -1, 2, 2, 0])         # 7 and -1 with n_types = 6: count only
    x = _place(values, torch.float32)
    want = C.words(values, label, types, 6)
    assert want[0] >= 1 and want[2] == rows and sum(want[11:]) == rows - 2 and sum(want[3:11]) < want[0]
    got = {}
    for name, lab in (("int64", label), ("bool", label != 0), ("uint8", label.to(torch.uint8)), ("f32", label.float()),
                      ("int32", label.to(torch.int32)), ("strided", torch.stack([label, label], 2)[:, :, 0])):
        got[name], _ = _run(x, lab, k, types=types, n_types=6)
        assert got[name] == want or name == "bool", name
    # a bool label cannot hold the 2: its row 0 is a hit at place 0, of type 0
    b = list(want)
    b[0] += 1
    b[1] += 1
    b[3] += 1
    assert got["bool"] == b
    # rows_dev below B; the dead rows hold NaN scores and labels of 1 everywhere: nothing of them is read or counted
    live = 4
    dead = values.clone()
    dead[live:] = NAN
    lab2 = label.clone()
    lab2[live:] = 1
    rd = torch.tensor([live], dtype=torch.int32, device=DEV)
    words, ids = _run(_place(dead, torch.float32), lab2, k, types=types, n_types=6, rows_dev=rd)
    assert words == C.words(values, label, types, 6, rows=live) and words[2] == live
    assert torch.equal(ids[:live], C.topk_ids(values[:live], k)) and bool((ids[live:] == -7).all())
    # words accumulate over launches; topk is optional
    acc = torch.zeros(answer_hits.WORDS, dtype=torch.int64, device=DEV)
    for _ in range(2):
        _run(x, label, k, types=types, n_types=6, words=acc, topk=False)
    assert acc.tolist() == [2 * w for w in want]


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_what_lies_around_the_rows_changes_nothing(dtype):
    """The out-of-row-read check, on values: the pitch padding, the element before the first row and the elements behind
    the last hold 0, NaN or +inf -- all three give the same ids and words."""
    values = _values(5, 8867, seed=9)
    label = _labels(values, 10, seed=4)
    runs = [_run(_place(values, dtype, fill=f), label, 10) for f in (0.0, NAN, float("inf"))]
    assert runs[0][0] == runs[1][0] == runs[2][0] == C.words(values, label)
    assert torch.equal(runs[0][1], runs[1][1]) and torch.equal(runs[0][1], runs[2][1])
    assert torch.equal(runs[0][1], C.topk_ids(values, 10))


def test_cols_are_not_limited_by_the_lds():
    V = 70001                                                  # 280 KB of fp32 per row: more than a CU's LDS
    values = _values(2, V, seed=21)
    label = _labels(values, 16, seed=1)
    words, ids = _run(_place(values, torch.float32), label, 16)
    assert torch.equal(ids, C.topk_ids(values, 16)) and words == C.words(values, label, k=16)


# ---- the counters against the reference ---------------------------------------------------------------------------------
def _item(d):
    return {k: v.item() for k, v in d.items()}


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_scanqa_counter_is_equal_to_the_reference(dtype):
    from sceneverse_amd.engine import ScanQACounter, scanqa_accuracy
    keys = tuple(GOLD["scanqa/keys"].tolist())
    c = ScanQACounter(DEV, topk=True)
    assert c.result() == {} and c.last() == {} and c.last_topk() is None
    total = np.zeros((len(keys), 2), dtype=np.int64)
    for i in range(len(C.SIZES)):
        cpu = C.batch("scanqa", i)
        d = C.to_device(cpu, DEV, dtype)                       # bf16: the same scores on the coarser grid, still tie-free
        c.update(d)
        last = _item(c.last())
        assert tuple(last) == keys
        assert np.array_equal(C.as_array(last, keys), GOLD[f"scanqa/{i}/metrics"]), (i, last)
        total += GOLD[f"scanqa/{i}/pairs"]
        pairs = c.result(include_count=True)
        assert np.array_equal(np.asarray([pairs[k] for k in keys]), total)
        assert torch.equal(c.last_topk().cpu(), C.topk_ids(cpu["answer_scores"]))
        # tie-free: the torch composition agrees
        t = scanqa_accuracy(d["answer_scores"], d["answer_label"])
        assert t["ans1_acc"] == last["ans1_acc"] and t["ans10_acc"] == last["ans10_acc"]
    assert np.array_equal(C.as_array(c.result(), keys), GOLD["scanqa/record"])
    assert c.words.tolist() == [0] * answer_hits.WORDS and not c.cls_words.any()     # the fold cleared the batch words
    c.reset()
    assert c.result() == {} and c.last() == {} and not c._sums.any()
    c.update({k: v for k, v in d.items() if k in ("answer_scores", "answer_label")})  # the scores and labels alone
    assert tuple(c.result()) == ("ans1_acc", "ans10_acc")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_sqa3d_counter_is_bit_equal_to_the_reference(dtype):
    from sceneverse_amd.engine import SQA3DCounter, sqa3d_accuracy
    keys = tuple(GOLD["sqa3d/keys"].tolist())
    assert keys == SQA3DCounter.KEYS
    counts = [f"type{t}_count" for t in range(C.N_TYPES)]
    c = SQA3DCounter(DEV)
    for rounds in range(2):                                    # the second round after reset(): the same numbers
        for i in range(len(C.SIZES)):
            d = C.to_device(C.batch("sqa3d", i), DEV, dtype)
            c.update(d)
            last = _item(c.last())
            assert tuple(last) == keys + tuple(counts)
            assert np.array_equal(C.as_array(last, keys), GOLD[f"sqa3d/{i}/metrics"]), (i, last)
            assert np.array_equal(C.as_array(last, counts), GOLD[f"sqa3d/{i}/type_count"])
            t = sqa3d_accuracy(d["answer_scores"], d["answer_label"], d["sqa_type"])
            assert all(t[k] == last[k] for k in t if k != "total_count")
        rec = c.result()
        assert tuple(rec) == keys and np.array_equal(C.as_array(rec, keys), GOLD["sqa3d/record"]), rec
        c.reset()
        assert c.result() == {} and c.last() == {} and c._type_total.tolist() == [1e-10] * C.N_TYPES
    # a batch without a masked object: obj_cls_raw_acc is defined as 0
    d["obj_masks"] = torch.zeros_like(d["obj_masks"])
    c.update(d)
    assert c.last()["obj_cls_raw_acc"].item() == 0.0 and c.last()["ans1_acc"].item() == GOLD["sqa3d/2/metrics"][2]


@pytest.mark.parametrize("task", ["scanqa", "sqa3d"])
def test_update_captured_in_a_graph_replays_over_the_batches(task):
    """`update` makes no host sync: captured once on static buffers and replayed for the three batches (cut / repeated
    to the first batch's B), it gives what the eager counter gives."""
    from sceneverse_amd import engine
    B = C.SIZES[0]
    batches = []
    for i in range(len(C.SIZES)):
        d = C.batch(task, i)
        batches.append(C.to_device({k: v[torch.arange(B) % v.shape[0]].contiguous() for k, v in d.items()}, DEV))
    cls = engine.ScanQACounter if task == "scanqa" else engine.SQA3DCounter
    eager, captured = cls(DEV, topk=True), cls(DEV, topk=True)
    static = {k: v.clone() for k, v in batches[0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.update(static)                                # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    captured.reset()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        captured.update(static)
    for b in batches:
        eager.update(b)
        for k, v in b.items():
            static[k].copy_(v)
        g.replay()
        assert _item(captured.last()) == _item(eager.last()) and len(eager.last()) >= 4
        assert torch.equal(captured.last_topk(), eager.last_topk())
    assert captured.result() == eager.result() and eager.result()["ans10_acc"] > 0


# ---- the engine ------------------------------------------------------------------------------------------------------
def _engine(graph, **kw):
    import torch.nn as nn
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.engine import GPSTrainStep
    from sceneverse_amd.modules.layers.transformers import MultiheadSelfAttention
    from tests.qa_cases import as_qa_cfg
    st = GPSTrainStep(as_qa_cfg(gps_pretrain_cfg(_lang_dir())), device=DEV, ddp=False, graph=graph, graph_warmup=2, seed=7,
                      **kw)
    for m in st.model.modules():                               # deterministic steps: no dropout
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, MultiheadSelfAttention):
            m.dropout = 0.0
        if hasattr(m, "attention_probs_dropout_prob"):
            m.attention_probs_dropout_prob = 0.0
        if hasattr(m, "dropout_prob"):
            m.dropout_prob = 0.0
    return st


def _qa_batches(n):
    from sceneverse_amd.data.synthetic import synth_qa_batch
    from tests.qa_cases import N_ANSWERS
    return [synth_qa_batch(2, n_obj=6, n_pts=1024, txt_len=12, n_answers=N_ANSWERS, seed=60 + i, min_real=3, device=DEV)
            for i in range(n)]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "graph"])
def test_train_metrics_scanqa_equal_a_counter_fed_the_same_outputs(graph):
    """Right before the engine's own update (inside the capture in the graph mode, so that it replays) a fresh
    ScanQACounter is fed the same outputs."""
    from sceneverse_amd.engine import ScanQACounter
    own = ScanQACounter(DEV)
    st = _engine(graph, train_metrics="scanqa" if graph else own)      # by name, or a counter instance taken as it is
    assert isinstance(st.metric_counter, ScanQACounter) and (graph or st.metric_counter is own)
    ref = ScanQACounter(DEV)
    seen = []

    def hook(engine, out):
        with torch.no_grad():
            ref.update(out)
        seen.append(1)

    st.metrics_hook = hook
    for b in _qa_batches(4):
        st.step(dict(b))
        got, want = st.train_metrics(), ref.last()
        assert tuple(got) == tuple(want) and tuple(got)[:2] == ("ans1_acc", "ans10_acc")
        assert _item(got) == _item(want) and all(0.0 <= v.item() <= 1.0 for v in got.values())
    assert st.metric_counter.result(include_count=True) == ref.result(include_count=True)
    assert st.metric_counter.result(include_count=True)["ans1_acc"][1] == 8          # 4 steps of 2 questions
    if graph:
        assert st._graph is not None and len(seen) == 3        # two warm-up steps, one capture, then replays


def test_train_metrics_off_is_the_step_as_it_was():
    runs = []
    for kw in ({}, {"train_metrics": False}):
        st = _engine(False, **kw)
        assert st.metric_counter is None
        runs.append([st.step(dict(b))[0].clone() for b in _qa_batches(3)])
        with pytest.raises(RuntimeError):
            st.train_metrics()
    assert all(torch.equal(a, b) for a, b in zip(*runs))
