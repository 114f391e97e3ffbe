"""The device-side evaluators on the GPU (csrc/gps_metrics.hip): gps_cls_hits against torch.argmax on the same tensor
(integers equal), the three counters of engine.py against the reference's own results (tests/golden/metrics_ref.npz,
bit-equal float64), the masked-LM hit count of the lazy path, and `GPSTrainStep(train_metrics=...)` in its three modes."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import metrics_cases as C  # noqa: E402
from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.common import cls_hits  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLD = np.load(os.path.join(HERE, "golden", "metrics_ref.npz"))
W = _native.CLS_HITS_WAVE_MAX_COLS
WIDTHS = [1, 63, 64, 65, 80, 607, W - 1, W, W + 1, 2 * W + 3, 4 * W + 8]
DTYPES = [torch.bfloat16, torch.float32]
IDS = ["bf16", "fp32"]


# ---- the kernel against torch on the same tensor ---------------------------------------------------------------------
def _tensor(rows, V, dtype, seed, pitch_pad=0, offset=0):
    """(rows, V) logits living in a buffer with row pitch V + pitch_pad, starting `offset` elements into it; the pad
    columns hold +inf and NaN.  Planted rows (cyclic): maximum in column 0, in column V - 1, in the scalar head, in the
    scalar tail, two equal maxima in different lanes, in different waves, a NaN pair, all -inf."""
    g = torch.Generator().manual_seed(seed)
    ld = V + pitch_pad
    buf = torch.randn(rows, ld, generator=g).to(torch.bfloat16).float()
    big = 30.0
    for r in range(rows):
        k = r % 10
        if k == 0:
            buf[r, 0] = big
        elif k == 1:
            buf[r, V - 1] = big
        elif k == 2:
            buf[r, min(3, V - 1)] = big                       # before the first 16-byte granule of most rows
        elif k == 3:
            buf[r, max(V - 2, 0)] = big                       # behind the last whole granule of most rows
        elif k == 4:
            buf[r, V // 3] = buf[r, min(V // 3 + 9, V - 1)] = big
        elif k == 5:
            buf[r, V // 7] = buf[r, V - 1 - V // 7] = buf[r, V // 2] = big     # lanes of different waves in a wide row
        elif k == 6:
            buf[r, V // 2] = buf[r, V - 1] = float("nan")
            buf[r, 0] = big
        elif k == 7:
            buf[r, :V] = float("-inf")
    if pitch_pad:
        buf[:, V::2] = float("inf")
        buf[:, V + 1::2] = float("nan")
    flat = torch.zeros(offset + rows * ld, dtype=dtype, device=DEV)
    flat[offset:] = buf.reshape(-1).to(dtype).to(DEV)
    x = flat[offset:].view(rows, ld)[:, :V]
    assert x.data_ptr() == flat.data_ptr() + offset * flat.element_size()
    return x


def _labels(x, seed, ignore=-1):
    """About half of the rows carry their own arg-max; the rest: random, the ignore index, negative, >= V."""
    rows, V = x.shape
    g = torch.Generator().manual_seed(seed + 1)
    pred = torch.argmax(x.float().cpu(), dim=1)
    lab = torch.where(torch.rand(rows, generator=g) < 0.5, pred, torch.randint(0, V, (rows,), generator=g))
    for r in range(rows):
        if r % 11 == 3:
            lab[r] = ignore
        elif r % 11 == 5:
            lab[r] = -7
        elif r % 11 == 8:
            lab[r] = V + r % 2
    return lab.to(DEV)


def _expected(x, labels, ignore=None, rows_dev=None, sel=None, a=None, b=None):
    rows = x.shape[0]
    pred = torch.argmax(x.float().cpu(), dim=1)
    lab = labels.cpu()
    counted = torch.arange(rows) < (rows if rows_dev is None else rows_dev)
    if sel is not None:
        counted &= sel.cpu() != 0
    if ignore is not None:
        counted &= lab != ignore
    hit = counted & (pred == lab)
    fa = torch.zeros(rows, dtype=torch.bool) if a is None else a.cpu() != 0
    fb = torch.zeros(rows, dtype=torch.bool) if b is None else b.cpu() != 0
    return [int(v.sum()) for v in (hit, counted, hit & fa, counted & fa, hit & fb, counted & fb)]


def _run(x, labels, ignore=None, rows_dev=None, sel=None, a=None, b=None, words=None):
    words = torch.zeros(6, dtype=torch.int64, device=DEV) if words is None else words
    ext = None if rows_dev is None else torch.tensor([rows_dev], dtype=torch.int32, device=DEV)
    cls_hits.launch([cls_hits.problem(x, labels, words, ignore_index=ignore, rows_dev=ext, sel=sel, split_a=a, split_b=b)],
                    torch.device(DEV))
    return words.tolist()


def _mask(rows, seed, p=0.6, dtype=torch.bool):
    m = torch.rand(rows, generator=torch.Generator().manual_seed(seed)) < p
    return (m.to(torch.int64) * 5 if dtype == torch.int64 else m).to(DEV)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", WIDTHS)
def test_hits_equal_torch_argmax_at_every_width(V, dtype):
    for rows in (1, 4, 5, 64):
        for pad, off in ((0, 0), (5, 0), (0, 1), (3, 1)):
            x = _tensor(rows, V, dtype, seed=V * 131 + rows, pitch_pad=pad, offset=off)
            lab = _labels(x, seed=V + rows)
            # every row, no masks: the plain hit count
            assert _run(x, lab) == _expected(x, lab), (V, rows, pad, off)
            sel, a, b = _mask(rows, 1), _mask(rows, 2, 0.5), _mask(rows, 3, 0.3, torch.int64)
            got = _run(x, lab, ignore=-1, sel=sel, a=a, b=b)
            assert got == _expected(x, lab, ignore=-1, sel=sel, a=a, b=b), (V, rows, pad, off)
    if dtype == torch.bfloat16 and V % 2 == 1 and V > 1:
        x = _tensor(4, V, dtype, seed=9)
        assert x.stride(0) == V and (x[1].data_ptr() % 4) == 2          # ld == V, odd: rows at 2-byte alignment


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("V", [607, 2 * W + 3])
def test_row_extent_and_mask_kinds(V, dtype):
    rows = 64
    x = _tensor(rows, V, dtype, seed=V, pitch_pad=6)
    lab = _labels(x, seed=77)
    for ext in (0, 1, 29, rows):
        assert _run(x, lab, ignore=-1, rows_dev=ext) == _expected(x, lab, ignore=-1, rows_dev=ext), ext
    for kind in (torch.bool, torch.int64):
        sel, a, b = _mask(rows, 4, dtype=kind), _mask(rows, 5, 0.5, kind), _mask(rows, 6, 0.4, kind)
        assert _run(x, lab, sel=sel, a=a, b=b, rows_dev=40) == _expected(x, lab, sel=sel, a=a, b=b, rows_dev=40)
        none, every = torch.zeros_like(sel), torch.ones_like(sel)
        assert _run(x, lab, sel=none, a=every, b=every) == [0] * 6
        want = _expected(x, lab)
        assert _run(x, lab, sel=every, a=every, b=none) == want[:2] + want[:2] + [0, 0]
        assert _run(x, lab, sel=every.view(8, 8), a=a.view(8, 8)) == _expected(x, lab, a=a)
    u8 = _mask(rows, 4).to(torch.uint8) * 200
    assert _run(x, lab, sel=u8) == _expected(x, lab, sel=u8)
    mixed = _run(x, lab, sel=_mask(rows, 4), a=_mask(rows, 5, 0.5, torch.int64))     # one element size per problem
    assert mixed == _expected(x, lab, sel=_mask(rows, 4), a=_mask(rows, 5, 0.5))


def test_eight_problems_in_one_launch_equal_single_launches_and_accumulate():
    dev = torch.device(DEV)
    shapes = [(5, 80, torch.float32), (64, 2 * W + 3, torch.bfloat16), (1, W, torch.bfloat16), (7, 607, torch.bfloat16),
              (3, 4 * W + 8, torch.float32), (64, 1, torch.float32), (9, W + 1, torch.bfloat16), (33, 63, torch.bfloat16)]
    items = []
    for i, (rows, V, dtype) in enumerate(shapes):
        x = _tensor(rows, V, dtype, seed=500 + i, pitch_pad=i % 3, offset=i % 2)
        lab = _labels(x, seed=600 + i)
        kw = dict(ignore_index=-1 if i % 2 else None, sel=_mask(rows, 10 + i) if i % 3 else None,
                  split_a=_mask(rows, 20 + i, 0.5), split_b=_mask(rows, 30 + i, 0.5) if i % 2 else None)
        ext = torch.tensor([max(rows - 2, 0)], dtype=torch.int32, device=DEV) if i in (1, 6) else None
        items.append((x, lab, kw, ext))
    single = torch.zeros((8, 6), dtype=torch.int64, device=DEV)
    for i, (x, lab, kw, ext) in enumerate(items):
        cls_hits.launch([cls_hits.problem(x, lab, single[i], rows_dev=ext, **kw)], dev)
        want = _expected(x, lab, ignore=kw["ignore_index"], rows_dev=None if ext is None else int(ext.item()), sel=kw["sel"],
                         a=kw["split_a"], b=kw["split_b"])
        assert single[i].tolist() == want, i
    assert int(single[:, 1].sum()) > 0 and int(single[:, 0].sum()) > 0
    runs = []
    for _ in range(2):                                       # two runs: identical words
        grouped = torch.zeros((8, 6), dtype=torch.int64, device=DEV)
        cls_hits.launch([cls_hits.problem(x, lab, grouped[i], rows_dev=ext, **kw)
                         for i, (x, lab, kw, ext) in enumerate(items)], dev)
        runs.append(grouped)
    assert torch.equal(runs[0], single) and torch.equal(runs[1], single)
    # a second launch into the same words adds; two problems may share their words
    cls_hits.launch([cls_hits.problem(x, lab, runs[0][i], rows_dev=ext, **kw) for i, (x, lab, kw, ext) in enumerate(items)], dev)
    assert torch.equal(runs[0], 2 * single)
    shared = torch.zeros(6, dtype=torch.int64, device=DEV)
    cls_hits.launch([cls_hits.problem(x, lab, shared, rows_dev=ext, **kw) for x, lab, kw, ext in items[:3]], dev)
    assert torch.equal(shared, single[:3].sum(0))
    with pytest.raises(ValueError):
        cls_hits.launch([cls_hits.problem(items[0][0], items[0][1], shared)] * 9, dev)


def test_non_contiguous_and_other_dtypes_are_brought_to_rows():
    x = _tensor(6, 80, torch.float32, seed=3)
    lab = _labels(x, seed=4)
    want = _expected(x, lab)
    assert _run(x.t().contiguous().t(), lab) == want                       # column-major: copied
    assert _run(x.half(), lab) == _expected(x.half(), lab)                 # fp16 -> fp32
    assert _run(x.view(2, 3, 80), lab.view(2, 3)) == want
    with pytest.raises(ValueError):
        _run(x, lab[:5])
    with pytest.raises(ValueError):
        _run(x, lab, sel=_mask(5, 1))


def test_metrics_fold_arithmetic():
    """One launch: ratios, weighted sums, the mean, the total, and the counters back at zero."""
    words = torch.tensor([[3, 7, 1, 2, 0, 0], [5, 0, 0, 0, 0, 0]], dtype=torch.int64, device=DEV)
    w = lambda s, i: words[s, i:i + 1]  # noqa: E731
    terms = [cls_hits.term(w(0, 0), w(0, 1), eps=1e-8), cls_hits.term(w(0, 2), w(0, 3), eps=1e-8),
             cls_hits.term(w(0, 0), w(0, 1), w(0, 2), w(0, 3), eps=1e-8), cls_hits.term(w(1, 0), const_denominator=8.0)]
    last = torch.zeros(5, dtype=torch.float64, device=DEV)
    acc = torch.full((5,), 0.5, dtype=torch.float64, device=DEV)
    total = torch.tensor([2.0], dtype=torch.float64, device=DEV)
    cls_hits.fold(terms, 3.0, 3, last, acc, total)
    f = np.float64
    r = [f(3) / (f(7) + f(1e-8)), f(1) / (f(2) + f(1e-8)), f(2) / (f(5) + f(1e-8)), f(5) / f(8)]
    mean = (((f(0) + r[0]) + r[1]) + r[2]) / f(3)
    assert last.tolist() == [float(v) for v in r + [mean]]
    assert acc.tolist() == [float(f(0.5) + v * f(3)) for v in r + [mean]]
    assert total.tolist() == [5.0] and int(words.abs().sum()) == 0
    cls_hits.fold(terms, 4.0, 0, last, acc, total)                           # no mean: its slot is left alone
    assert last.tolist() == [0.0, 0.0, 0.0, 0.0, float(mean)] and total.tolist() == [9.0]


# ---- the counters against the reference's results --------------------------------------------------------------------
def _gold_dict(seq, name):
    return dict(zip(C.SEQUENCES[seq][0], GOLD[f"{seq}/{name}"].tolist()))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("seq", C.PRETRAIN)
def test_pretrain_counter_is_bit_equal_to_the_reference(seq, dtype):
    from sceneverse_amd.engine import PretrainCounter
    keys, sizes = C.SEQUENCES[seq]
    c = PretrainCounter(DEV)
    for rnd in range(2):                                     # reset() gives a fresh evaluation
        for i in range(len(sizes)):
            c.update(C.to_device(C.batch(seq, i), DEV, dtype))
            last = c.last()
            assert tuple(last) == tuple(keys)
            assert all(v.dtype == torch.float64 and v.dim() == 0 and v.is_cuda for v in last.values())
            assert {k: v.item() for k, v in last.items()} == _gold_dict(seq, f"{i}/metrics"), (seq, i)
        assert c.result() == _gold_dict(seq, "record")
        assert int(c.words.abs().sum()) == 0                 # the fold cleared the batch's counts
        c.reset()
        assert c.result() == {}


def test_pretrain_counter_key_filter_and_key_set():
    from sceneverse_amd.engine import PretrainCounter
    c = PretrainCounter(DEV, keys=["lang_cls_acc_mask", "obj_cls_pre_acc_mask"])
    c.update(C.to_device(C.batch("pre", 0), DEV))
    g = _gold_dict("pre", "0/metrics")
    got = {k: v.item() for k, v in c.last().items()}
    assert got == {k: g[k] for k in ("lang_cls_acc_mask", "obj_cls_pre_acc_mask")}
    full = PretrainCounter(DEV)
    full.update(C.to_device(C.batch("pre", 0), DEV))
    with pytest.raises(ValueError):                          # another key set needs a reset()
        full.update(C.to_device(C.batch("pre_min", 0), DEV))
    # integer masks count as nonzero = true
    d = C.to_device(C.batch("pre", 1), DEV)
    d["obj_masks"], d["obj_sem_masks"] = d["obj_masks"].to(torch.int64) * 3, d["obj_sem_masks"].to(torch.uint8)
    ints = PretrainCounter(DEV)
    ints.update(d)
    assert {k: v.item() for k, v in ints.last().items()} == _gold_dict("pre", "1/metrics")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("seq", ["referit", "perscene", "objcls"])
def test_count_counters_equal_the_reference(seq, dtype):
    from sceneverse_amd.engine import ObjClsCounter, ReferIt3DCounter
    keys, sizes = C.SEQUENCES[seq]
    c = (ObjClsCounter if seq == "objcls" else ReferIt3DCounter)(DEV)
    total = np.zeros((len(keys), 2), dtype=np.int64)
    for i in range(len(sizes)):
        one = type(c)(DEV)
        one.update(C.to_device(C.batch(seq, i), DEV, dtype))
        pairs = one.result(include_count=True)
        assert tuple(sorted(pairs)) == tuple(sorted(keys))
        assert np.array_equal(np.asarray([pairs[k] for k in keys]), GOLD[f"{seq}/{i}/pairs"]), (seq, i)
        assert one.result() == _gold_dict(seq, f"{i}/metrics")
        c.update(C.to_device(C.batch(seq, i), DEV, dtype))
        total += GOLD[f"{seq}/{i}/pairs"]
    pairs = c.result(include_count=True)
    assert np.array_equal(np.asarray([pairs[k] for k in keys]), total)
    assert c.result() == _gold_dict(seq, "record")
    c.reset()
    assert all(v == (0, 0) for v in c.result(include_count=True).values())


@pytest.mark.parametrize("seq", ["pre", "referit", "objcls"])
def test_update_captured_in_a_graph_replays_over_the_sequence(seq):
    """`update` makes no host sync: it is captured once on static batch buffers and replayed for every batch of a
    sequence of equal shapes (the sequence's batches cut / repeated to its first B)."""
    from sceneverse_amd import engine
    keys, sizes = C.SEQUENCES[seq]
    B = sizes[0]

    def fit(d):                                              # every batch at the first batch's B (rows repeated / cut)
        out = {}
        for k, v in d.items():
            idx = torch.arange(B) % v.shape[0]
            out[k] = v[idx].contiguous()
        return out

    batches = [C.to_device(fit(C.batch(seq, i)), DEV) for i in range(len(sizes))]
    cls = {"pre": engine.PretrainCounter, "referit": engine.ReferIt3DCounter, "objcls": engine.ObjClsCounter}[seq]
    eager, captured = cls(DEV), cls(DEV)
    static = {k: v.clone() for k, v in batches[0].items()}
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        captured.update(static)                              # warm-up outside the capture
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
        if seq == "pre":
            assert {k: v.item() for k, v in captured.last().items()} == {k: v.item() for k, v in eager.last().items()}
    if seq == "pre":
        assert captured.result() == eager.result() and len(captured.result()) == len(keys)
    else:
        assert captured.result(include_count=True) == eager.result(include_count=True)
        assert eager.result(include_count=True)[keys[-1]][1] > 0


# ---- the masked-LM hit count on the lazy path ------------------------------------------------------------------------
def _lazy_run(head, hidden, labels, words):
    """loss + gradients of the head on the fused path (training mode, bf16 autocast), with the sink when `words`."""
    import contextlib
    from sceneverse_amd.modules.heads.pretrain_head import fused_lm_loss
    from sceneverse_amd.optim.loss import fused_lm_loss as F_lm
    for p in head.parameters():
        p.grad = None
    h = hidden.clone().requires_grad_(True)
    sink = None
    with torch.autocast(device_type="cuda", dtype=torch.bfloat16), fused_lm_loss(True):
        lazy = head(h)
        assert isinstance(lazy, F_lm.LazyLMLogits)
        with (F_lm.hits_sink(words) if words is not None else contextlib.nullcontext()) as sink:
            if sink is not None:
                sink.keep = True
            loss = lazy.loss(labels, ignore_index=-1)
    loss.backward()
    grads = [h.grad.clone()] + [p.grad.clone() for p in head.parameters()]
    return lazy, loss.detach().clone(), grads, sink


def test_lazy_path_hit_count():
    head, hidden, labels = C.lazy_case()
    head, hidden, labels = head.to(DEV), hidden.to(DEV), labels.to(DEV)
    words = torch.zeros(6, dtype=torch.int64, device=DEV)
    lazy, loss_on, grads_on, sink = _lazy_run(head, hidden, labels, words)
    assert sink.launches == 1
    logits, lp, n_valid, V = sink.saved
    nv = int(n_valid.item())
    assert V == C.LAZY_VOCAB and logits.shape[1] == 30528 and nv == int((labels != -1).sum())
    # exactly torch.argmax over the SAME saved labelled-row logits
    pred = torch.argmax(logits[:nv, :V].float(), dim=1)
    assert words.tolist() == [int((pred == lp[:nv]).sum()), nv, 0, 0, 0, 0]
    # against the fp32 logits: every labelled row with a clear top-two margin agrees
    with torch.no_grad():
        full = lazy.materialize().float().reshape(-1, V)
    rows = full[labels.reshape(-1) != -1]                    # the plan keeps the labelled rows in their order
    assert torch.equal(lp[:nv], labels.reshape(-1)[labels.reshape(-1) != -1])
    clear = C.clear_margin(rows)
    share = clear.float().mean().item()
    print(f"lazy path: {nv} labelled rows, {share:.3f} outside the margin, hits {words[0].item()}")
    assert share >= 0.75 and nv // 4 <= int(words[0]) <= nv // 2 + 1      # every second label is an fp32 arg-max
    agree = pred == torch.argmax(rows, dim=1)
    assert bool(agree[clear].all()), (int((~agree & clear).sum()), nv)
    # the sink changes neither the loss nor any gradient
    _, loss_off, grads_off, _ = _lazy_run(head, hidden, labels, None)
    assert torch.equal(loss_on, loss_off)
    assert len(grads_on) == len(grads_off) and all(torch.equal(a, b) for a, b in zip(grads_on, grads_off))
    assert words.tolist()[1] == nv                           # and no launch without the sink


def test_pretrain_counter_uses_the_sink_or_materializes():
    from sceneverse_amd.engine import PretrainCounter
    from sceneverse_amd.modules.heads.pretrain_head import fused_lm_loss
    head, hidden, labels = C.lazy_case()
    head, hidden, labels = head.to(DEV), hidden.to(DEV), labels.to(DEV)
    c = PretrainCounter(DEV, keys=["lang_cls_acc_mask"])
    with torch.no_grad(), torch.autocast(device_type="cuda", dtype=torch.bfloat16), fused_lm_loss(True):
        lazy = head(hidden)
        with c.sink() as sink:
            sink.keep = True
            lazy.loss(labels, ignore_index=-1)
    logits, lp, n_valid, V = sink.saved
    nv = int(n_valid.item())
    hits = int((torch.argmax(logits[:nv, :V].float(), dim=1) == lp[:nv]).sum())
    c.update({"txt_lm_cls_logits": lazy, "masked_lm_labels": labels})
    assert c.last()["lang_cls_acc_mask"].item() == hits / float(nv + 1e-8)
    # no loss under the sink since: the counter materialises the (B, L, V) logits itself
    c.update({"txt_lm_cls_logits": lazy, "masked_lm_labels": labels})
    with torch.no_grad():
        full = lazy.materialize()
    want = int((torch.argmax(full, dim=2)[labels != -1] == labels[labels != -1]).sum())
    assert c.last()["lang_cls_acc_mask"].item() == want / float(nv + 1e-8)


# ---- the engine ------------------------------------------------------------------------------------------------------
def _engine(graph, **kw):
    import torch.nn as nn
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.engine import GPSTrainStep
    from sceneverse_amd.modules.layers.transformers import MultiheadSelfAttention
    st = GPSTrainStep(gps_pretrain_cfg(_lang_dir()), device=DEV, ddp=False, graph=graph, graph_warmup=2, seed=7, **kw)
    for m in st.model.modules():                             # deterministic steps: no dropout
        if isinstance(m, nn.Dropout):
            m.p = 0.0
        if isinstance(m, MultiheadSelfAttention):
            m.dropout = 0.0
        if hasattr(m, "attention_probs_dropout_prob"):
            m.attention_probs_dropout_prob = 0.0
        if hasattr(m, "dropout_prob"):
            m.dropout_prob = 0.0
    return st


def _batches(n=4):
    from sceneverse_amd.data.synthetic import synth_batch
    return [synth_batch(4, n_obj=16, seed=40 + i, min_real=5, device=DEV) for i in range(n)]


@pytest.mark.parametrize("graph", [False, True, "dp"], ids=["eager", "graph", "graph_dp"])
def test_train_metrics_equal_a_counter_fed_the_same_outputs(graph):
    """Right before the engine's own update (inside the capture in the graph modes, so that it replays), a second
    PretrainCounter is fed the same outputs as plain tensors: the labelled-row logits the loss has just computed stand in
    for `txt_lm_cls_logits` (rows past the device-side count carry label -1)."""
    from sceneverse_amd.engine import PretrainCounter
    st = _engine(graph, train_metrics=True)
    ref = PretrainCounter(DEV)
    with st.metric_counter.sink() as sink:                   # creates the engine counter's sink
        sink.keep = True
    seen = []

    def hook(engine, out):
        logits, lp, n_valid, V = sink.saved
        B, L = out["masked_lm_labels"].shape
        live = torch.arange(lp.numel(), device=lp.device) < n_valid
        d = {k: v for k, v in out.items() if torch.is_tensor(v) or hasattr(v, "materialize")}
        d["txt_lm_cls_logits"] = logits[:, :V].reshape(B, L, V)
        d["masked_lm_labels"] = torch.where(live, lp, torch.full_like(lp, -1)).reshape(B, L)
        with torch.no_grad():
            ref.update(d)
        seen.append(1)

    st.metrics_hook = hook
    for b in _batches():
        st.step(dict(b))
        got, want = st.train_metrics(), ref.last()
        assert tuple(got) == tuple(want) and "lang_cls_acc_mask" in got and "target_metric" in got
        assert {k: v.item() for k, v in got.items()} == {k: v.item() for k, v in want.items()}
        assert all(0.0 <= v.item() <= 1.0 for v in got.values())
    assert st.metric_counter.result() == ref.result()
    if graph:
        assert st._graph is not None and len(seen) == 3      # two warm-up steps, one capture, then replays
    assert sink.launches == 0                                # every update consumed the loss's hit count


def test_train_metrics_off_is_the_step_as_it_was():
    runs = []
    for kw in ({}, {"train_metrics": False}):
        st = _engine(False, **kw)
        assert st.metric_counter is None
        runs.append([st.step(dict(b))[0].clone() for b in _batches(3)])
        with pytest.raises(RuntimeError):
            st.train_metrics()
    assert all(torch.equal(a, b) for a, b in zip(*runs))
