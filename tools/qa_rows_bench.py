"""Timing of the device-side ScanQA batch (csrc/gps_obj_select_qa.hip, sceneverse_amd/data/gpu_qa.py: qa_rows) against
the host path it replaces.

    python tools/qa_rows_bench.py [--rounds 5] [--samples 10] [--out profiles/qa_rows/qa_rows_bench.txt]

Batch: B = 32 questions (the configs' batch), O = 80, M = 79, A = 8864 answers, 607 classes, scans of 128 to 384 objects
(about one in seven background), 0 to 3 targets and 0 to 3 answers per question, float32 multi-hots, the fill drawn on the
device.  The three measurements ALTERNATE for `--rounds` rounds, so that a drift of the machine meets all of them alike;
per measurement the median over all its samples, with min and max:
  * the launch alone: 20 launches captured into one graph and replayed, divided by 20 (GPU time, no host launch path),
    `--samples` device-event windows per round;
  * the wrapper call as a loader makes it: `qa_rows(out=static buffers)` eager, q_idx and the keep table already on the
    device, `--samples` device-event windows per round;
  * the host path: this tool's own restatement of the per-sample selection (filter, targets first, class-mates,
    `random.shuffle`, the three multi-hots as numpy arrays) over the same batch in one process, the batch stacked and
    its tensors uploaded, host clock around work that ends in a device synchronise, one batch per round.  It is not the
    reference's code."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_qa import PackedQuestions, qa_rows  # noqa: E402

GRAPH_ITERS = 20
N_LABELS = 607
INT2CAT = ["wall", "floor", "ceiling"] + [f"cat{i}" for i in range(3, N_LABELS)]


def event_samples(fn, n):
    """n device-event timings of fn() in us."""
    out = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize()
        out.append(s.elapsed_time(e) * 1e3)
    return out


def captured(fn, iters):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    return g.replay


def host_item(obj_labels, targets, answers, max_obj_len, n_answers):
    """One question through the per-sample work: filter, targets first, class-mates, shuffle, the three multi-hots."""
    selected = [i for i, l in enumerate(obj_labels) if INT2CAT[l] not in ["wall", "floor", "ceiling"]]
    for t in targets:
        if t not in selected:
            selected.append(t)
    labels = [obj_labels[i] for i in selected]
    tgt = [selected.index(t) for t in targets]
    tgt_labels = [labels[t] for t in tgt]
    rows = selected
    if max_obj_len < len(labels):
        picked, remained = list(tgt), []
        for kobj, klabel in enumerate(labels):
            if kobj not in tgt:
                if klabel in tgt_labels:
                    picked.append(kobj)
                else:
                    remained.append(kobj)
            if len(picked) == max_obj_len:
                break
        if len(picked) < max_obj_len:
            random.shuffle(remained)
            picked += remained[:(max_obj_len - len(picked))]
        rows = [selected[i] for i in picked]
        labels = [labels[i] for i in picked]
        tgt = list(range(len(tgt)))
    if not tgt:
        tgt, tgt_labels = [len(rows)], [5]
    row = np.full(max_obj_len + 1, -1, np.int32)
    row[:len(rows)] = rows
    obj = np.full(max_obj_len + 1, -100, np.int64)
    obj[:len(rows)] = labels
    answer_label = np.zeros(n_answers, np.float32)
    answer_label[answers] = 1
    tgt_object_id = np.zeros(max_obj_len + 1, np.float32)
    tgt_object_id[tgt] = 1
    tgt_object_label = np.zeros(N_LABELS, np.float32)
    tgt_object_label[tgt_labels] = 1
    return row, obj, tgt_object_id, tgt_object_label, answer_label


def line(name, t):
    return f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "qa_rows_bench.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {args.rounds} alternating rounds, {args.samples} device-event "
             f"samples per round and measurement after warm-up; median [min .. max]; host CPUs visible: {os.cpu_count()}, "
             f"host path in one process, one batch per round"]
    rng = np.random.default_rng(0)
    n_scans, n_questions, B, M, O, A = 64, 512, 32, 79, 80, 8864
    packed, scans = G.PackedScans(dev), []
    for s in range(n_scans):
        n = int(rng.integers(128, 385))
        labels = rng.integers(3, 40, size=n)
        bg = rng.random(n) < 0.15
        labels[bg] = rng.integers(0, 3, size=int(bg.sum()))
        packed.add_scan(f"s{s}", rng.random((n, 3)).astype(np.float32), np.zeros((n, 3), np.uint8), np.arange(n),
                        list(range(n)), inst_labels=labels.tolist())
        scans.append(labels.tolist())
    packed.finalize()
    questions, items = PackedQuestions(dev), []
    for i in range(n_questions):
        s = int(rng.integers(n_scans))
        fg = [p for p, l in enumerate(scans[s]) if l >= 3]
        targets = [int(t) for t in rng.choice(fg, size=int(rng.integers(0, 4)), replace=False)]
        answers = [int(a) for a in rng.choice(A, size=int(rng.integers(0, 4)), replace=False)]
        questions.add_question(f"s{s}", targets, answers, texts=i)
        items.append((s, targets, answers))
    questions.finalize(packed)
    keep = G.keep_table(INT2CAT).to(dev)

    pick = rng.integers(0, n_questions, size=B)
    q_idx = torch.from_numpy(pick).to(device=dev, dtype=torch.int32)
    seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    kw = dict(O=O, n_answers=A, keep=keep, seed=7, seed_dev=seed_dev)
    out = qa_rows(packed, questions, q_idx, M, **kw)
    n_fill = int((out["n_rem"] > 0).sum())

    def call():
        qa_rows(packed, questions, q_idx, M, out=out, **kw)

    def host():
        parts = [host_item(scans[items[i][0]], items[i][1], items[i][2], M, A) for i in pick]
        up = [torch.from_numpy(np.stack(x)).to(dev) for x in zip(*parts)]
        torch.cuda.synchronize()
        return up
    up = host()
    same = all(torch.equal(a, b) for a, b in zip(up[2:], (out["tgt_object_id"], out["tgt_object_label"], out["answer_label"])))
    replay = captured(call, GRAPH_ITERS)
    for _ in range(10):
        replay()
        call()
    torch.cuda.synchronize()
    t_launch, t_call, t_host = [], [], []
    for _ in range(args.rounds):
        t_launch += [t / GRAPH_ITERS for t in event_samples(replay, args.samples)]
        t_call += event_samples(call, args.samples)
        t0 = time.perf_counter()
        host()
        t_host.append((time.perf_counter() - t0) * 1e6)
    sizes = [len(scans[items[i][0]]) for i in pick]
    nbytes = sum(t.numel() * t.element_size() for t in out.values())
    lines.append(f"[qa B={B} O={O} M={M} A={A}] scans of {min(sizes)} .. {max(sizes)} objects (mean {sum(sizes) / B:.0f}), "
                 f"{n_fill} rows take the random fill; outputs {nbytes} bytes per batch; host multi-hots == the launch's: {same}")
    lines.append(line("  gps_obj_select_qa, the launch alone (graph of 20, per launch)", t_launch))
    lines.append(line("  qa_rows(out=) eager, events around the call", t_call))
    lines.append(line("  host path (selection loop, multi-hots, stack, upload, synchronise), same batch (host clock)", t_host))
    lines.append(f"  host path / eager call = {statistics.median(t_host) / statistics.median(t_call):.1f}x; outputs over the launch "
                 f"= {nbytes / statistics.median(t_launch) / 1e3:.1f} GB/s")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
