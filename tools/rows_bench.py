"""Timing of the device-side object selection (csrc/gps_obj_select.hip, sceneverse_amd/data/gpu_objects.py: select_rows)
against the host loop it replaces.

    python tools/rows_bench.py [--rounds 5] [--samples 10] [--out profiles/rows/rows_bench.txt]

Batches: B = 64 and B = 256 'refer' rows, O = 80, M = 79, scans of 40 to 400 objects (about one in seven background),
the fill drawn on the device.  The three measurements ALTERNATE for `--rounds` rounds, so that a drift of the machine
meets all of them alike; per measurement the median over all its samples, with min and max:
  * the launch alone: 20 launches captured into one graph and replayed, divided by 20 (GPU time, no host launch path),
    `--samples` device-event windows per round;
  * the wrapper call as a loader makes it: `select_rows(out=static buffers)` eager, the range table, the targets and the
    keep table already on the device, `--samples` device-event windows per round;
  * the host loop: this tool's own restatement of the reference's per-sample selection (list comprehensions over the
    objects, `kobj not in selected_obj_idxs` on a list, `random.shuffle`) over the same batch, on this machine's CPU in
    one process, host clock, one batch per round.  It is not the reference's code, which is not on the GPU box."""
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

GRAPH_ITERS = 20
INT2CAT = ["wall", "floor", "ceiling"] + [f"cat{i}" for i in range(3, 40)]


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


def host_select(obj_labels, tgt_object_id, max_obj_len):
    """One item through the per-sample selection: filter, target-first crop, class-mates, shuffle of the rest."""
    selected = [i for i, l in enumerate(obj_labels) if INT2CAT[l] not in ["wall", "floor", "ceiling"]]
    if tgt_object_id not in selected:
        selected.append(tgt_object_id)
    labels = [obj_labels[i] for i in selected]
    tgt = selected.index(tgt_object_id)
    tgt_label = labels[tgt]
    rows = selected
    if max_obj_len < len(labels):
        picked = [tgt]
        remained = []
        for kobj, klabel in enumerate(labels):
            if kobj not in picked:
                if klabel == tgt_label:
                    picked.append(kobj)
                else:
                    remained.append(kobj)
            if len(picked) == max_obj_len:
                break
        if len(picked) < max_obj_len:
            random.shuffle(remained)
            picked += remained[:(max_obj_len - len(picked))]
        rows = [selected[i] for i in picked]
        tgt = 0
    return rows, tgt, sum(1 for l in obj_labels if l == tgt_label) > 1, sum(1 for l in obj_labels if l == tgt_label) > 2


def line(name, t):
    return f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rows_bench.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {args.rounds} alternating rounds, {args.samples} device-event "
             f"samples per round and measurement after warm-up; median [min .. max]; host CPUs visible: {os.cpu_count()}, "
             f"host loop in one process, one batch per round"]
    rng = np.random.default_rng(0)
    n_scans, M, O = 128, 79, 80
    packed, scans = G.PackedScans(dev), []
    for s in range(n_scans):
        n = int(rng.integers(40, 401))
        labels = rng.integers(3, len(INT2CAT), size=n)
        bg = rng.random(n) < 0.15
        labels[bg] = rng.integers(0, 3, size=int(bg.sum()))
        packed.add_scan(f"s{s}", rng.random((n, 3)).astype(np.float32), np.zeros((n, 3), np.uint8), np.arange(n),
                        list(range(n)), inst_labels=labels.tolist())
        scans.append(labels.tolist())
    packed.finalize()
    keep = G.keep_table(INT2CAT).to(dev)

    for B in (64, 256):
        pick = rng.integers(0, n_scans, size=B)
        sids = [f"s{s}" for s in pick]
        tgt_host = [int(rng.choice([i for i, l in enumerate(scans[s]) if l >= 3])) for s in pick]
        ranges = G.scan_ranges(packed, sids)
        tgt = torch.tensor(tgt_host, dtype=torch.int32, device=dev)
        seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        kw = dict(O=O, tgt_obj=tgt, keep=keep, seed=7, seed_dev=seed_dev)
        out = G.select_rows(packed, ranges, M, **kw)
        n_fill = int((out["n_rem"] > 0).sum())

        def call():
            G.select_rows(packed, ranges, M, out=out, **kw)
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
            for s, t in zip(pick, tgt_host):
                host_select(scans[s], t, M)
            t_host.append((time.perf_counter() - t0) * 1e6)
        sizes = [len(scans[s]) for s in pick]
        lines.append(f"[refer B={B} O={O} M={M}] scans of {min(sizes)} .. {max(sizes)} objects (mean {sum(sizes) / B:.0f}), "
                     f"{n_fill} rows take the random fill")
        lines.append(line("  gps_obj_select, the launch alone (graph of 20, per launch)", t_launch))
        lines.append(line("  select_rows(out=) eager, events around the call", t_call))
        lines.append(line("  host selection loop, same batch, this machine's CPU (host clock)", t_host))
        lines.append(f"  host loop / eager call = {statistics.median(t_host) / statistics.median(t_call):.1f}x")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
