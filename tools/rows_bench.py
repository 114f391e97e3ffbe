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
    one process, host clock, one batch per round.  It is not the reference's code, which is not on the GPU box.

    python tools/rows_bench.py --pred [--out profiles/rows/pred_rows_bench.txt]

The selection of predicted proposals (csrc/gps_obj_select_pred.hip, select_rows(pc_type="pred")): B = 64 and B = 256 rows,
O = 80, M = 79, scans of 20 annotated objects and 40 to 400 proposals (trimmed copies of the objects), the fill drawn on the
device.  Alternating rounds as above:
  * gps_obj_select_pred WITH its four target outputs, the launch alone (graph of 20, per launch);
  * the chain it replaces on the device: gps_obj_select_pred without targets, then gps_refer_targets('pred') on its rows
    (graph of 20 pairs, per pair);
  * `select_rows(pc_type="pred", targets=True, out=)` eager, device events around the call;
  * the host loop: this tool's own restatement of the reference's per-sample work on plain Python floats -- the matching
    loop over proposals x annotated objects, the two IoU passes against the target, the crop with `random.shuffle` --
    over the same batch, host clock, in the first `--host-rounds` rounds only (it takes seconds)."""
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


def host_iou(a, b):
    """box3d_iou on (lo x, y, z, hi x, y, z) tuples of Python floats."""
    dx, dy, dz = min(a[3], b[3]) - max(a[0], b[0]), min(a[4], b[4]) - max(a[1], b[1]), min(a[5], b[5]) - max(a[2], b[2])
    inter = max(dx, 0.0) * max(dy, 0.0) * max(dz, 0.0)
    va = (a[3] - a[0]) * (a[4] - a[1]) * (a[5] - a[2])
    vb = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2])
    return inter / (va + vb - inter + 1e-8)


def host_select_pred(ann_boxes, ann_labels, prop_boxes, prop_labels, tgt, max_obj_len):
    """One 'pred' item through the per-sample work: relabel by the first match, flag lists, crop."""
    obj_labels = list(prop_labels)
    for i, pb in enumerate(prop_boxes):
        for j, ab in enumerate(ann_boxes):
            if host_iou(ab, pb) >= 0.25:
                obj_labels[i] = ann_labels[j]
                break
    gt = ann_boxes[tgt]
    tgt_id, l25, l50 = -1, [], []
    for i, pb in enumerate(prop_boxes):
        if host_iou(pb, gt) >= 0.25:
            tgt_id = i
            l25.append(i)
    for i, pb in enumerate(prop_boxes):
        if host_iou(pb, gt) >= 0.5:
            l50.append(i)
    selected = list(range(len(prop_boxes)))
    if max_obj_len < len(prop_boxes):
        if tgt_id != -1:
            selected = [tgt_id]
        selected.extend(l25)
        selected.extend(l50)
        selected = list(set(selected))
        remained = []
        for kobj, klabel in enumerate(obj_labels):
            if kobj not in selected:
                if klabel == ann_labels[tgt]:
                    selected.append(kobj)
                else:
                    remained.append(kobj)
            if len(selected) == max_obj_len:
                break
        if len(selected) < max_obj_len:
            random.shuffle(remained)
            selected += remained[:(max_obj_len - len(selected))]
        selected = selected[:max_obj_len]
    return selected, tgt_id


def main_pred(args):
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {args.rounds} alternating rounds, {args.samples} device-event "
             f"samples per round and measurement after warm-up; median [min .. max]; host CPUs visible: {os.cpu_count()}, "
             f"host loop in one process, one batch in each of the first {args.host_rounds} rounds"]
    rng = np.random.default_rng(0)
    n_scans, n_ann, M, O, levels = 128, 20, 79, 80, 8
    # every scan: 20 unit cubes side by side, each with its two corners and the corner points of its trimmed copies
    pts, inst = [], []
    for j in range(n_ann):
        for k in range(levels + 1):
            pts += [(2.0 * j, 0.0, k / levels), (2.0 * j + 1.0, 1.0, k / levels)]
            inst += [j, j]
    pts, inst = np.asarray(pts, dtype=np.float32), np.asarray(inst)
    colors = np.zeros((len(pts), 3), np.uint8)
    packed, scans = G.PackedScans(dev), []
    for s in range(n_scans):
        P = int(rng.integers(40, 401))
        ann_labels = rng.integers(3, len(INT2CAT), size=n_ann).tolist()
        obj, lev = rng.integers(0, n_ann, size=P), rng.integers(1, levels + 1, size=P)
        masks = (inst[None, :] == obj[:, None]) & (pts[None, :, 2] <= (lev[:, None] / levels).astype(np.float32))
        prop_labels = rng.integers(3, len(INT2CAT), size=P).tolist()
        packed.add_scan(f"s{s}", pts, colors, inst, list(range(n_ann)), inst_labels=ann_labels)
        packed.add_proposals(f"s{s}", pts, colors, masks, prop_labels)
        scans.append({"ann_boxes": [(2.0 * j, 0.0, 0.0, 2.0 * j + 1.0, 1.0, 1.0) for j in range(n_ann)], "ann_labels": ann_labels,
                      "prop_boxes": [(2.0 * int(j), 0.0, 0.0, 2.0 * int(j) + 1.0, 1.0, int(k) / levels) for j, k in zip(obj, lev)],
                      "prop_labels": prop_labels})
    packed.finalize()

    for B in (64, 256):
        pick = rng.integers(0, n_scans, size=B)
        sids = [f"s{s}" for s in pick]
        tgt_host = [int(t) for t in rng.integers(0, n_ann, size=B)]
        tabs = (G.scan_ranges(packed, sids), G.scan_ranges(packed, sids, proposals=True))
        tgt = torch.tensor(tgt_host, dtype=torch.int32, device=dev)
        seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        kw = dict(O=O, tgt_obj=tgt, pc_type="pred", seed=7, seed_dev=seed_dev)
        out = G.select_rows(packed, tabs, M, targets=True, **kw)
        rows_only = {k: out[k] for k in ("row_obj", "tgt_slot", "n_sel", "n_rem", "is_multiple", "is_hard")}
        tout = {k: torch.empty_like(out[k]) for k in ("tgt_object_id_iou25", "tgt_object_id_iou50", "tgt_object_id", "obj_labels")}
        n_fill, n_hit = int((out["n_rem"] > 0).sum()), int((out["tgt_slot"] >= 0).sum())

        def fused():
            G.select_rows(packed, tabs, M, targets=True, out=out, **kw)

        def chain():
            G.select_rows(packed, tabs, M, out=rows_only, **kw)
            G.refer_targets(packed, rows_only["row_obj"], tgt, tabs[0], "pred", out=tout)
        chain()
        torch.cuda.synchronize()
        same = all(torch.equal(out[k], tout[k]) for k in tout)
        replay_fused, replay_chain = captured(fused, GRAPH_ITERS), captured(chain, GRAPH_ITERS)
        for _ in range(10):
            replay_fused()
            replay_chain()
            fused()
        torch.cuda.synchronize()
        t_fused, t_chain, t_call, t_host = [], [], [], []
        for r in range(args.rounds):
            t_fused += [t / GRAPH_ITERS for t in event_samples(replay_fused, args.samples)]
            t_chain += [t / GRAPH_ITERS for t in event_samples(replay_chain, args.samples)]
            t_call += event_samples(fused, args.samples)
            if r < args.host_rounds:
                t0 = time.perf_counter()
                for s, t in zip(pick, tgt_host):
                    d = scans[s]
                    host_select_pred(d["ann_boxes"], d["ann_labels"], d["prop_boxes"], d["prop_labels"], t, M)
                t_host.append((time.perf_counter() - t0) * 1e6)
        sizes = [len(scans[s]["prop_boxes"]) for s in pick]
        lines.append(f"[pred B={B} O={O} M={M}] scans of {n_ann} annotated objects and {min(sizes)} .. {max(sizes)} proposals (mean "
                     f"{sum(sizes) / B:.0f}); {n_hit} rows have a hit at 0.25, {n_fill} take the random fill; fused targets == "
                     f"gps_refer_targets on the same rows: {same}")
        lines.append(line("  gps_obj_select_pred with targets, the launch alone (graph of 20, per launch)", t_fused))
        lines.append(line("  gps_obj_select_pred without targets + gps_refer_targets (graph of 20 pairs, per pair)", t_chain))
        lines.append(line("  select_rows(pc_type='pred', targets=True, out=) eager, events around the call", t_call))
        if t_host:
            lines.append(line("  host loop (matching, flags, crop), same batch, this machine's CPU (host clock)", t_host))
            lines.append(f"  host loop / eager call = {statistics.median(t_host) / statistics.median(t_call):.1f}x")
    return lines


def line(name, t):
    return f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--pred", action="store_true", help="the selection of predicted proposals (gps_obj_select_pred)")
    ap.add_argument("--host-rounds", type=int, default=2, help="--pred: rounds in which the host loop runs too")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "rows_bench.py measures on a GPU"
    if args.pred:
        return write(main_pred(args), args.out)
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
    write(lines, args.out)


def write(lines, path):
    text = "\n".join(lines)
    print(text, flush=True)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
