"""Timing of the ScanRefer target path (csrc/gps_refer.hip): gps_obj_boxes, gps_refer_targets, gps_refer_metrics.

    python tools/refer_bench.py [--rounds 7] [--out profiles/refer/refer_bench.txt]

Alternating windows, medians: every round times each launch once, one after the other, so that a drift of the machine
hits all of them alike; the figure reported is the median over the rounds (min and max beside it).  A window is `iters`
calls captured into one graph and replayed (GPU time of the launches, not the host's launch path); what cannot be
captured -- `scanrefer_accuracy`, which reads its counts back -- is timed eagerly with the host clock around a
synchronise, and so is `ScanReferCounter.update` for the comparison in kind.
Workloads: boxes -- 64 scans x 80 objects, sizes log-uniform 50..20 000 points (the population of
tools/kernel_bench.py --objects-only) plus one 300 000-point object; targets / metrics -- B = 256, O = 80, 50 proposals
and 60 annotated objects per scan."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sceneverse_amd import _native  # noqa: E402
from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.engine import ScanReferCounter, scanrefer_accuracy  # noqa: E402


def graph_window(fn, iters):
    """-> a callable that replays `iters` captured calls and returns the GPU time of one call in us."""
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(iters):
            fn()
    g.replay()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def run():
        s.record()
        g.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3 / iters
    return run


def eager_window(fn, iters):
    def run():
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e6 / iters
    fn()
    return run


def boxes_population(dev):
    rng = np.random.default_rng(0)
    packed = G.PackedScans(dev)
    for s in range(64):
        ks = np.exp(rng.uniform(np.log(50), np.log(20000), size=80)).astype(np.int64)
        n = int(ks.sum())
        packed.add_scan(f"s{s}", rng.normal(size=(n, 3)).astype(np.float32), rng.integers(0, 256, size=(n, 3), dtype=np.uint8),
                        np.repeat(np.arange(80), ks), list(range(80)))
    packed.add_scan("floor", rng.normal(size=(300000, 3)).astype(np.float32),
                    rng.integers(0, 256, size=(300000, 3), dtype=np.uint8), np.zeros(300000, np.int64), [0])
    return packed.finalize()


def refer_population(dev, n_scans=16, n_gt=60, n_prop=50):
    rng = np.random.default_rng(1)
    packed = G.PackedScans(dev)
    for s in range(n_scans):
        ks = rng.integers(100, 400, size=n_gt)
        lo = rng.uniform(-4, 4, size=(n_gt, 3))
        pts = np.concatenate([rng.uniform(size=(k, 3)) * rng.uniform(0.3, 1.5, size=3) + lo[j] for j, k in enumerate(ks)])
        pts = pts.astype(np.float32)
        inst = np.repeat(np.arange(n_gt), ks)
        col = rng.integers(0, 256, size=(len(pts), 3), dtype=np.uint8)
        packed.add_scan(f"s{s}", pts, col, inst, list(range(n_gt)), inst_labels=rng.integers(3, 607, size=n_gt).tolist())
        cut = rng.uniform(0.1, 1.0, size=n_prop)
        masks = np.stack([(inst == q % n_gt) & (pts[:, 2] <= lo[q % n_gt, 2] + cut[q] * (pts[inst == q % n_gt, 2].max() - lo[q % n_gt, 2]))
                          for q in range(n_prop)])
        packed.add_proposals(f"s{s}", pts, col, masks, rng.integers(3, 607, size=n_prop).tolist())
    return packed.finalize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "refer_bench.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lib = _native.load()
    stream = lambda: torch.cuda.current_stream(dev).cuda_stream  # noqa: E731
    lines = [f"device: {torch.cuda.get_device_name(dev)}; rounds {args.rounds}; median [min .. max]"]

    big = boxes_population(dev)
    work = torch.from_numpy(G.boxes_work_list(big.sizes_host)).to(dev)
    ws = torch.empty(big.n_objects * 6, dtype=torch.int32, device=dev)
    boxes = torch.empty((big.n_objects, 6), dtype=torch.float64, device=dev)
    n_pts = int(big.xyz.shape[0])

    def run_boxes():
        _native.check(lib.gps_obj_boxes(big.n_objects, n_pts, int(work.shape[0]), big.xyz.data_ptr(), 1, work.data_ptr(),
                                        ws.data_ptr(), boxes.data_ptr(), stream()), "obj_boxes")
    run_boxes()
    assert torch.equal(boxes, big.boxes)
    box_bytes = n_pts * 16 + big.n_objects * 48 + int(work.shape[0]) * 24

    B, O = args.batch, 80
    small = refer_population(dev)
    sids = [f"s{i % 16}" for i in range(B)]
    rows = G.batch_rows(small, sids, O, proposals=True).to(dev)
    tgt = torch.from_numpy(np.random.default_rng(2).integers(0, 60, size=B)).to(dev)
    out = {"tgt_object_id_iou25": torch.empty((B, O), dtype=torch.int64, device=dev),
           "tgt_object_id_iou50": torch.empty((B, O), dtype=torch.int64, device=dev),
           "tgt_object_id": torch.empty((B, 1), dtype=torch.int64, device=dev),
           "obj_labels": torch.empty((B, O), dtype=torch.int64, device=dev)}
    ranges = torch.tensor([[small.scan_objects(s).start, small.scan_objects(s).stop] for s in sids], dtype=torch.int32, device=dev)
    tgt_g = (tgt.int() + ranges[:, 0]).contiguous()

    def run_targets():                           # the launch alone; refer_targets() adds one small upload per batch
        _native.check(lib.gps_refer_targets(B, O, small.n_objects, 0, small.boxes.data_ptr(), small.labels.data_ptr(),
                                            rows.data_ptr(), tgt_g.data_ptr(), ranges.data_ptr(),
                                            out["tgt_object_id_iou25"].data_ptr(), out["tgt_object_id_iou50"].data_ptr(),
                                            out["tgt_object_id"].data_ptr(), out["obj_labels"].data_ptr(), stream()),
                      "refer_targets")
    run_targets()
    check = G.refer_targets(small, rows, tgt, sids, "pred")
    assert all(torch.equal(check[k], out[k]) for k in out)
    batch = dict(out, is_multiple=(torch.arange(B, device=dev) % 3 == 0).to(torch.uint8))
    logits = torch.randn(B, O, device=dev)
    logits[torch.arange(0, B, 2, device=dev), out["tgt_object_id"].reshape(-1)[::2].clamp(max=O - 1)] = 9.0
    counter = ScanReferCounter(dev)

    def run_update():
        counter.update(logits, batch)

    def run_accuracy():
        return scanrefer_accuracy(logits, batch["tgt_object_id_iou25"], batch["tgt_object_id_iou50"])

    # one update in a graph: capture succeeds only because nothing in it waits for the device
    counter.reset()
    run_update()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run_update()
    g.replay()
    got, want = counter.result(), run_accuracy()
    assert got["og_acc_iou25"] == want["og_acc_iou25"] and got["og_acc_iou50"] == want["og_acc_iou50"], (got, want)
    lines.append(f"ScanReferCounter.update captured in a graph and replayed: counts equal scanrefer_accuracy "
                 f"(acc@0.25 {got['og_acc_iou25']:.4f}, acc@0.5 {got['og_acc_iou50']:.4f}) -> no host sync in update")

    windows = [("gps_obj_boxes, graph replay", graph_window(run_boxes, 10)),
               ("gps_refer_targets, graph replay", graph_window(run_targets, 50)),
               ("gps_refer_metrics (ScanReferCounter.update), graph replay", graph_window(run_update, 50)),
               ("ScanReferCounter.update, eager host clock", eager_window(run_update, 200)),
               ("scanrefer_accuracy (torch, 2 x .item()), eager host clock", eager_window(run_accuracy, 200))]
    times = {name: [] for name, _ in windows}
    for _ in range(args.rounds):
        for name, run in windows:
            times[name].append(run())
    for name, _ in windows:
        t = times[name]
        line = f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]"
        if name.startswith("gps_obj_boxes"):
            gbps = box_bytes / statistics.median(t) / 1e3
            line += (f"; {big.n_objects} objects, {n_pts} points, {int(work.shape[0])} chunks, {box_bytes / 1e6:.1f} MB "
                     f"-> {gbps:.0f} GB/s = {gbps / 8000:.3f} of 8 TB/s")
        elif "targets" in name or "metrics" in name:
            line += f"; B = {B}, O = {O}, 50 proposals, 60 annotated objects per scan"
        lines.append(line)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
