"""Timing of a pre-train batch's input pipeline: the host path of today against the captured chain of
sceneverse_amd/data/gpu_batch.py (`pretrain_batch`).

    python tools/loader_bench.py [--batch 64] [--rounds 3] [--samples 10] [--out profiles/loader/loader_bench.json]

Batch: B = 64 items, O = 80 slots (max_keep 79), 1024 points per object, the published `data_aug:` block (one of four
z-rotations per scene), `pc_type: 'gt'`, masked texts of 50 / 300 tokens; 32 synthetic scans of 40 to 120 objects of 200
to 4000 points (uint8 colours, 16-byte records).  Both paths produce the same tensors into the same static buffers.
  * host: what a loader does per batch today -- `draw_aug_params` (numpy loops) + `AugParams.to_device` (table, upload),
    the items' scan ids, target positions and caption picks looked up in Python lists, their tables uploaded, then the
    four calls `select_rows`, `refer_targets`, `obj_processing_aug`, `text_batch` with `out=`; host clock around work that
    ends in a device synchronise.
  * captured: `pretrain_batch(out=)` captured once in a HIP graph together with `seed_dev.add_(1)`; one replay per
    sample, device events around the replay (GPU time) and the host clock around replay + synchronise.
The two ALTERNATE for `--rounds` windows, so that a drift of the machine meets both alike; per window the median of
`--samples` samples, reported per window and as the median of the windows.  One process, one GPU, nothing else timed.
A record, not a pass criterion."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from sceneverse_amd.data import gpu_objects as G  # noqa: E402
from sceneverse_amd.data.gpu_batch import pretrain_batch  # noqa: E402
from sceneverse_amd.data.gpu_items import PackedItems  # noqa: E402
from sceneverse_amd.data.gpu_text import text_batch  # noqa: E402
from sceneverse_amd.data.synthetic import synth_packed_texts  # noqa: E402

PUBLISHED = {
    "aug_list": ["scene_aug"],
    "scene_aug": {
        "translation": {"enabled": False, "value": [1.0, 1.0, 1.0], "p": 1.0},
        "scaling": {"enabled": False, "p": 1.0, "value": [0.9, 1.1]},
        "flip": {"enabled": False, "p": 0.5},
        "rotation": {"enabled": True, "p": 1.0, "axis_align": True, "value": [0.0, 0.0, 1.0], "shuffle": True},
        "color_jitter": False,
        "order_shuffle": False,
    },
}
N_LABELS, N_SCANS, N_ITEMS, N_SENT, N_CAP = 607, 32, 4096, 4096, 128


def build(dev, seed=0):
    rng = np.random.default_rng(seed)
    packed = G.PackedScans(dev)
    for s in range(N_SCANS):
        n_obj = int(rng.integers(40, 121))
        ks = rng.integers(200, 4001, n_obj)
        pts = rng.normal(size=(int(ks.sum()), 3)).astype(np.float32)
        col = rng.integers(0, 256, (int(ks.sum()), 3)).astype(np.uint8)
        lab = np.repeat(np.arange(n_obj), ks)
        pts += (lab[:, None] % 7).astype(np.float32)
        packed.add_scan(f"scan{s}", pts, col, lab, list(range(n_obj)), inst_labels=rng.integers(3, N_LABELS, n_obj).tolist())
    packed.finalize()
    texts = synth_packed_texts(N_SENT, N_CAP, seed=seed, device=dev)
    items = PackedItems(packed, default_caption=N_SENT)
    host = []
    for i in range(N_ITEMS):
        s = int(rng.integers(N_SCANS))
        sid = f"scan{s}"
        t = int(rng.integers(len(packed.scan_objects(sid))))
        items.add_item(sid, t, int(packed._labels[packed.scan_objects(sid).start + t]), i % N_SENT)
        host.append((sid, t, i % N_SENT))
    caps = {}
    for s in range(N_SCANS):
        caps[f"scan{s}"] = [N_SENT + int(c) for c in rng.integers(0, N_CAP, 4)]
        items.set_captions(f"scan{s}", caps[f"scan{s}"])
    return packed, texts, items.finalize(), host, caps


def median_window(samples):
    return statistics.median(samples)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--slots", type=int, default=80)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--samples", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loader", "loader_bench.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", torch.cuda.current_device())
    B, O, P, M = a.batch, a.slots, a.points, a.slots - 1
    packed, texts, items, host_items, caps = build(dev)
    keep = G.keep_table(["wall", "floor", "ceiling"] + [f"cat{i}" for i in range(3, N_LABELS)]).to(dev)
    rng = np.random.default_rng(1)
    seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    ids = torch.from_numpy(rng.integers(0, N_ITEMS, B).astype(np.int32)).to(dev)
    kw = dict(O=O, num_points=P, pc_type="gt", aug_cfg=PUBLISHED, keep=keep)
    out = pretrain_batch(packed, texts, items, ids, M, seed=7, seed_dev=seed_dev, **kw)      # the static buffers
    torch.cuda.synchronize()

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        seed_dev.add_(1)
        pretrain_batch(packed, texts, items, ids, M, seed=7, seed_dev=seed_dev, out=out, **kw)

    def captured_sample():
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        s.record()
        graph.replay()
        e.record()
        torch.cuda.synchronize()
        return s.elapsed_time(e) * 1e3, (time.perf_counter() - t0) * 1e6

    def host_sample(step):
        batch = rng.integers(0, N_ITEMS, B)
        t0 = time.perf_counter()
        aug = G.draw_aug_params(PUBLISHED, "train", B, O, rng).to_device(B, O, dev)
        sids = [host_items[i][0] for i in batch]
        tgt = [host_items[i][1] for i in batch]
        sent = [host_items[i][2] for i in batch]
        cap = [caps[s][int(rng.integers(len(caps[s])))] for s in sids]
        ranges = G.scan_ranges(packed, sids)
        tgt_d = torch.tensor(tgt, dtype=torch.int32).to(dev)
        sel = G.select_rows(packed, ranges, M, O, tgt_obj=tgt_d, mode="refer", keep=keep, seed=step, out=out)
        G.refer_targets(packed, sel["row_obj"], tgt_d, ranges, "gt", out=out)
        obj = G.obj_processing_aug(packed, sel["row_obj"], P, aug=aug, seed=step, out=out)
        text_batch(texts, torch.tensor(sent, dtype=torch.int32).to(dev), torch.tensor(cap, dtype=torch.int32).to(dev),
                   obj_masks=obj["obj_masks"], seed=step, out=out)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6

    for _ in range(3):                             # warm both paths
        captured_sample()
        host_sample(0)
    windows = {"captured_gpu_us": [], "captured_wall_us": [], "host_wall_us": []}
    for r in range(a.rounds):
        cap_s = [captured_sample() for _ in range(a.samples)]
        windows["captured_gpu_us"].append(median_window([g for g, _ in cap_s]))
        windows["captured_wall_us"].append(median_window([w for _, w in cap_s]))
        windows["host_wall_us"].append(median_window([host_sample(r * a.samples + i + 1) for i in range(a.samples)]))
    res = {"what": "pre-train batch input pipeline: host path of today vs the captured pretrain_batch chain",
           "device": torch.cuda.get_device_name(dev), "B": B, "O": O, "num_points": P,
           "config": "published (scene_aug: one of four z-rotations)", "pc_type": "gt", "rounds": a.rounds,
           "samples_per_window": a.samples,
           "windows": windows, "median_of_windows": {k: statistics.median(v) for k, v in windows.items()},
           "bytes_out_obj_fts": B * O * P * 24}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
