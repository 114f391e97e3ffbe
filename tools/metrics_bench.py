"""Timing of the device-side evaluators (csrc/gps_metrics.hip): PretrainCounter / ReferIt3DCounter updates against the
torch composition of the same arithmetic, and the captured pre-train step with `train_metrics` on and off.

    python tools/metrics_bench.py [--rounds 7] [--out profiles/metrics/metrics_bench.txt] [--no-step]

Alternating windows, medians: every round times each form once, one after the other, so that a drift of the machine
hits all of them alike; the figure reported is the median over the rounds (min and max beside it).  A window is `iters`
calls captured into one graph and replayed (GPU time of the launches, not the host's launch path).  The reference's own
form -- boolean-mask indexing and one `.item()` per figure -- cannot be captured; it is timed eagerly with the host
clock around a synchronise, and so is the counters' `update` for the comparison in kind.  The "sync-free torch" form is
the same arithmetic written as arg-max / compare / and / sum on whole tensors, which can be captured.
Workloads: pre-train -- B = 64, 80 objects, 50 tokens, 30 522 words, 607 classes, bf16, the (B, L, V) logits materialised
(195 MB) with 15 % of the tokens labelled; the lazy path's extra launch -- the labelled-rows buffer of the fused loss
(3 200 rows of pitch 30 528, the labelled ones first); ReferIt3D -- B = 256, 80 objects, 607 classes; the step -- the
pre-train preset of bench.py at B = 64 in two engines of one process, one with `train_metrics=True`."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from sceneverse_amd.common import cls_hits  # noqa: E402
from sceneverse_amd.engine import PretrainCounter, ReferIt3DCounter  # noqa: E402


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


def _planted(shape, labels, dev, dtype, p=0.5):
    x = torch.randn(shape, device=dev, dtype=torch.float32).to(dtype)
    flat, lab = x.view(-1, shape[-1]), labels.reshape(-1)
    rows = torch.nonzero((torch.rand(lab.numel(), device=dev) < p) & (lab >= 0) & (lab < shape[-1])).reshape(-1)
    flat[rows, lab[rows]] = 9.0
    return x


def pretrain_batch(dev, B=64, O=80, L=50, V=30522, C=607, dtype=torch.bfloat16):
    torch.manual_seed(0)
    lm_labels = torch.where(torch.rand(B, L, device=dev) < 0.15, torch.randint(0, V, (B, L), device=dev), -1)
    obj_labels = torch.randint(0, C, (B, O), device=dev)
    tgt = torch.randint(0, O, (B, 1), device=dev)
    d = {"masked_lm_labels": lm_labels, "obj_labels": obj_labels, "tgt_object_id": tgt,
         "obj_masks": torch.arange(O, device=dev)[None, :] < torch.randint(20, O + 1, (B, 1), device=dev),
         "obj_sem_masks": torch.rand(B, O, device=dev) > 0.25,
         "og3d_logits": _planted((B, O), tgt, dev, dtype),
         "txt_lm_cls_logits": _planted((B, L, V), lm_labels, dev, dtype)}
    for k in ("post", "raw", "pre"):
        d[f"obj_cls_{k}_logits"] = _planted((B, O, C), obj_labels, dev, dtype)
    return d


def pretrain_reference_form(d):
    """PretrainEval.batch_metrics as the reference writes it: mask indexing, one or two `.item()` per figure."""
    m = {}
    tm = d["masked_lm_labels"] != -1
    m["og_acc"] = (torch.argmax(d["og3d_logits"], dim=-1) == d["tgt_object_id"].squeeze(1)).sum().item() / float(len(d["tgt_object_id"]))
    m["lang_cls_acc_mask"] = torch.sum(torch.argmax(d["txt_lm_cls_logits"], dim=2)[tm] == d["masked_lm_labels"][tm]).item() / float(
        tm.sum().item() + 1e-8)
    om, sem = d["obj_masks"], d["obj_sem_masks"]
    for key, split in (("obj_cls_post", True), ("obj_cls_raw", False), ("obj_cls_pre", True)):
        pred = torch.argmax(d[f"{key}_logits"], dim=2)
        sels = [("", om)] + ([("_unmask", om * sem), ("_mask", om * sem.logical_not())] if split else [])
        for suffix, s in sels:
            m[f"{key}_acc{suffix}"] = torch.sum(pred[s] == d["obj_labels"][s]).item() / float(s.sum().item() + 1e-8)
    m["target_metric"] = float(sum(m.values())) / len(m)
    return m


def pretrain_syncfree_torch(d, out):
    """The same counts as whole-tensor torch ops, written into `out` (18 int64): no indexing by mask, no `.item()`."""
    vals = [(torch.argmax(d["og3d_logits"], dim=-1) == d["tgt_object_id"].squeeze(1)).sum(), out.new_zeros(())]
    tm = d["masked_lm_labels"] != -1
    vals += [((torch.argmax(d["txt_lm_cls_logits"], dim=2) == d["masked_lm_labels"]) & tm).sum(), tm.sum()]
    om, sem = d["obj_masks"], d["obj_sem_masks"]
    for key, split in (("obj_cls_post", True), ("obj_cls_raw", False), ("obj_cls_pre", True)):
        hit = (torch.argmax(d[f"{key}_logits"], dim=2) == d["obj_labels"]) & om
        vals += [hit.sum(), om.sum()]
        if split:
            vals += [(hit & sem).sum(), (om & sem).sum()]
    out[:len(vals)] = torch.stack(vals)


def referit_batch(dev, B=256, O=80, C=607, dtype=torch.bfloat16):
    torch.manual_seed(1)
    tgt = torch.randint(0, O, (B, 1), device=dev)
    lab = torch.randint(0, C, (B, 1), device=dev)
    obj_labels = torch.randint(0, C, (B, O), device=dev)
    return {"tgt_object_id": tgt, "tgt_object_label": lab, "obj_labels": obj_labels,
            "is_hard": torch.rand(B, device=dev) < 0.5, "is_view_dependent": torch.rand(B, device=dev) < 0.3,
            "obj_masks": torch.arange(O, device=dev)[None, :] < torch.randint(20, O + 1, (B, 1), device=dev),
            "og3d_logits": _planted((B, O), tgt, dev, dtype), "txt_cls_logits": _planted((B, C), lab, dev, dtype),
            "obj_cls_post_logits": _planted((B, O, C), obj_labels, dev, dtype),
            "obj_cls_pre_logits": _planted((B, O, C), obj_labels, dev, dtype)}


def referit_reference_form(d):
    """ReferIt3DEval.batch_metrics(include_count=True), its `.item()` calls included."""
    m = {}
    pred = torch.argmax(d["og3d_logits"], dim=-1)
    total = len(pred)
    hard, dep = d["is_hard"].sum().item(), d["is_view_dependent"].sum().item()
    ok = d["tgt_object_id"].flatten() == pred
    correct = ok.sum().item()
    hc, dc = (ok & d["is_hard"]).sum().item(), (ok & d["is_view_dependent"]).sum().item()
    m.update({"og_acc_easy": (correct - hc, total - hard), "og_acc_hard": (hc, hard), "og_acc_view_dep": (dc, dep),
              "og_acc_view_indep": (correct - dc, total - dep),
              "og_acc": ((pred == d["tgt_object_id"].squeeze(1)).sum().item(), total),
              "txt_acc": ((torch.argmax(d["txt_cls_logits"], dim=1) == d["tgt_object_label"].squeeze(1)).sum().item(), total)})
    gt, mask = d["obj_labels"], d["obj_masks"]
    for key in ("obj_cls_post_logits", "obj_cls_pre_logits"):
        p = torch.argmax(d[key], dim=2)
        m[key.replace("logits", "acc")] = ((p[mask] == gt[mask]).sum().item(), mask.sum().item())
    return m


def step_windows(rounds, steps, lines):
    """The captured pre-train step of bench.py's preset, with and without train_metrics, alternating in one process."""
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.data.synthetic import synth_batch
    from sceneverse_amd.engine import GPSTrainStep
    dev = torch.device("cuda", 0)
    batch = synth_batch(64, seed=42, device=dev)
    engines = {}
    for name, tm in (("train_metrics off", False), ("train_metrics on", True)):
        e = GPSTrainStep(gps_pretrain_cfg(_lang_dir()), device=dev, ddp=False, graph=True, seed=4321, train_metrics=tm)
        for _ in range(e.graph_warmup + 3):
            e.step(dict(batch))
        torch.cuda.synchronize()
        engines[name] = e
    s, t = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    times = {name: [] for name in engines}
    for _ in range(rounds):
        for name, e in engines.items():
            s.record()
            for _ in range(steps):
                e.step(dict(batch))
            t.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(t) / steps)
    for name, v in times.items():
        lines.append(f"captured pre-train step, B = 64, {name}: {statistics.median(v):.3f} ms [{min(v):.3f} .. {max(v):.3f}] "
                     f"({steps} replays per window)")
    on = engines["train_metrics on"]
    lines.append("last step's train_metrics(): " + ", ".join(f"{k} {v.item():.4f}" for k, v in on.train_metrics().items()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-step", action="store_true", help="skip the captured training step")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; rounds {args.rounds}; median [min .. max]"]

    d = pretrain_batch(dev)
    counter = PretrainCounter(dev)
    counter.update(d)
    got, want = {k: v.item() for k, v in counter.last().items()}, pretrain_reference_form(d)
    assert got == want, (got, want)
    lines.append("PretrainCounter.update equals the reference form on the same tensors, bit for bit: "
                 + ", ".join(f"{k} {v:.4f}" for k, v in got.items()))
    sync_out = torch.zeros(18, dtype=torch.int64, device=dev)
    # the lazy path's extra launch: the labelled rows of the fused loss (first n_valid rows of 3 200, pitch 30 528)
    n, V, Vp = 64 * 50, 30522, 30528
    lp = d["masked_lm_labels"].reshape(-1)
    order = torch.argsort((lp == -1).to(torch.int8), stable=True)
    lp = lp[order].contiguous()
    n_valid = (lp != -1).sum().to(torch.int32).reshape(1)
    rows_buf = torch.zeros((n, Vp), dtype=torch.bfloat16, device=dev)
    rows_buf[:, :V] = d["txt_lm_cls_logits"].reshape(n, V)[order]
    words = torch.zeros(6, dtype=torch.int64, device=dev)

    def run_lazy():
        cls_hits.launch([cls_hits.problem(rows_buf, lp, words, ignore_index=-1, rows_dev=n_valid, cols=V)], dev)
    run_lazy()
    full = PretrainCounter(dev, keys=["lang_cls_acc_mask"])
    full.update(d)
    assert words.tolist()[:2] == [round(full.last()["lang_cls_acc_mask"].item() * int(n_valid)), int(n_valid)]
    live_mb = int(n_valid) * V * 2 / 1e6

    r = referit_batch(dev)
    rc = ReferIt3DCounter(dev)
    rc.update(r)
    assert rc.result(include_count=True) == referit_reference_form(r)
    lines.append("ReferIt3DCounter.update equals the reference form on the same tensors: "
                 + ", ".join(f"{k} {h}/{c}" for k, (h, c) in rc.result(include_count=True).items()))

    windows = [("PretrainCounter.update (materialised logits), graph replay", graph_window(lambda: counter.update(d), 20)),
               ("sync-free torch composition of the same counts, graph replay", graph_window(lambda: pretrain_syncfree_torch(d, sync_out), 20)),
               (f"gps_cls_hits on the fused loss's labelled rows ({int(n_valid)} of {n} live, {live_mb:.1f} MB), graph replay",
                graph_window(run_lazy, 50)),
               ("PretrainCounter.update, eager host clock", eager_window(lambda: counter.update(d), 50)),
               ("reference form (mask indexing, .item()), eager host clock", eager_window(lambda: pretrain_reference_form(d), 50)),
               ("ReferIt3DCounter.update, B = 256, graph replay", graph_window(lambda: rc.update(r), 50)),
               ("ReferIt3DCounter.update, B = 256, eager host clock", eager_window(lambda: rc.update(r), 200)),
               ("ReferIt3D reference form (.item()), B = 256, eager host clock", eager_window(lambda: referit_reference_form(r), 200))]
    times = {name: [] for name, _ in windows}
    for _ in range(args.rounds):
        for name, run in windows:
            times[name].append(run())
    for name, _ in windows:
        t = times[name]
        lines.append(f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]")
    if not args.no_step:
        step_windows(args.rounds, 10, lines)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
