"""Time the device-side ScanQA answer counter against the torch forms it replaces.

    python tools/answers_bench.py --out profiles/qa/answers_bench.json

(a) `update`: ScanQACounter.update (gps_answer_hits + gps_answer_fold) on bf16 scores at V = 8864, B = 64 and 256, against
    the SYNC-FREE torch composition of the same arithmetic (argmax, topk, two gathers, sums added into device words) --
    each captured in a graph of its own.
(b) the captured ScanQA fine-tune step of tools/qa_bench.py at B = 64 in three forms:
      in_graph   GPSTrainStep(train_metrics="scanqa"): the counter's launches replay inside the step's graph
      off        no metrics
      after      no metrics in the graph, `engine.scanqa_accuracy` on the step's scores after every replay (its `.item()`
                 read-backs included): what a trainer that wants per-step metrics does without the counter
    `off` and `after` share one engine, whose metric counter is a stand-in that launches nothing and only keeps the
    step's static score / label tensors.
Every figure: windows of `--steps` replays bracketed by device events, the forms alternating, `--rounds` windows each;
the median window and the spread (max - min) of the windows are reported per replay.  No GPU: the script fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from tools.qa_bench import qa_cfg  # noqa: E402


def _windows(forms, steps, rounds, scale=1e3):
    """forms: {name: callable running ONE replay} -> {name: per-replay times of `rounds` alternating windows}."""
    ts = {k: [] for k in forms}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(rounds):
        for k, f in forms.items():
            torch.cuda.synchronize()
            e0.record()
            for _ in range(steps):
                f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(scale * e0.elapsed_time(e1) / steps)
    return ts


def _summary(ts, unit):
    return {k: {f"{unit}_per_window": [round(t, 3) for t in v], f"{unit}_median": round(statistics.median(v), 3),
                f"{unit}_spread": round(max(v) - min(v), 3)} for k, v in ts.items()}


def _capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def bench_update(args, dev):
    from sceneverse_amd.engine import ScanQACounter
    out = {}
    for B in args.update_batches:
        gen = torch.Generator().manual_seed(B)
        scores = torch.randn(B, args.answers, generator=gen).to(dev, torch.bfloat16)
        label = (torch.rand(B, args.answers, generator=gen) < 2e-4).long().to(dev)
        d = {"answer_scores": scores, "answer_label": label}
        counter = ScanQACounter(dev)
        sums = torch.zeros(3, dtype=torch.int64, device=dev)

        def composed():
            top1 = scores.argmax(dim=-1, keepdim=True)
            topk = torch.topk(scores, 10, -1)[1]
            hit1 = torch.gather(label, 1, top1).squeeze(1) == 1
            hitk = (torch.gather(label, 1, topk) == 1).any(dim=1)
            sums.add_(torch.stack([hit1.sum(), hitk.sum(), torch.ones_like(hit1).sum()]))

        graphs = {"torch": _capture(composed), "native": _capture(lambda: counter.update(d))}
        ts = _windows({k: g.replay for k, g in graphs.items()}, args.steps, args.rounds)
        r = _summary(ts, "us")
        r["native_over_torch"] = round(r["native"]["us_median"] / r["torch"]["us_median"], 4)
        r["shape"] = [B, args.answers]
        out[f"B{B}"] = r
    return out


class _Keep:
    """A stand-in metric counter: no launch, it only keeps the step's (static) scores and labels."""
    scores = label = None

    def update(self, out):
        self.scores, self.label = out["answer_scores"].detach(), out["answer_label"]

    def last(self):
        return {}


def bench_step(args, dev):
    from sceneverse_amd.data.synthetic import synth_qa_batch
    from sceneverse_amd.engine import GPSTrainStep, scanqa_accuracy
    batch = synth_qa_batch(args.batch, n_obj=args.objects, n_pts=args.points, txt_len=args.tokens, n_answers=args.answers,
                           seed=42, device=dev)
    keep = _Keep()
    engines = {}
    for name, tm in (("in_graph", "scanqa"), ("off", keep)):
        st = GPSTrainStep(qa_cfg(args.answers), device=dev, ddp=False, graph=True, graph_warmup=2, seed=7, train_metrics=tm)
        for _ in range(2 + 1 + args.warmup):            # eager warm-up, capture, replays
            st.step(dict(batch))
        torch.cuda.synchronize()
        assert st._graph is not None
        engines[name] = st
    seen = []

    def after():
        engines["off"].step(dict(batch))
        seen.append(scanqa_accuracy(keep.scores, keep.label))

    forms = {"in_graph": lambda: engines["in_graph"].step(dict(batch)), "off": lambda: engines["off"].step(dict(batch)),
             "after": after}
    r = _summary(_windows(forms, args.steps, args.rounds, scale=1.0), "ms")
    r["in_graph_minus_after_ms"] = round(r["in_graph"]["ms_median"] - r["after"]["ms_median"], 3)
    r["in_graph_minus_off_ms"] = round(r["in_graph"]["ms_median"] - r["off"]["ms_median"], 3)
    r["train_metrics_last"] = {k: v.item() for k, v in engines["in_graph"].train_metrics().items()}
    r["after_last"] = seen[-1]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--update-batches", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--objects", type=int, default=80)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=50)
    ap.add_argument("--answers", type=int, default=8864)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("answers_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = {"config": vars(args), "device": torch.cuda.get_device_name(0), "update": bench_update(args, dev)}
    if not args.skip_step:
        res["step"] = bench_step(args, dev)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
