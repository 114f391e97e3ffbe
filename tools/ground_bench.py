"""Time the grounding fine-tune step and the native head / loss ops against the torch compositions they replace.

    python tools/ground_bench.py --out profiles/ground/ground_bench.json

Step: bench.py's `finetune` workload (finetune/scanrefer_finetune.yaml's model: GroundHeadV1 768 / 384 / 607, og3d_loss)
at B = 256, 80 objects x 1024 points, 50 tokens, bf16 autocast, HIP-graph replay.  Five engines live in one process:
"torch" = set_ground_backend("torch") and `_FUSED_OG3D = False` (the behaviour before the native grounding path),
"native" = set_ground_backend("hip") and the fused loss, and three in between that add one native piece at a time to
the og3d head (VARIANTS).  Each is captured under its own setting (a replay no longer consults the switches), then timed
windows of `--steps` replays alternate between them, `--rounds` times; the host clock brackets a window that ends in a
device synchronise.  Reported: the median of the windows and their spread (max - min) for every engine -- the spread
between repeated windows of the same code is what a difference of medians has to exceed (`pieces`).  Ops: the og3d head
(forward + backward), a class head (forward) and og3d_loss (forward + backward) on the step's shapes, single eager calls
bracketed by device events, alternating.  No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


# engine variants of the step comparison: (backend, pieces "auto" runs natively, fused og3d loss)
VARIANTS = {
    "torch": ("torch", None, False),
    "og3d_head": ("auto", dict(og3d_head=True, class_heads=False), False),
    "og3d_head+class_heads": ("auto", dict(og3d_head=True, class_heads=True), False),
    "og3d_head+loss": ("auto", dict(og3d_head=True, class_heads=False), True),
    "native": ("hip", None, True),
}


def set_variant(name: str) -> None:
    from sceneverse_amd.modules.heads import grounding_head
    from sceneverse_amd.optim.loss import loss
    backend, pieces, fused = VARIANTS[name]
    grounding_head.set_ground_backend(backend)
    if pieces:
        grounding_head.set_ground_auto(**pieces)
    loss._FUSED_OG3D = bool(fused)


def set_mode(native: bool) -> None:
    set_variant("native" if native else "torch")


def restore_defaults(saved) -> None:
    from sceneverse_amd.modules.heads import grounding_head
    from sceneverse_amd.optim.loss import loss
    grounding_head.set_ground_backend("auto")
    grounding_head.set_ground_auto(**saved[0])
    loss._FUSED_OG3D = saved[1]


def save_defaults():
    from sceneverse_amd.modules.heads import grounding_head
    from sceneverse_amd.optim.loss import loss
    return grounding_head.set_ground_auto(), loss._FUSED_OG3D


def _summary(ts):
    return {"ms_per_round": [round(t, 4) for t in ts], "ms_median": round(statistics.median(ts), 4),
            "ms_spread": round(max(ts) - min(ts), 4)}


def bench_step(args, dev):
    from bench import _lang_dir, gps_pretrain_cfg
    from sceneverse_amd.data.synthetic import synth_batch
    from sceneverse_amd.engine import GPSTrainStep
    batch = synth_batch(args.batch, n_obj=args.objects, n_pts=args.points, txt_len=args.tokens, seed=42, device=dev)
    batch.pop("scene_txt_ids", None), batch.pop("scene_txt_masks", None)
    saved = save_defaults()
    engines, first_loss = {}, {}
    for name in VARIANTS:
        set_variant(name)
        st = GPSTrainStep(gps_pretrain_cfg(_lang_dir(), workload="finetune"), device=dev, ddp=False, graph=True,
                          graph_warmup=2, seed=7)
        for _ in range(2 + 1 + args.warmup):            # eager warm-up, capture, replays
            total, _ = st.step(dict(batch))
        torch.cuda.synchronize()
        assert st._graph is not None
        engines[name], first_loss[name] = st, total.item()
    restore_defaults(saved)
    times = {name: [] for name in VARIANTS}
    for _ in range(args.rounds):
        for name in VARIANTS:
            st = engines[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                total, _ = st.step(dict(batch))
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {name: dict(_summary(ts), loss_after_warmup=first_loss[name]) for name, ts in times.items()}
    spread = max(v["ms_spread"] for v in out.values())
    out["window_spread_ms"] = spread                     # the largest max - min between repeated windows of one engine

    def gain(a, b):                                      # median of a minus median of b; a piece wins when this exceeds the spread
        d = round(out[a]["ms_median"] - out[b]["ms_median"], 4)
        return {"saves_ms": d, "beyond_spread": bool(d > spread)}

    out["pieces"] = {"og3d_head": gain("torch", "og3d_head"),
                     "class_heads": gain("og3d_head", "og3d_head+class_heads"),
                     "og3d_loss": gain("og3d_head", "og3d_head+loss")}
    out["native_minus_torch_ms"] = round(out["native"]["ms_median"] - out["torch"]["ms_median"], 4)
    out["native_over_torch"] = round(out["native"]["ms_median"] / out["torch"]["ms_median"], 4)
    return out


def _time_pair(fns, iters, warmup):
    """fns: {name: callable}; alternating single calls bracketed by device events -> {name: median / min / spread us}."""
    for f in fns.values():
        for _ in range(warmup):
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(iters):
        for k, f in fns.items():
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(1e3 * e0.elapsed_time(e1))
    q = lambda v, f: sorted(v)[int(f * (len(v) - 1))]  # noqa: E731
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2),
                "iqr_us": round(q(v, 0.75) - q(v, 0.25), 2)} for k, v in ts.items()}


def bench_ops(args, dev):
    from sceneverse_amd.modules.heads.grounding_head import GroundHeadV1, _cls_logits, _og3d_logits
    from sceneverse_amd.optim.loss import loss as L
    saved = save_defaults()
    g = torch.Generator().manual_seed(0)
    B, O = args.batch, args.objects
    head = GroundHeadV1(None, input_size=768, hidden_size=384, sem_cls_size=607, dropout=0.3,
                        detach_all_aux_loss=True).to(dev).train()
    obj = torch.randn(B, O, 768, generator=g).to(dev).requires_grad_(True)               # fp32 encoder output
    masks = (torch.rand(B, O, generator=g) > 0.3).to(dev)
    masks[:, 0] = True
    dl = torch.randn(B, O, generator=g).to(dev)
    tgt = torch.zeros(B, 1, dtype=torch.long, device=dev)

    def run(native, fn):
        def call():
            set_mode(native)
            with torch.autocast("cuda", dtype=torch.bfloat16):
                fn()
        return call

    def og3d_head():
        y = _og3d_logits(head.og3d_head, obj, masks, True)
        y.backward(dl.to(y.dtype))

    def cls_head():
        with torch.no_grad():
            _cls_logits(head.obj3d_clf_head, obj, True)

    logits32 = torch.randn(B, O, generator=g).to(dev).masked_fill(masks.logical_not(), -float("inf")).requires_grad_(True)
    logits16 = logits32.detach().to(torch.bfloat16).requires_grad_(True)      # what the torch head hands the loss under autocast

    def loss_native():
        L.og3d_loss({"og3d_logits": logits32, "tgt_object_id": tgt}).backward()

    def loss_torch():
        L.og3d_loss({"og3d_logits": logits16, "tgt_object_id": tgt}).backward()

    out = {"og3d_head_fwd_bwd": dict(_time_pair({"torch": run(False, og3d_head), "native": run(True, og3d_head)},
                                                args.op_iters, 5), shape=[B, O, 768, 384]),
           "class_head_fwd": dict(_time_pair({"torch": run(False, cls_head), "native": run(True, cls_head)},
                                             args.op_iters, 5), shape=[B, O, 768, 384, 607]),
           "og3d_loss_fwd_bwd": dict(_time_pair({"torch": run(False, loss_torch), "native": run(True, loss_native)},
                                                args.op_iters, 5), shape=[B, O])}
    restore_defaults(saved)
    for v in out.values():
        v["native_over_torch"] = round(v["native"]["median_us"] / v["torch"]["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--objects", type=int, default=80)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=50)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ground_bench: no GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    res = {"config": vars(args), "device": torch.cuda.get_device_name(0), "ops": bench_ops(args, dev)}
    if not args.skip_step:
        res["step"] = bench_step(args, dev)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
