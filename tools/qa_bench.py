"""Time the ScanQA fine-tune step and its three native ops against the torch compositions they replace.

    python tools/qa_bench.py --out profiles/qa/qa_bench.json

Step: finetune/scanqa_finetune.yaml's model (QAHeadV1 with 8864 answers, answer_loss + BCE TextObjWithinBatch) at
B = 64, 80 objects x 1024 points, 50 tokens, bf16 autocast, HIP-graph replay.  Two engines live in one process: "torch" =
set_qa_backend("torch") and the fused loss branches off (the behaviour before the native QA path), "native" = the
defaults.  Each is captured under its own setting (a replay no longer consults the switches), then timed windows of
`--steps` replays alternate between the two, `--rounds` times; the host clock brackets a window that ends in a device
synchronise.  Ops: forward + backward of each native op and of its torch composition on the step's shapes, device
events, alternating.  No GPU: the script fails, it does not fall back."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def set_mode(native: bool) -> None:
    from sceneverse_amd.modules.heads import qa_head
    from sceneverse_amd.optim.loss import contra_loss, loss
    qa_head.set_qa_backend("auto" if native else "torch")
    contra_loss._FUSED = bool(native)
    loss._FUSED_BCE = bool(native)


def qa_cfg(answers: int):
    from bench import _lang_dir, gps_pretrain_cfg
    cfg = gps_pretrain_cfg(_lang_dir())
    cfg["task"] = "ScanQA"
    cfg["data"] = {"args": {"use_scene_cap": False}}
    cfg.model["heads"] = {"head_list": ["qa_head"],
                          "qa_head": {"name": "QAHeadV1", "args": {"hidden_size": 768, "mlp_size": 256, "glimpse": 1,
                                                                   "flat_out_size": 512, "num_answers": answers}}}
    cfg.model["loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    cfg.model["vis_loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    return cfg


def bench_step(args, dev):
    from sceneverse_amd.data.synthetic import synth_qa_batch
    from sceneverse_amd.engine import GPSTrainStep
    batch = synth_qa_batch(args.batch, n_obj=args.objects, n_pts=args.points, txt_len=args.tokens, n_answers=args.answers,
                           seed=42, device=dev)
    engines, first_loss = {}, {}
    for name in ("torch", "native"):
        set_mode(name == "native")
        st = GPSTrainStep(qa_cfg(args.answers), device=dev, ddp=False, graph=True, graph_warmup=2, seed=7)
        for _ in range(2 + 1 + args.warmup):            # eager warm-up, capture, replays
            total, _ = st.step(dict(batch))
        torch.cuda.synchronize()
        assert st._graph is not None
        engines[name], first_loss[name] = st, total.item()
    set_mode(True)
    times = {"torch": [], "native": []}
    for _ in range(args.rounds):
        for name in ("torch", "native"):
            st = engines[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                total, _ = st.step(dict(batch))
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / args.steps)
    out = {name: {"step_ms_per_round": [round(t, 4) for t in ts], "step_ms_median": round(statistics.median(ts), 4),
                  "loss_after_warmup": first_loss[name]} for name, ts in times.items()}
    out["native_over_torch"] = round(out["native"]["step_ms_median"] / out["torch"]["step_ms_median"], 4)
    return out


def _time_pair(fns, iters, warmup):
    """fns: {name: callable}; alternating single calls bracketed by device events -> {name: median us}."""
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
    return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2)} for k, v in ts.items()}


def bench_ops(args, dev):
    from sceneverse_amd.modules.heads.fused_attflat import attflat_pool
    from sceneverse_amd.optim.loss.fused_bce import bce_logits_sum, text_obj_bce
    g = torch.Generator().manual_seed(0)
    B, D, M, A = args.batch, 768, 256, args.answers
    out = {}
    for tag, T in (("attflat_objects", args.objects), ("attflat_text", args.tokens)):
        x = torch.randn(B, T, D, generator=g).to(dev).requires_grad_(True)               # fp32 encoder output
        h = torch.randn(B, T, M, generator=g).to(dev, torch.bfloat16).requires_grad_(True)   # bf16 GEMM output
        w2 = (torch.randn(1, M, generator=g) / 16).to(dev).requires_grad_(True)
        b2 = torch.zeros(1, device=dev, requires_grad=True)
        keep = (torch.rand(B, T, generator=g) > 0.3).to(dev)
        keep[:, 0] = True
        dp = torch.randn(B, D, generator=g).to(dev)

        def native():
            attflat_pool(x, h, w2, b2, keep).backward(dp)

        def composed():
            with torch.autocast("cuda", dtype=torch.bfloat16):
                att = F.linear(h, w2, b2).masked_fill(keep.logical_not().unsqueeze(2), -1e9)
                att = F.softmax(att, dim=1)
                pooled = torch.einsum('btg,btd->bgd', att, x).flatten(1)
            pooled.backward(dp.to(pooled.dtype))

        out[tag] = dict(_time_pair({"torch": composed, "native": native}, args.op_iters, 5), shape=[B, T, D, M, 1])
    x = torch.randn(B, A, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    y = (torch.rand(B, A, generator=g) < 2e-4).long().to(dev)
    out["answer_loss"] = dict(_time_pair({
        "torch": lambda: (F.binary_cross_entropy_with_logits(x, y.float(), reduction='sum') / B).backward(),
        "native": lambda: bce_logits_sum(x, y, None, 1.0 / B).backward()}, args.op_iters, 5), shape=[B, A])
    O = args.objects
    obj = torch.randn(B, O, D, generator=g).to(dev).requires_grad_(True)
    txt = torch.randn(B, D, generator=g).to(dev).requires_grad_(True)
    masks = (torch.rand(B, O, generator=g) > 0.3).to(dev)
    labels = ((torch.rand(B, O, generator=g) < 0.05).to(dev) & masks).long()

    def composed_tob():
        from sceneverse_amd.modules.layers.fused_norm import l2_normalize
        logits = torch.einsum('bod,bd->bo', l2_normalize(obj), l2_normalize(txt))
        (F.binary_cross_entropy_with_logits(logits, labels.float(), reduction="sum", weight=masks) / float(B)).backward()

    out["text_obj_bce"] = dict(_time_pair({"torch": composed_tob,
                                           "native": lambda: text_obj_bce(obj, txt, labels, masks).backward()},
                                          args.op_iters, 5), shape=[B, O, D])
    for v in out.values():
        v["native_over_torch"] = round(v["native"]["median_us"] / v["torch"]["median_us"], 4)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--objects", type=int, default=80)
    ap.add_argument("--points", type=int, default=1024)
    ap.add_argument("--tokens", type=int, default=50)
    ap.add_argument("--answers", type=int, default=8864)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--op-iters", type=int, default=50)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("qa_bench: no GPU; nothing is measured without one")
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
