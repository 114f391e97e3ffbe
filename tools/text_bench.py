"""Timing of the resident text path (csrc/gps_text.hip, sceneverse_amd/data/gpu_text.py) against the host loop it replaces.

    python tools/text_bench.py [--samples 50] [--out profiles/text/text_bench.txt]

Shapes: the pre-train batch (B = 64, L = 50, Ls = 300, O = 80, captions and masking) and the fine-tune batch (B = 256,
L = 50, no captions, gather only).  Per shape, medians of `--samples` device-event windows after warm-up:
  * the launch alone: 20 launches captured into one graph and replayed, divided by 20 (GPU time, no host launch path);
  * the wrapper call as a loader makes it: `text_batch(out=static buffers)` eager, index tensors already on the device.
Host comparison, on this machine's CPU in one process: the per-sample loop the launch replaces -- this tool's own
restatement of the reference's masking (a Python loop over the tokens with an `.item()` per token and the vocabulary
list rebuilt for every random replacement, a Python loop over the object slots), on the same batch; the two tokenizer
calls per sample are NOT in it (a corpus can be tokenised once on either path).  Host clock, median of 5 batches."""
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

from sceneverse_amd.data import gpu_text as T  # noqa: E402
from sceneverse_amd.data.synthetic import synth_packed_texts  # noqa: E402

GRAPH_ITERS = 20


def event_samples(fn, n):
    """n device-event timings of fn() in us, after 10 warm-up calls."""
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
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


def host_masking(txt_ids, txt_masks, obj_masks, vocab, txt_ratio, pc_ratio, mask_id=103):
    """One batch through the per-sample loops: per token a draw (and `.item()`), 80 / 10 / 10; per object slot a draw."""
    ids_out, labels_out, sem_out = [], [], []
    for b in range(txt_ids.shape[0]):
        tokens, tokens_mask = txt_ids[b], txt_masks[b]
        out_tokens, labels = tokens.clone(), []
        for i, token in enumerate(tokens):
            if tokens_mask[i] == 0:
                labels.append(-1)
                continue
            p = random.random()
            if p < txt_ratio:
                p /= txt_ratio
                if p < 0.8:
                    out_tokens[i] = mask_id
                elif p < 0.9:
                    out_tokens[i] = random.choice(list(vocab.items()))[1]
                labels.append(token.item())
            else:
                labels.append(-1)
        ids_out.append(out_tokens)
        labels_out.append(torch.Tensor(labels).long())
    for b in range(obj_masks.shape[0]):
        sem = []
        for o in range(obj_masks.shape[1]):
            sem.append(0 if obj_masks[b][o] == 0 or random.random() < pc_ratio else 1)
        sem_out.append(torch.tensor(sem, dtype=torch.bool))
    return torch.stack(ids_out), torch.stack(labels_out), torch.stack(sem_out)


def line(name, t):
    return f"{name}: {statistics.median(t):.2f} us [{min(t):.2f} .. {max(t):.2f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "text_bench.py measures on a GPU"
    dev = torch.device("cuda", 0)
    lines = [f"device: {torch.cuda.get_device_name(dev)}; {args.samples} device-event samples after warm-up; "
             f"median [min .. max]; host CPUs visible: {os.cpu_count()}, host loop in one process"]
    texts = synth_packed_texts(4096, 512, seed=0, device=dev)
    rng = np.random.default_rng(1)
    vocab = {str(i): i for i in range(T.BERT_VOCAB)}

    for name, B, with_caps, mask in (("pre-train B=64 L=50 Ls=300 O=80, captions, masking", 64, True, True),
                                     ("fine-tune B=256 L=50, no captions, gather only", 256, False, False)):
        L, Ls, O = 50, 300, 80
        sent = torch.from_numpy(rng.integers(0, 4096, size=B).astype(np.int32)).to(dev)
        cap = torch.from_numpy((4096 + rng.integers(0, 512, size=B)).astype(np.int32)).to(dev) if with_caps else None
        obj_masks = torch.from_numpy(np.arange(O)[None, :] < rng.integers(20, O, size=B)[:, None]).to(dev)
        seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
        kw = dict(max_seq_len=L, max_scene_cap_len=Ls, mask=mask, obj_masks=obj_masks, seed=7, seed_dev=seed_dev)
        out = T.text_batch(texts, sent, cap, **kw)

        def call():
            T.text_batch(texts, sent, cap, out=out, **kw)
        n_bytes = sum(t.numel() * t.element_size() for t in out.values())
        t_launch = [t / GRAPH_ITERS for t in event_samples(captured(call, GRAPH_ITERS), args.samples)]
        t_call = event_samples(call, args.samples)
        lines.append(f"[{name}] {n_bytes / 1e3:.0f} kB of outputs per batch")
        lines.append(line("  gps_text_batch, the launch alone (graph of 20, per launch)", t_launch))
        lines.append(line("  text_batch(out=) eager, events around the call", t_call))
        if mask:
            gathered = T.text_batch(texts, sent, None, max_seq_len=L, mask=False)
            ids, masks, om = gathered["txt_ids"].cpu(), gathered["txt_masks"].cpu(), obj_masks.cpu()
            t_host = []
            for _ in range(5):
                t0 = time.perf_counter()
                host_masking(ids, masks, om, vocab, 0.15, 0.1)
                t_host.append((time.perf_counter() - t0) * 1e6)
            lines.append(line("  host masking loop, same batch, this machine's CPU (host clock, 5 batches)", t_host))
            lines.append(f"  host loop / eager call = {statistics.median(t_host) / statistics.median(t_call):.0f}x")
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
