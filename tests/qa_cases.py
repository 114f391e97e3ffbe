"""Seeded inputs of the question-answering checks, shared by tests/golden/make_golden_qa.py (which runs the reference
on them) and the tests (which regenerate them: they are not stored twice)."""
import os

import torch

from oracle.param_fill import fill_params
from sceneverse_amd.data.synthetic import synth_qa_batch
from tests.util import gps_cfg, lang_dir

SEED = 11
N_ANSWERS = 8864
HEAD_CONFIGS = {
    "sqa3d": dict(hidden_size=768, mlp_size=256, glimpse=1, flat_out_size=512, num_answers=706),
    "glimpse2": dict(hidden_size=768, mlp_size=256, glimpse=2, flat_out_size=512, num_answers=64),
}


def load_gold():
    return torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qa_reference_cpu.pt"),
                      weights_only=False)


def head_inputs(num_answers):
    """Seeded inputs shared with the tests (regenerated there, not stored twice): 3 scenes x 7 objects x 12 tokens; scene
    0 all objects valid + a full-length text, scene 1 ONE valid object + a short text, scene 2 NO valid object (the
    -1e9 fill: uniform 1 / 7 weights)."""
    g = torch.Generator().manual_seed(211)
    obj = torch.randn(3, 7, 768, generator=g)
    txt = torch.randn(3, 12, 768, generator=g)
    obj_masks = torch.zeros(3, 7, dtype=torch.bool)
    obj_masks[0] = True
    obj_masks[1, 2] = True
    txt_masks = (torch.arange(12)[None, :] < torch.tensor([12, 5, 8])[:, None]).long()
    label = torch.zeros(3, num_answers, dtype=torch.long)
    label[0, torch.randint(0, num_answers, (3,), generator=g)] = 1
    label[1, torch.randint(0, num_answers, (1,), generator=g)] = 1      # row 2: unanswerable, all zero
    return {"obj": obj, "txt": txt, "obj_masks": obj_masks, "txt_masks": txt_masks, "answer_label": label}


def model_batch():
    """OpenVocab input: 2 scenes x 6 objects x 1024 points, 12 tokens, multi-hot answers and target objects."""
    return synth_qa_batch(2, n_obj=6, n_pts=1024, txt_len=12, n_answers=N_ANSWERS, seed=SEED, min_real=3)


def metric_inputs():
    """16 questions x 64 answers, continuous scores (no ties); the labels hit the best answer, one of ranks 2 - 10, a
    rank past 10 or nothing; question type 4 does not occur (the 1e-10 count floor)."""
    g = torch.Generator().manual_seed(307)
    scores = torch.randn(16, 64, generator=g)
    order = scores.argsort(dim=1, descending=True)
    label = torch.zeros(16, 64, dtype=torch.long)
    for i in range(16):
        kind = i % 4
        if kind == 0:
            label[i, order[i, 0]] = 1
        elif kind == 1:
            label[i, order[i, 1 + (i % 9)]] = 1
            label[i, order[i, 40]] = 1
        elif kind == 2:
            label[i, order[i, 10 + (i % 20)]] = 1
    types = torch.tensor([0, 1, 2, 3, 5, 0, 1, 2, 3, 5, 0, 0, 1, 5, 5, 2])
    obj_logits = torch.randn(16, 5, 9, generator=g)
    obj_labels = torch.randint(0, 9, (16, 5), generator=g)
    obj_masks = torch.rand(16, 5, generator=g) > 0.3
    obj_masks[:, 0] = True
    return {"answer_scores": scores, "answer_label": label, "sqa_type": types, "obj_cls_raw_logits": obj_logits,
            "obj_labels": obj_labels, "obj_masks": obj_masks}


def as_qa_cfg(cfg, num_answers=N_ANSWERS):
    """Edit a GPS config in place into finetune/scanqa_finetune.yaml's head and loss section: QAHeadV1
    (768 / 256 / glimpse 1 / 512), task 'ScanQA', answer_loss + TextObjWithinBatch (its BCE branch)."""
    cfg["task"] = "ScanQA"
    cfg["data"] = {"args": {"use_scene_cap": False}}
    cfg.model["heads"] = {"head_list": ["qa_head"],
                          "qa_head": {"name": "QAHeadV1",
                                      "args": {"hidden_size": 768, "mlp_size": 256, "glimpse": 1, "flat_out_size": 512,
                                               "num_answers": num_answers}}}
    cfg.model["loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    cfg.model["vis_loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    return cfg


def close(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.float().cpu()
    err, scale = (a - b).abs().max().item(), b.abs().max().item()
    assert err <= tol * max(1.0, scale), f"{what}: {err:.3e} vs scale {scale:.3e}"


def close_l2(a, b, tol, what):
    a, b = a.detach().float().cpu(), b.float().cpu()
    err, scale = (a - b).norm().item(), b.norm().item()
    assert err <= tol * scale, f"{what}: relative L2 {err / max(scale, 1e-30):.3e}"


# gradient bounds: (norm, first 256 entries relative L2, floor of that L2's denominator as a share of the norm)
FP32_CPU_GRADS = (2e-4, 2e-4, 1e-3)
FP32_MODEL_CPU_GRADS = (2e-3, 2e-3, 1e-3)
FP32_GPU_GRADS = (2e-2, 2e-2, 1e-3)                     # tests/test_a16_vs_golden.py, the device fp32 run
BF16_STEP_GRADS = (5e-2, 1e-1, 1e-2)                    # tests/test_gpu_model.py, the bf16 whole-step bounds


def check_grads(named_params, ref_grads, bounds, what):
    ntol, htol, floor = bounds
    params = dict(named_params)
    for name, ref in ref_grads.items():
        gr = params[name].grad.float().cpu()
        assert abs(gr.norm().item() - ref["norm"]) <= ntol * ref["norm"], (what, name, gr.norm().item(), ref["norm"])
        err = (gr.flatten()[:256] - ref["head"]).norm().item()
        assert err <= htol * max(ref["head"].norm().item(), floor * ref["norm"]), (what, name, err)


def run_head(dev, gold, name, tol, bounds, autocast=False, ltol=None):
    """Forward + answer_loss + backward of the product's QAHeadV1 against the reference's.  tol: outputs, relative to
    max(1, output scale); ltol: the loss, relative (default 5 tol); bounds: the parameter gradients (see above); the
    input gradients are held to tol (fp32) or, under autocast, to the relative L2 of `bounds`."""
    from sceneverse_amd.modules.heads.qa_head import QAHeadV1
    from sceneverse_amd.optim.loss.loss import answer_loss
    kw, g = HEAD_CONFIGS[name], gold["head_" + name]
    head = QAHeadV1(None, **kw).eval()
    fill_params(head, SEED)
    head.to(dev)
    x = {k: v.to(dev) for k, v in head_inputs(kw["num_answers"]).items()}
    obj, txt = x["obj"].clone().requires_grad_(True), x["txt"].clone().requires_grad_(True)
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if autocast else torch.autocast("cpu", enabled=False)
    with ctx:
        scores = head(obj, x["obj_masks"], txt, x["txt_masks"])
        loss = answer_loss({"answer_scores": scores, "answer_label": x["answer_label"]})
    loss.backward()
    assert torch.isfinite(scores).all()
    close(scores, g["answer_scores"], tol, name + " answer_scores")
    ltol = 5 * tol if ltol is None else ltol
    assert abs(loss.item() - g["answer_loss"]) <= ltol * abs(g["answer_loss"]), (loss.item(), g["answer_loss"])
    if autocast:
        close_l2(obj.grad, g["d_obj"], bounds[1], name + " d_obj")
        close_l2(txt.grad, g["d_txt"], bounds[1], name + " d_txt")
    else:
        close(obj.grad, g["d_obj"], bounds[0], name + " d_obj")
        close(txt.grad, g["d_txt"], bounds[0], name + " d_txt")
    check_grads(head.named_parameters(), g["grads"], bounds, name)


def run_model(dev, gold, tol, bounds, autocast=False, ltol=None):
    from sceneverse_amd.model.build import build_model
    from sceneverse_amd.optim.loss import Loss
    cfg = as_qa_cfg(gps_cfg(lang_dir(SEED), heads="pretrain", use_scene_cap=False))
    model = build_model(cfg).eval()
    loss_mod = Loss(cfg)
    fill_params(model, SEED)
    model.to(dev)
    loss_mod.to(dev)
    data = {k: v.to(dev) for k, v in model_batch().items()}
    ctx = torch.autocast("cuda", dtype=torch.bfloat16) if autocast else torch.autocast("cpu", enabled=False)
    with ctx:
        out = model(data)
        total, losses = loss_mod(out)
    total.backward()
    g = gold["model"]
    close(out["answer_scores"], g["answer_scores"], tol, "model answer_scores")
    close(out["intra_text_embed"], g["intra_text_embed"], tol, "intra_text_embed")
    ltol = 5 * tol if ltol is None else ltol
    for k, v in g["losses"].items():
        assert abs(losses[k].item() - v) <= ltol * max(1.0, abs(v)), (k, losses[k].item(), v)
    check_grads(model.named_parameters(), g["grads"], bounds, "model")
