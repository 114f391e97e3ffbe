"""Generate tests/golden/qa_reference_cpu.pt: outputs of the REFERENCE's own question-answering classes -- QAHeadV1
(modules/heads/qa_head.py), answer_loss (optim/loss/loss.py:50-53), the BCE branch of TextObjWithinBatch
(optim/loss/contra_loss.py:29-35), OpenVocab with `head_list: [qa_head]` and `task: 'ScanQA'`
(configs/final/finetune/scanqa_finetune.yaml) and the metrics of ScanQAEval / SQA3DEval -- run unmodified on CPU from
/root/reference with the recipe of make_golden.py (stubs, oracle point ops, offline BERT).  Weights are not stored:
oracle/param_fill.fill_params derives them from parameter names.

    python tests/golden/make_golden_qa.py
"""
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets up sys.path, stubs, the .cuda() patch)

import torch  # noqa: E402

from oracle.param_fill import fill_params  # noqa: E402
from tests.qa_cases import HEAD_CONFIGS, N_ANSWERS, SEED, head_inputs, metric_inputs, model_batch  # noqa: E402

HEAD_GRAD_NAMES = ["attflat_visual.mlp.linear.weight", "attflat_lang.mlp.fc.linear.weight",
                   "attflat_lang.linear_merge.weight", "answer_cls.3.bias"]
MODEL_GRAD_NAMES = ["qa_head.attflat_visual.mlp.fc.linear.weight", "unified_encoder.unified_encoder.1.linear2.weight",
                    "lang_encoder.model.encoder.layer.0.attention.self.query.weight"]


def qa_cfg(lang_path):
    cfg = MG.gps_cfg(lang_path, heads="pretrain", use_scene_cap=False)
    cfg["task"] = "ScanQA"
    cfg.model["heads"] = {"head_list": ["qa_head"],
                          "qa_head": {"name": "QAHeadV1",
                                      "args": {"hidden_size": 768, "mlp_size": 256, "glimpse": 1, "flat_out_size": 512,
                                               "num_answers": N_ANSWERS}}}
    cfg.model["loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    cfg.model["vis_loss_list"] = ["answer_loss", "TextObjWithinBatch"]
    return cfg


def main():
    MG.import_reference()
    from model.build import build_model
    from modules.heads.qa_head import QAHeadV1
    from optim.loss.loss import Loss, answer_loss

    fx = {"seed": SEED}
    # ---- 1. the head alone, eval mode, forward + answer_loss + backward ---------------------------------------------
    for name, kw in HEAD_CONFIGS.items():
        head = QAHeadV1(None, **kw).eval()
        fill_params(head, SEED)
        x = head_inputs(kw["num_answers"])
        obj, txt = x["obj"].clone().requires_grad_(True), x["txt"].clone().requires_grad_(True)
        scores = head(obj, x["obj_masks"], txt, x["txt_masks"])
        loss = answer_loss({"answer_scores": scores, "answer_label": x["answer_label"]})
        loss.backward()
        fx["head_" + name] = {"answer_scores": scores.detach(), "answer_loss": float(loss), "d_obj": obj.grad.clone(),
                              "d_txt": txt.grad.clone(), "grads": MG.grad_summary(head, HEAD_GRAD_NAMES),
                              "state_dict_keys": sorted(head.state_dict().keys())}

    # ---- 2. OpenVocab with the QA head, task ScanQA: answer_loss + BCE TextObjWithinBatch ----------------------------
    tmp = tempfile.mkdtemp()
    torch.save(MG.text_features(SEED), os.path.join(tmp, "scannet_607_bert-base-uncased_id.pth"))
    cfg = qa_cfg(tmp)
    model = build_model(cfg).eval()
    loss_mod = Loss(cfg)
    fill_params(model, SEED)
    out = model({k: v.clone() for k, v in model_batch().items()})
    total, losses = loss_mod(out)
    total.backward()
    fx["model"] = {"answer_scores": out["answer_scores"].detach(),
                   "intra_text_embed": out["intra_text_embed"].detach(),
                   "intra_obj_embeds": out["intra_obj_embeds"].detach(),
                   "losses": {k: float(v) for k, v in losses.items()},
                   "grads": MG.grad_summary(model, MODEL_GRAD_NAMES)}

    # ---- 3. metrics: the evaluators' batch_metrics, called unbound on a bare object (their constructors read files) ---
    from evaluator.scanqa_eval import ScanQAEval
    from evaluator.sqa3d_eval import SQA3DEval

    class Bare:
        save = False

    m = metric_inputs()
    fx["metrics_scanqa"] = {k: float(v) for k, v in ScanQAEval.batch_metrics(
        Bare(), {k: m[k] for k in ("answer_scores", "answer_label")}).items()}
    fx["metrics_sqa3d"] = {k: float(v) for k, v in SQA3DEval.batch_metrics(Bare(), dict(m)).items()}

    dst = os.path.join(HERE, "qa_reference_cpu.pt")
    torch.save(fx, dst)
    print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
    print("head losses", {k: fx["head_" + k]["answer_loss"] for k in HEAD_CONFIGS}, "model losses", fx["model"]["losses"])
    print("scanqa", fx["metrics_scanqa"])
    print("sqa3d", fx["metrics_sqa3d"])


if __name__ == "__main__":
    main()
