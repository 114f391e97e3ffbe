"""Generate tests/golden/ground_reference_cpu.pt: outputs of the REFERENCE's own grounding classes -- GroundHeadV1 /
GroundHead (modules/heads/grounding_head.py) and og3d_loss (optim/loss/loss.py:8-9) -- run unmodified on CPU from the
reference checkout with the recipe of make_golden.py, in eval mode (no dropout), forward + backward on the seeded inputs
of tests/ground_cases.py.  Weights are not stored: oracle/param_fill.fill_params derives them from parameter names.

    python tests/golden/make_golden_ground.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  (sets up sys.path, stubs, the .cuda() patch)

import torch  # noqa: E402

from oracle.param_fill import fill_params  # noqa: E402
from tests.ground_cases import GRAD_NAMES, HEAD_CONFIGS, SEED, forward_backward, head_inputs, summary  # noqa: E402


def main():
    MG.import_reference()
    from modules.heads import grounding_head as ref_heads
    from optim.loss.loss import og3d_loss

    fx = {"seed": SEED}
    for name, (kind, kw) in HEAD_CONFIGS.items():
        head = getattr(ref_heads, kind)(None, **kw).eval()
        fill_params(head, SEED)
        x = head_inputs()
        obj, obj_pre, txt = (x[k].clone().requires_grad_(True) for k in ("obj", "obj_pre", "txt"))
        logits, loss, total = forward_backward(head, kind, og3d_loss, x, obj, obj_pre, txt)
        rec = {k: (v.detach().clone() if k == "og3d_logits" else summary(v)) for k, v in logits.items()}
        rec.update({"og3d_loss": loss.item(), "total": total.item(),
                    "d_obj": summary(obj.grad), "d_obj_pre": summary(obj_pre.grad), "d_txt": summary(txt.grad),
                    "grads": MG.grad_summary(head, GRAD_NAMES[kind]),
                    "state_dict_keys": sorted(head.state_dict().keys())})
        fx["head_" + name] = rec

    dst = os.path.join(HERE, "ground_reference_cpu.pt")
    torch.save(fx, dst)
    print("wrote", dst, os.path.getsize(dst) // 1024, "KiB")
    print({k: (fx["head_" + k]["og3d_loss"], fx["head_" + k]["total"]) for k in HEAD_CONFIGS})


if __name__ == "__main__":
    main()
