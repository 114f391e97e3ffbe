"""Grounding heads (reference modules/heads/grounding_head.py:7-55): small MLPs over the fused
object / text tokens.

On GPU tensors the heads run on libgps_hip.so (`fused_mlp_head`, csrc/gps_ground.hip): `og3d_head` = the first Linear
(the in-tree GEMM with its bias + ReLU epilogue under bf16 execution, torch's Linear for fp32 tensors) and ONE launch for
ReLU, LayerNorm, dropout, the 1-output Linear, the squeeze and the -inf fill of the padded objects; the three class heads
run their hidden part the same way under bf16 execution and keep torch's last Linear (607 classes are not a multiple of
8).  CPU tensors keep the reference's formulation.  Parameter names and state-dict keys are the reference's.

Under autocast the native `og3d_logits` are fp32 (the dot product of the unrounded hidden row); the torch composition
rounds them to bf16 and `og3d_loss` casts them up again.  Shape, -inf positions and the dict keys are the same.

Backends (see `set_ground_backend`): "auto" = native where the library serves the call, "hip" = native or an error for
`og3d_head` (CPU tensors included; the class heads behave as under "auto", like the Linears around the QA head's pooling
core), "torch" = the composition on any tensor."""
import torch.nn as nn

from ..build import HEADS_REGISTRY
from ..utils import get_mlp_head

_BACKEND = "auto"  # "auto" | "hip" | "torch"
# the pieces "auto" runs natively on GPU tensors: those that measured faster than their torch composition inside the
# captured fine-tune step (tools/ground_bench.py); "hip" runs every piece natively
_AUTO_NATIVE = {"og3d_head": True, "class_heads": True}


def set_ground_backend(name: str) -> None:
    global _BACKEND
    if name not in ("auto", "hip", "torch"):
        raise ValueError(name)
    _BACKEND = name


def get_ground_backend() -> str:
    return _BACKEND


def set_ground_auto(og3d_head=None, class_heads=None) -> dict:
    """Choose the pieces backend "auto" runs natively (None = leave as it is); -> the selection."""
    if og3d_head is not None:
        _AUTO_NATIVE["og3d_head"] = bool(og3d_head)
    if class_heads is not None:
        _AUTO_NATIVE["class_heads"] = bool(class_heads)
    return dict(_AUTO_NATIVE)


def _native(piece: str, x) -> bool:
    return _BACKEND == "hip" or (_BACKEND == "auto" and x.is_cuda and _AUTO_NATIVE[piece])


def _refuse(x, seq, what):
    raise RuntimeError(f"grounding backend 'hip' requested for an unsupported call ({what}: x {tuple(x.shape)} "
                       f"{x.dtype} on {x.device.type}, stack {[type(m).__name__ for m in seq]}, hidden "
                       f"{getattr(seq[0], 'out_features', None)})")


def _og3d_logits(seq, obj_embeds, obj_masks, training):
    """`seq(obj_embeds).squeeze(2)` with -inf at the padded objects."""
    if _native("og3d_head", obj_embeds):
        from . import fused_mlp_head
        ok = (fused_mlp_head.mlp_head_usable(obj_embeds, seq) and seq[4].out_features == 1 and obj_embeds.dim() == 3
              and (obj_masks is None or (obj_masks.is_cuda and obj_masks.shape == obj_embeds.shape[:2])))
        if ok:
            return fused_mlp_head.mlp_head_logit(obj_embeds, seq, obj_masks, training)
        if _BACKEND == "hip":
            _refuse(obj_embeds, seq, "og3d_head")
    og3d_logits = seq(obj_embeds).squeeze(2)
    if obj_masks is not None:
        og3d_logits = og3d_logits.masked_fill_(obj_masks.logical_not(), -float('inf'))
    return og3d_logits


def _cls_logits(seq, x, training):
    """A class head: the hidden part natively under bf16 execution, torch's last Linear."""
    if x.is_cuda and _native("class_heads", x):
        from . import fused_mlp_head
        if fused_mlp_head.mlp_head_hidden_usable(x, seq):
            return seq[4](fused_mlp_head.mlp_head_hidden(x, seq, training))
    return seq(x)


@HEADS_REGISTRY.register()
class GroundHeadV1(nn.Module):
    def __init__(self, cfg, input_size=768, hidden_size=768, sem_cls_size=607, dropout=0.3,
                 detach_all_aux_loss=False):
        super().__init__()
        self.og3d_head = get_mlp_head(input_size, hidden_size, 1, dropout=dropout)
        self.txt_clf_head = get_mlp_head(input_size, hidden_size, sem_cls_size, dropout=dropout)
        self.obj3d_clf_head = get_mlp_head(input_size, hidden_size, sem_cls_size, dropout=dropout)
        self.obj3d_clf_pre_head = get_mlp_head(input_size, hidden_size, sem_cls_size, dropout=dropout)
        self.detach_all_aux_loss = detach_all_aux_loss

    def forward(self, txt_embeds, obj_embeds, obj_pre_embeds, obj_masks, **kwargs):
        og3d_logits = _og3d_logits(self.og3d_head, obj_embeds, obj_masks, self.training)
        if self.detach_all_aux_loss:
            txt_embeds, obj_embeds, obj_pre_embeds = (txt_embeds.detach(), obj_embeds.detach(),
                                                      obj_pre_embeds.detach())
        return (_cls_logits(self.txt_clf_head, txt_embeds[:, 0], self.training),
                _cls_logits(self.obj3d_clf_head, obj_embeds, self.training),
                _cls_logits(self.obj3d_clf_pre_head, obj_pre_embeds, self.training), og3d_logits)


@HEADS_REGISTRY.register()
class GroundHead(nn.Module):
    def __init__(self, cfg, input_size=768, hidden_size=768, dropout=0.3):
        super().__init__()
        self.og3d_head = get_mlp_head(input_size, hidden_size, 1, dropout=dropout)

    def forward(self, obj_embeds, obj_masks=None, **kwargs):
        return _og3d_logits(self.og3d_head, obj_embeds, obj_masks, self.training)
