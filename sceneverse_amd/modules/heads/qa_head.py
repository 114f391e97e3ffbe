"""Question-answering head (reference modules/heads/qa_head.py:8-91): attention-flatten both
streams, fuse, classify -- the head of the ScanQA / SQA3D fine-tune configurations.

On GPU tensors the head runs on libgps_hip.so: `AttFlat` = the first Linear + GELU as one GEMM (`gemm.linear_gelu`
where `gemm.usable`, i.e. bf16 execution), training dropout on the hidden activations, then ONE launch for the glimpse
logits, the masked softmax over the tokens and the weighted pooling (`fused_attflat.attflat_pool`, csrc/gps_qa.hip) and
the merge GEMM; `QAHeadV1` = the fused LayerNorm for `fusion_norm` and `gemm.ffn` (GELU, p = 0.3) for `answer_cls`.
`gemm.ffn` needs feature counts that are multiples of 8: ScanQA's 8864 answers qualify, SQA3D's 706 do not, so that
configuration runs the first layer of `answer_cls` as `gemm.linear_gelu` and keeps torch's Linear for the last one.
CPU tensors keep the reference's formulation.  Parameter names and state-dict keys are the reference's (its
checkpoints load).

Backends of the pooling core (see `set_qa_backend`): "auto" = native where the library serves the call, "hip" = native
or an error (CPU tensors included), "torch" = the composition below on any tensor."""
import torch
import torch.nn.functional as F
from torch import nn

from ..build import HEADS_REGISTRY

_BACKEND = "auto"  # "auto" | "hip" | "torch"


def set_qa_backend(name: str) -> None:
    global _BACKEND
    if name not in ("auto", "hip", "torch"):
        raise ValueError(name)
    _BACKEND = name


def get_qa_backend() -> str:
    return _BACKEND


def _use_hip(x, h, w2, keep) -> bool:
    if _BACKEND == "torch" or (_BACKEND == "auto" and not x.is_cuda):
        return False
    from . import fused_attflat
    ok = fused_attflat.attflat_pool_usable(x, h, w2, keep)
    if _BACKEND == "hip" and not ok:
        raise RuntimeError("QA backend 'hip' requested for an unsupported call "
                           f"(x {tuple(x.shape)} {x.dtype}, hidden {tuple(h.shape)} {h.dtype}, glimpses {w2.shape[0]})")
    return ok


class FC(nn.Module):
    def __init__(self, in_size, out_size, pdrop=0., use_gelu=True):
        super().__init__()
        self.pdrop, self.use_gelu = pdrop, use_gelu
        self.linear = nn.Linear(in_size, out_size)
        if use_gelu:
            self.gelu = nn.GELU()
        if pdrop > 0:
            self.dropout = nn.Dropout(pdrop)

    def forward(self, x):
        from ..layers import gemm
        if self.use_gelu and _BACKEND != "torch" and gemm.usable(x, self.linear.in_features, self.linear.out_features):
            x = gemm.linear_gelu(x, self.linear)
        else:
            x = self.linear(x)
            if self.use_gelu:
                x = self.gelu(x)
        return self.dropout(x) if self.pdrop > 0 else x


class MLP(nn.Module):
    def __init__(self, in_size, mid_size, out_size, pdrop=0., use_gelu=True):
        super().__init__()
        self.fc = FC(in_size, mid_size, pdrop=pdrop, use_gelu=use_gelu)
        self.linear = nn.Linear(mid_size, out_size)

    def forward(self, x):
        return self.linear(self.fc(x))


def _linear(x, layer: nn.Linear):
    from ..layers import gemm
    if _BACKEND != "torch" and gemm.usable(x, layer.in_features, layer.out_features):
        return gemm.linear(x, layer.weight, layer.bias)
    return layer(x)


class AttFlat(nn.Module):
    """Learned soft pooling over tokens: `flat_glimpses` attention maps -> concat -> linear."""

    def __init__(self, hidden_size, flat_mlp_size=512, flat_glimpses=1, flat_out_size=1024, pdrop=0.1):
        super().__init__()
        self.mlp = MLP(hidden_size, flat_mlp_size, flat_glimpses, pdrop=pdrop, use_gelu=True)
        self.flat_glimpses = flat_glimpses
        self.linear_merge = nn.Linear(hidden_size * flat_glimpses, flat_out_size)

    def forward(self, x, x_mask, keep=None):
        """x (B, T, D); x_mask (B, T) True = padding (filled with -1e9 before the softmax), or None.  keep: the same mask
        the other way round (nonzero = valid token, bool or 0 / 1 integers) when the caller has it: no negation launches."""
        h = self.mlp.fc(x)
        if keep is None and x_mask is not None:
            keep = x_mask.logical_not()
        if _use_hip(x, h, self.mlp.linear.weight, keep):
            from .fused_attflat import attflat_pool
            return _linear(attflat_pool(x, h, self.mlp.linear.weight, self.mlp.linear.bias, keep), self.linear_merge)
        if x_mask is None and keep is not None:
            x_mask = keep.logical_not()
        att = self.mlp.linear(h)
        if x_mask is not None:
            att = att.masked_fill(x_mask.unsqueeze(2), -1e9)
        att = F.softmax(att, dim=1)                      # (B, T, G)
        pooled = torch.einsum('btg,btd->bgd', att, x)    # glimpse-major, as the reference's cat
        return self.linear_merge(pooled.flatten(1))


@HEADS_REGISTRY.register()
class QAHeadV1(nn.Module):
    def __init__(self, cfg, hidden_size=768, mlp_size=256, glimpse=1, flat_out_size=512, num_answers=8864):
        super().__init__()
        self.attflat_visual = AttFlat(hidden_size, mlp_size, glimpse, flat_out_size, 0.1)
        self.attflat_lang = AttFlat(hidden_size, mlp_size, glimpse, flat_out_size, 0.1)
        self.answer_cls = nn.Sequential(nn.Linear(flat_out_size, hidden_size), nn.GELU(),
                                        nn.Dropout(0.3), nn.Linear(hidden_size, num_answers))
        self.fusion_norm = nn.LayerNorm(flat_out_size)

    def _classify(self, fused):
        from ..layers import gemm
        lin1, drop, lin2 = self.answer_cls[0], self.answer_cls[2], self.answer_cls[3]
        if _BACKEND == "torch" or not gemm.usable(fused, lin1.in_features, lin1.out_features):
            return self.answer_cls(fused)
        if gemm.usable(fused, lin2.in_features, lin2.out_features):
            return gemm.ffn(fused, lin1, lin2, "gelu", drop.p, self.training)
        return lin2(drop(gemm.linear_gelu(fused, lin1)))           # e.g. SQA3D's 706 answers: not a multiple of 8

    def forward(self, obj_embeds, obj_masks, txt_embeds, txt_masks, **kwargs):
        object_feat = self.attflat_visual(obj_embeds, None, keep=obj_masks)
        lang_feat = self.attflat_lang(txt_embeds, None, keep=txt_masks)
        from ..layers import fused_norm
        if _BACKEND != "torch" and fused_norm.supported(lang_feat, object_feat, self.fusion_norm):
            fused = fused_norm.add_dropout_layer_norm(lang_feat, object_feat, self.fusion_norm)
        else:
            fused = self.fusion_norm(lang_feat + object_feat)
        return self._classify(fused)
