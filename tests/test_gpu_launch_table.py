"""The native launch after it got one definition (sceneverse_amd/_launch.py): the same launches with the same profile
keys and per-launch accounting as the commit before (tests/golden/launch_table_parent.json), and wrappers that used to
take the bare `torch.cuda.current_stream()` still launch on the stream their inputs were made on."""
import json
import math

import pytest
import torch
import torch.nn.functional as F

from launch_table_cases import GOLDEN, launch_table

pytestmark = pytest.mark.gpu
DEV = "cuda"


def test_launch_table_equals_the_parent_commit():
    """Same key set, equal launch counts, MFMA dtypes and work-fraction flags; FLOPs and bytes per launch equal to 1e-9
    relative (integer expressions of the shapes and of seeded extent words).  Nothing timed is compared."""
    with open(GOLDEN) as f:
        want = json.load(f)
    got = launch_table(DEV)
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    for key, w in want.items():
        g = got[key]
        assert g["launches"] == w["launches"], (key, g["launches"], w["launches"])
        assert g["mfma_dtype"] == w["mfma_dtype"] and g["work_fraction"] == w["work_fraction"], (key, g, w)
        for field in ("flops_per_launch", "bytes_per_launch"):
            assert abs(g[field] - w[field]) <= 1e-9 * abs(w[field]), (key, field, g[field], w[field])


def test_wrappers_launch_on_the_side_stream_their_inputs_were_made_on():
    """Inputs made by torch ops on a fresh side stream -- behind a matrix product that keeps that stream busy, so that a
    launch on any other stream would read them before they are written -- and handed to the wrappers at once, no
    synchronisation in between, with the profiler on.  masked_ce (4 x 16) and l2_normalize (4 x 8) took the bare current
    stream before; add_dropout_layer_norm (4 x 256, its smallest width) did too and, unlike l2_normalize -- which records
    no profile entry, before or now -- is timed.  Results against torch within the bounds of the ops' own tests
    (test_gpu_losses.py: 1e-5 relative + 1e-6 on the loss, 1e-6 on the fp32 gradient; test_gpu_fused_norm.py: 1e-6 on
    l2_normalize, 2e-5 max(1, scale) on the fp32 LayerNorm rows); the timed launches report a finite, non-negative duration."""
    from sceneverse_amd.modules.layers.fused_norm import add_dropout_layer_norm, l2_normalize
    from sceneverse_amd.optim.loss.masked_ce import masked_cross_entropy
    from sceneverse_amd.pointnet2 import _ext
    norm = torch.nn.LayerNorm(256).to(DEV)
    with torch.no_grad():
        norm.weight.uniform_(0.5, 1.5)
        norm.bias.uniform_(-0.5, 0.5)
    labels = torch.tensor([3, -1, 15, 0], device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    _ext.profile_start()
    try:
        with torch.cuda.stream(s):
            busy = torch.randn(2048, 2048, device=DEV)
            zero = (busy @ busy).sum() * 0.0                    # finite: the inputs below wait for the product
            logits = (torch.randn(4, 16, device=DEV) * 3 + zero).requires_grad_(True)
            rows = torch.randn(4, 8, device=DEV) + zero
            x, h = torch.randn(4, 256, device=DEV) + zero, torch.randn(4, 256, device=DEV) + zero
            loss = masked_cross_entropy(logits, labels, ignore_index=-1)
            loss.backward()
            unit = l2_normalize(rows)
            y = add_dropout_layer_norm(x, h, norm)
        s.synchronize()
    finally:
        rec = _ext.profile_stop()
    ref_in = logits.detach().clone().requires_grad_(True)
    ref = F.cross_entropy(ref_in, labels, ignore_index=-1)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * abs(ref.item()) + 1e-6, (loss.item(), ref.item())
    assert (logits.grad - ref_in.grad).abs().max().item() <= 1e-6
    assert (unit - F.normalize(rows, dim=-1, p=2)).abs().max().item() <= 1e-6
    want = norm(x + h)
    assert (y - want).abs().max().item() <= 2e-5 * max(1.0, want.abs().max().item())
    timed = {k.split("(")[0]: v for k, v in rec.items()}
    assert {"masked_ce_forward", "masked_ce_backward", "add_dropout_layernorm_forward"} <= set(timed), sorted(rec)
    assert not any("l2_normalize" in k for k in rec)
    for k, v in timed.items():
        assert v["launches"] == 1 and math.isfinite(v["avg_us"]) and v["avg_us"] >= 0.0, (k, v)
