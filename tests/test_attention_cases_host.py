"""tests/attention_cases.py can fail: its read-out and its acceptance function are driven by a torch fp32 stand-in for
the attention kernels (attention_cases.StandIn) that applies a KNOWN dropout mask.  The right stand-in must give the mask
back bit for bit and pass; each deliberately wrong one must be rejected by the assertion named for its defect.  Also:
the packed variable-length reference equals the padded one on the same sequences.  No GPU."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_cases as AC  # noqa: E402

D, H = AC.D, AC.H
P_DROP = 0.1


def _randn(shape, g, q_cols=True):
    x = torch.randn(*shape, generator=g)
    if q_cols:
        x[..., :D] *= 0.5                        # live probabilities far above bf16 underflow
    return x.to(torch.bfloat16)


def _fixed(L, seed=0, n_real_last=None):
    g = torch.Generator().manual_seed(seed)
    n_real = torch.tensor([L, n_real_last if n_real_last is not None else max(1, L // 2)])
    mask = torch.arange(L)[None, :] >= n_real[:, None]
    lay = AC.Fixed(2, L, mask)
    return lay, [_randn((2, L, 3 * D), g)], _randn((2, L, D), g, False), g


def _packed(seed=1):
    g = torch.Generator().manual_seed(seed)
    lens = [17, 0, 65, 1, 30]
    lay = AC.Packed(lens, 128, tail=3, q_limit=[1, 4, 33, 7, 500])
    packed, dout = _randn((lay.T, 3 * D), g), _randn((lay.T, D), g, False)
    packed[lay.cu[-1]:] = float("nan")           # rows behind the last sequence are nobody's
    dout[lay.cu[-1]:] = float("nan")
    return lay, [packed], dout, g


def _cross(seed=2):
    g = torch.Generator().manual_seed(seed)
    Lq, Lk = 5, 70
    mask = torch.arange(Lk)[None, :] >= torch.tensor([Lk, 41])[:, None]
    lay = AC.Cross(2, Lq, Lk, mask)
    return lay, [_randn((2, Lq, D), g), _randn((2, Lk, 2 * D), g, False)], _randn((2, Lq, D), g, False), g


def _keep(lay, g, p=P_DROP):
    return torch.rand(lay.live.shape, generator=g) >= p


CASES = {"fixed17": lambda: _fixed(17), "fixed65": lambda: _fixed(65, seed=5), "packed": _packed, "cross": _cross}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("p", [0.0, P_DROP])
def test_the_right_stand_in_passes_and_its_mask_comes_back_bit_for_bit(case, p):
    lay, inputs, dout, g = CASES[case]()
    keep = _keep(lay, g) if p else None
    mask, figures = AC.examine(lay, AC.StandIn(lay, keep, p), inputs, dout, p)
    if p:
        assert torch.equal(mask, keep & lay.live)
    else:
        assert torch.equal(mask, lay.live.expand_as(mask))
    assert figures["read-out"] <= AC.READ_BAR and set(figures) >= {"out", "dq", "dk", "dv"}


def test_window_and_assembler_are_exact_inverses():
    """out = P V with the window as V reads P itself: the builder's ones sit where the assembler reads"""
    lay = AC.Packed([3, 0, 130], 192, tail=2)
    P = torch.rand(lay.T, H, 192, dtype=torch.float64)
    pieces = []
    for j in range(AC.n_windows(192)):
        win = AC.one_hot_window(lay.k_index, j).double().view(lay.T, H, 64)
        assert set(win.unique().tolist()) <= {0.0, 1.0} and (win.sum(-1) <= 1).all()
        piece = torch.zeros(lay.T, H, 64, dtype=torch.float64)
        for s, n in enumerate(lay.lens):
            r = slice(lay.cu[s], lay.cu[s] + n)
            piece[r] = torch.einsum("lht,thc->lhc", P[r, :, :n], win[r])
        pieces.append(piece.view(lay.T, D))
    R = AC.assemble(pieces, 192)
    assert torch.equal(R[lay.live], P.float()[lay.live])
    assert AC.one_hot_window(lay.k_index, 0)[lay.cu[-1]:].abs().sum() == 0        # rows of no sequence: no ones


def test_a_wrong_scale_is_rejected_by_the_read_out():
    """1 / sqrt(63) instead of 1 / 8 moves the largest logits by 1.5 %: inside the 2e-2 / 4e-2 max bars of the results
    (out, dk and dv pass all their bars; only dq's rel-L2, 1.04e-2, shows the 0.8 % of the scale itself), outside 2^-7
    of single probabilities"""
    lay, inputs, dout, _ = _fixed(65, seed=5)
    with pytest.raises(AssertionError, match="read-out: a non-zero entry is not P"):
        AC.examine(lay, AC.StandIn(lay, scale=1.0 / math.sqrt(63.0)), inputs, dout, 0.0)


def test_a_backward_mask_shifted_by_one_key_is_rejected_by_the_mask_comparison():
    lay, inputs, dout, g = _fixed(65, seed=5)
    keep = _keep(lay, g)
    with pytest.raises(AssertionError, match="mask: the backward drew another mask"):
        AC.examine(lay, AC.StandIn(lay, keep, P_DROP, bwd_keep=torch.roll(keep, 1, dims=-1)), inputs, dout, P_DROP)


def test_a_shifted_backward_mask_is_rejected_by_the_bars_too():
    lay, inputs, dout, g = _fixed(65, seed=5)
    keep = _keep(lay, g)
    ref = AC.reference(lay, inputs, dout, keep, P_DROP)
    out, grads = AC.StandIn(lay, keep, P_DROP, bwd_keep=torch.roll(keep, 1, dims=-1))(inputs, dout)
    with pytest.raises(AssertionError, match="d[qkv]: "):
        AC.accept(lay, dict(out=out, **lay.split(grads)), ref)


def test_q_limit_ignored_in_dk_is_rejected():
    lay, inputs, dout, g = _packed()
    for p in (0.0, P_DROP):
        keep = _keep(lay, g) if p else None
        with pytest.raises(AssertionError, match="dk: "):
            AC.examine(lay, AC.StandIn(lay, keep, p, dk_ignores_q_limit=True), inputs, dout, p)


def test_a_dropped_last_key_block_is_rejected():
    """65 tokens: key 64 is the whole last block.  Every query must read a non-zero probability there."""
    lay, inputs, dout, _ = _fixed(65, seed=5)
    with pytest.raises(AssertionError, match="read-out: live pairs read zero without dropout"):
        AC.examine(lay, AC.StandIn(lay, drop_last_block=True), inputs, dout, 0.0)


def test_one_pair_redrawn_by_the_backward_is_caught_by_the_mask_comparison_not_by_the_bars():
    lay, inputs, dout, g = _fixed(17)
    keep = _keep(lay, g)
    other = keep.clone()
    other[0, 3, 5, 7] = ~other[0, 3, 5, 7]
    wrong = AC.StandIn(lay, keep, P_DROP, bwd_keep=other)
    with pytest.raises(AssertionError, match="mask: the backward drew another mask.*1, 'pairs differ'"):
        AC.examine(lay, wrong, inputs, dout, P_DROP)                # reports exactly the one pair, before any bar is tried


def test_a_forward_that_draws_another_stream_is_caught_across_families():
    lay, inputs, dout, g = _fixed(17)
    keep = _keep(lay, g)
    other = keep.clone()
    other[1, 0, 11, 2] = ~other[1, 0, 11, 2]
    a, _ = AC.examine(lay, AC.StandIn(lay, keep, P_DROP), inputs, dout, P_DROP)
    b, _ = AC.examine(lay, AC.StandIn(lay, other, P_DROP), inputs, dout, P_DROP)     # consistent in itself: passes alone
    with pytest.raises(AssertionError, match="mask: families"):
        AC.same_mask(a, b, "families")


def test_a_wrong_keep_rate_is_rejected():
    lay, inputs, dout, g = _fixed(65, seed=5)
    keep = _keep(lay, g, 0.12)
    with pytest.raises(AssertionError, match="read-out: (keep rate|a non-zero entry)"):
        AC.examine(lay, AC.StandIn(lay, keep, P_DROP), inputs, dout, P_DROP)


def test_nonzero_gradients_of_padded_keys_and_skipped_queries_are_rejected():
    lay, inputs, dout, _ = _fixed(17)
    ref = AC.reference(lay, inputs, dout)
    out, grads = AC.StandIn(lay)(inputs, dout)
    got = dict(out=out, **lay.split(grads))
    AC.accept(lay, got, ref)
    got["dv"] = got["dv"].clone()
    got["dv"][1, 16, 5] = 1e-30
    with pytest.raises(AssertionError, match="dv: rows that must be exact zeros"):
        AC.accept(lay, got, ref)
    lay, inputs, dout, _ = _packed()
    ref = AC.reference(lay, inputs, dout)
    out, grads = AC.StandIn(lay)(inputs, dout)
    got = dict(out=out, **lay.split(grads))
    AC.accept(lay, got, ref)
    got["dq"] = got["dq"].clone()
    got["dq"][lay.cu[2] + 40, 0] = 1e-30
    with pytest.raises(AssertionError, match="dq: rows that must be exact zeros"):
        AC.accept(lay, got, ref)
    got = dict(got, out=torch.where(lay.out_rows[:, None], torch.tensor(float("nan")), out.float()))
    with pytest.raises(AssertionError, match="out: "):
        AC.accept(lay, got, ref)


def test_packed_reference_equals_the_padded_one():
    lay, inputs, dout, g = _packed()
    lay = AC.Packed(lay.lens, lay.cap, tail=3)                     # every row computed: the padded form has no q_limit
    n = lay.cu[-1]
    keep = _keep(lay, g)
    for p, kp in ((0.0, None), (P_DROP, keep)):
        packed_ref = AC.reference(lay, inputs, dout, kp, p)
        padded, mask = AC.padded_from_packed(inputs[0][:n], lay.lens, lay.cap)
        live_seq = ~mask.all(dim=1)                                # a zero-length sequence has no row in the padded batch
        dpad, _ = AC.padded_from_packed(dout[:n], lay.lens, lay.cap)
        kpad = None
        if kp is not None:
            kpad = torch.zeros(len(lay.lens), lay.cap, H, lay.cap, dtype=torch.bool)
            for s, m in enumerate(lay.lens):
                kpad[s, :m] = kp[lay.cu[s]:lay.cu[s] + m]
            kpad = kpad[live_seq]
        flay = AC.Fixed(int(live_seq.sum()), lay.cap, mask[live_seq])
        dpad = torch.where(mask[:, :, None], torch.zeros((), dtype=dpad.dtype), dpad)   # padded queries: no cotangent
        padded_ref = AC.reference(flay, [padded[live_seq]], dpad[live_seq], kpad, p)
        rows = ~mask[live_seq]
        for name in ("out", "dq", "dk", "dv"):
            a, b = packed_ref[name][:n], padded_ref[name][rows]
            assert (a - b).abs().max().item() <= 1e-12 * max(1.0, b.abs().max().item()), name
        assert (packed_ref["P"][:n][lay.live[:n]] - padded_ref["P"][rows][lay.live[:n]]).abs().max().item() <= 1e-14
