"""Plain and packed attention, with dropout, against an fp64 reference of the same operation -- through
_FusedSelfAttention, _FusedVarlenSelfAttention and _FusedCrossAttention, in every plain mode a call can take (0 whole-
sequence, 3 block-streaming, 4 K / V-resident, 9 = 1 | 8 block-streaming forward + one-launch backward, 13 = 1 | 4 | 8
the product default), never against another kernel.  tests/attention_cases.py has the references, the one-hot read-out
and the acceptance function; tests/test_attention_cases_host.py shows on the CPU that they can fail.

Inputs: bf16 randn, the q columns scaled by 0.5 so that every live probability is far above bf16 underflow.

Per case and mode:
  p = 0, real V   out, dq, dk, dv against the fp64 reference: out <= 2e-2 max|ref|, gradients <= 4e-2 max|ref|, every
                  rel-L2 <= 1e-2; exact zeros in dk / dv of padded keys and in dq of rows past q_limit; everything
                  compared is finite although the seven rows behind the last packed sequence are NaN in `packed` and in
                  the cotangent.
  p = 0, read-out every live pair reads non-zero and within 2^-7 relative of the fp64 softmax.
  p > 0, read-out every entry is 0 or within 2^-7 of P / (1 - p); the keep rate is within five binomial standard deviations
                  + 2^-16 of 1 - p; a second call gives the same mask, another seed_dev value another one; the backward's
                  dV product read the same way (one-hot cotangent) drew the forward's mask bit for bit; the mask is
                  bit-identical across all modes of the case (the shared stream of gps_attn_set_plain_blocks).
  p > 0, real V   out, dq, dk, dv against the fp64 reference that applies the read-out mask, same bars, for every mode and
                  for forward mode 3 with backward mode 9 and forward mode 0 with backward mode 13.

Worst values measured on an MI355X against the fp64 reference, over all 94 cases (max error / max|ref|; rel-L2):
  out        3.9e-3  mode 0, fixed L = 257, p = 0             rel-L2 2.3e-3  spatial L = 80, p = 0.1
  dq         9.6e-3  mode 3, packed cap 64, q_limit, p = 0.1   rel-L2 7.2e-3  modes 3 / 9, fixed L = 17, p = 0.1
  dk         2.4e-2  modes 3 / 9, fixed L = 17, p = 0.1        rel-L2 7.4e-3  the same
  dv         4.5e-3  mode 0, cross (1, 70), p = 0              rel-L2 2.4e-3  mode 3, fixed L = 129, p = 0.1
  dsw        5.4e-3  spatial L = 200, p = 0
  read-out   7.71e-3 of the bar's 7.81e-3: every mode, packed cap 128, p = 0 (every case and mode lies between 7.2e-3 and
             7.7e-3: two bf16 roundings at their worst, found among 1e5 .. 1e7 entries)
  keep rate  0.900091 over the 6.7e6 pairs of packed cap 320 (the 16-bit threshold keeps 1 - 6553 / 65536 = 0.900009);
             0.875 = 21 of the 24 pairs of fixed L = 1
  masks      bit-identical across all modes of every case, between forward and the backward's dV product, and between
             calls; the typical rel-L2 of every gradient is 2.3e-3 .. 2.5e-3 in every mode

What these tests found.  A row with ONE live key has dq = dk = 0 in exact arithmetic.  With dropout its output is
bf16(v / (1 - p)), and a backward that takes delta = rowsum(dout * out) from it keeps dout . (out - bf16(out)) in dS
where the truth is 0.  cross (65, 64), p = 0.1 (second batch row: one live key) measured dk 7.9e-2 of max|ref| and rel-L2
1.25e-2 (dq) / 1.22e-2 (dk) on the whole-sequence streaming backward of gps_attention.hip, which serves every cross-
attention backward: over the bars.  That kernel now forms delta = rowsum(P' dP') from the probabilities when dropout is on
(plain form), as the K / V-resident kernels do: the case measures dk 3.3e-3, rel-L2 2.3e-3.  The block-streaming and the
one-launch backward (modes 3 and 9) still take delta from the output; fixed L = 17 (second row: one live key) shows it
above, inside the bars, against 2.3e-3 in modes 0, 4 and 13.  At fixed L = 1 both references are identically zero and the
error is measured against the whole gradient's scale (tests/attention_cases.py): dq 4.1e-3, dk 2.1e-3 in modes 3 / 9,
3.5e-8 in modes 0 / 4 / 13.
"""
import functools
import json
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import attention_cases as AC  # noqa: E402
from sceneverse_amd.modules.layers import fused_attention as FA  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
H, D = AC.H, AC.D
P_DROP = 0.1
SEED = 77
CROSSED = ((3, 9), (0, 13))                 # (forward mode, backward mode)


def _randn(shape, g, q_cols=True):
    x = torch.randn(*shape, generator=g)
    if q_cols:
        x[..., :D] *= 0.5
    return x.to(torch.bfloat16)


def _seed_word(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


class _Case:
    """one layout with its inputs on the device and what its launches need besides them"""

    def __init__(self, name, layout, inputs, dout, apply, modes, crossed=CROSSED):
        self.name, self.layout, self.apply, self.modes, self.crossed = name, layout, apply, modes, crossed
        self.inputs, self.dout = [t.to(DEV) for t in inputs], dout.to(DEV)
        self._p0 = None

    def p0(self):
        """the p = 0 reference (out, gradients, P): computed once per case, never modified"""
        if self._p0 is None:
            self._p0 = AC.reference(self.layout, self.inputs, self.dout)
            self._p0["P"] = self._p0["P"].to(DEV)
        return self._p0

    def driver(self, fwd_mode, bwd_mode, p, seed_word=12345):
        seed_dev = _seed_word(seed_word) if p else None

        def run(inputs, dout):
            FA.set_plain_mode(fwd_mode)
            FA.set_spatial_planes(False)            # the spatial cases stay on the general kernels at p = 0 too
            try:
                xs = [t.clone().requires_grad_(dout is not None) for t in inputs]
                out = self.apply(xs, p, seed_dev)
                if dout is None:
                    return out.detach(), None
                FA.set_plain_mode(bwd_mode)
                return out.detach(), list(torch.autograd.grad(out, xs, dout))
            finally:
                FA.set_plain_mode()
                FA.set_spatial_planes(True)
        return run


def _report(case, mode, p, figures):
    flat = {k: (v[0] if isinstance(v, tuple) else v) for k, v in figures.items()}
    flat.update({k + " rel-L2": v[1] for k, v in figures.items() if isinstance(v, tuple) and v[1] is not None})
    print("attention-reference", json.dumps({"case": case.name, "mode": mode, "p": p, **flat}))


def _accept(case, run, ref, missed, what):
    """the figures of one run against the reference; bars that were missed go onto `missed` (raised at the case's end, so
    that one mode's miss does not hide the figures of the others)"""
    out, grads = run(case.inputs, case.dout)
    try:
        return AC.accept(case.layout, dict(out=out, **case.layout.split(grads)), ref)
    except AC.Missed as e:
        missed.append((what, e.args[0]))
        return e.figures


def _check(case, p):
    lay, ref0 = case.layout, case.p0()
    masks, missed = {}, []
    for mode in case.modes:
        run = case.driver(mode, mode, p)
        mask, rel, rate = AC.check_readout(AC.read_forward(lay, run, case.inputs), ref0["P"], lay.live, p)
        figures = {"read-out": rel}
        if p == 0.0:
            figures.update(_accept(case, run, ref0, missed, f"mode {mode}"))
        else:
            figures["keep rate"] = rate
            again = AC.read_forward(lay, run, case.inputs)
            AC.same_mask((again != 0) & lay.live.to(DEV), mask, f"mode {mode}: a second call drew another mask")
            # a case of n live pairs repeats its mask under another word with probability (1 - 2 p (1 - p))^n: 0.8 % at
            # the 24 pairs of L = 1, so the smallest cases may need a second word; every other case differs at the first
            for word in (12346, 12347, 12348):
                other = AC.read_forward(lay, case.driver(mode, mode, p, seed_word=word), case.inputs)
                if not torch.equal((other != 0) & lay.live.to(DEV), mask):
                    break
            else:
                raise AssertionError(f"mode {mode}: seed_dev does not move the mask")
            assert word == 12346 or int(lay.live.sum()) < 100, f"mode {mode}: seed_dev word 12346 repeats the mask"
            back = AC.read_backward(lay, run, case.inputs)
            AC.same_mask((back != 0) & lay.live.to(DEV), mask, f"mode {mode}: the backward drew another mask than the forward")
            masks[mode] = mask
        _report(case, mode, p, figures)
    if p == 0.0:
        assert not missed, (case.name, missed)
        return
    first = case.modes[0]
    for mode in case.modes[1:]:
        AC.same_mask(masks[mode], masks[first], f"modes {first} and {mode} draw different streams")
    ref = AC.reference(lay, case.inputs, case.dout, masks[first], p)
    for fwd, bwd in [(m, m) for m in case.modes] + list(case.crossed):
        what = fwd if fwd == bwd else f"{fwd}/{bwd}"
        _report(case, what, p, _accept(case, case.driver(fwd, bwd, p), ref, missed, f"mode {what}"))
    assert not missed, (case.name, missed)


# ---------------------------------------------------------------------------------------------------------------
# a. fixed length with a key-padding mask
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixed_case(L):
    g = torch.Generator().manual_seed(1000 + L)
    n_real = torch.tensor([L, int(torch.randint(1, L + 1, (1,), generator=g))])       # one full row, one random prefix
    mask = torch.arange(L)[None, :] >= n_real[:, None]
    mask_d = mask.to(DEV)

    def apply(xs, p, seed_dev):
        return FA._FusedSelfAttention.apply(xs[0], None, mask_d, H, p, SEED, seed_dev)
    modes = [0, 3] + ([4] if L <= 144 else []) + [9, 13]
    return _Case(f"fixed L={L}", AC.Fixed(2, L, mask), [_randn((2, L, 3 * D), g)], _randn((2, L, D), g, False), apply, modes)


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L", [1, 17, 64, 65, 128, 129, 192, 193, 256, 257, 320])
def test_fixed_length_with_key_padding(L, p):
    _check(_fixed_case(L), p)


# ---------------------------------------------------------------------------------------------------------------
# b. packed variable length
# ---------------------------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 300, 320)
TAIL = 7


@functools.lru_cache(maxsize=None)
def _packed_inputs(cap):
    g = torch.Generator().manual_seed(2000 + cap)
    lens = [n for n in LENGTHS if n <= cap]
    lens = [lens[i] for i in torch.randperm(len(lens), generator=g).tolist()]
    T = sum(lens) + TAIL
    packed, dout = _randn((T, 3 * D), g), _randn((T, D), g, False)
    packed[T - TAIL:] = float("nan")
    dout[T - TAIL:] = float("nan")
    limit = [(1, max(1, n // 2), n + 5)[i % 3] for i, n in enumerate(lens)]
    orders = {"natural": None, "longest": torch.argsort(torch.tensor(lens), descending=True, stable=True).to(torch.int32),
              "random": torch.randperm(len(lens), generator=g).to(torch.int32)}
    return lens, packed, dout, limit, orders


@functools.lru_cache(maxsize=None)
def _packed_case(cap, order, use_limit):
    lens, packed, dout, limit, orders = _packed_inputs(cap)
    if order != "natural":                       # the results do not depend on the order: one reference serves all three
        base = _packed_case(cap, "natural", use_limit)
    lay = AC.Packed(lens, cap, TAIL, limit if use_limit else None)
    cu_d = torch.tensor(lay.cu, dtype=torch.int32, device=DEV)
    order_d = orders[order].to(DEV) if orders[order] is not None else None
    limit_d = torch.tensor(limit, dtype=torch.int32, device=DEV) if use_limit else None

    def apply(xs, p, seed_dev):
        return FA._FusedVarlenSelfAttention.apply(xs[0], cu_d, len(lens), cap, H, p, seed_dev, order_d, limit_d)
    case = _Case(f"packed cap={cap} order={order} q_limit={int(use_limit)}", lay, [packed], dout, apply, [0, 3, 13])
    if order != "natural":
        case._p0 = base.p0()
    return case


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("use_limit", [False, True])
@pytest.mark.parametrize("order", ["natural", "longest", "random"])
@pytest.mark.parametrize("cap", [64, 128, 192, 256, 320])
def test_packed_variable_length(cap, order, use_limit, p):
    _check(_packed_case(cap, order, use_limit), p)


# ---------------------------------------------------------------------------------------------------------------
# c. cross-attention
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cross_case(Lq, Lk):
    g = torch.Generator().manual_seed(3000 + Lq + Lk)
    n_real = torch.tensor([Lk, int(torch.randint(1, Lk + 1, (1,), generator=g))])
    mask = torch.arange(Lk)[None, :] >= n_real[:, None]
    mask_d = mask.to(DEV)

    def apply(xs, p, seed_dev):
        return FA._FusedCrossAttention.apply(xs[0], xs[1], mask_d, H, p, seed_dev)
    return _Case(f"cross Lq={Lq} Lk={Lk}", AC.Cross(2, Lq, Lk, mask), [_randn((2, Lq, D), g), _randn((2, Lk, 2 * D), g, False)],
                 _randn((2, Lq, D), g, False), apply, [0, 13])


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("Lq,Lk", [(1, 70), (50, 80), (65, 64), (130, 300)])
def test_cross_attention(Lq, Lk, p):
    _check(_cross_case(Lq, Lk), p)


# ---------------------------------------------------------------------------------------------------------------
# d. the spatial form on the general kernels (the plane form refuses dropout)
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _spatial_case(L):
    g = torch.Generator().manual_seed(4000 + L)
    n_real = torch.tensor([L, int(torch.randint(L // 3, L + 1, (1,), generator=g))])
    mask = torch.arange(L)[None, :] >= n_real[:, None]
    packed = torch.randn(2, L, 3 * D + 6 * H, generator=g)
    packed[..., :D] *= 0.5
    packed[..., 3 * D:] *= 2.0
    pl = torch.rand(2, L, L, 5, generator=g) * 2 - 1
    mask_d, pl_d = mask.to(DEV), pl.to(DEV)

    def apply(xs, p, seed_dev):
        return FA._FusedSelfAttention.apply(xs[0], pl_d, mask_d, H, p, SEED, seed_dev)
    return _Case(f"spatial L={L}", AC.Fixed(2, L, mask, pl), [packed.to(torch.bfloat16)], _randn((2, L, D), g, False), apply,
                 [0], crossed=())


@pytest.mark.parametrize("p", [0.0, P_DROP])
@pytest.mark.parametrize("L", [80, 200])
def test_spatial_form_on_the_general_kernels(L, p):
    _check(_spatial_case(L), p)
