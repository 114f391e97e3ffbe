"""Host logic of the lock-step Linear / FFN nodes (modules/layers/gemm.py drive_pair) without a GPU: `_launch` and
`_launch_together` are replaced by a torch emulation of the products they are handed, so that what the nodes prepare,
in which groups it leaves and what comes back can be checked on CPU bf16 tensors.

* two stacks driven in lock-step == driven one after the other, exactly (the emulation is deterministic per product);
* the forward products of the common depth leave in pairs, the deeper stack's tail alone;
* with a paired backward the input-gradient products of the common depth leave in pairs, forward-only pairing leaves
  them alone;
* a backward call that brings one side's gradient leaves the other side's parameters untouched;
* nothing stays behind in module state keyed by a tensor id."""
import pytest
import torch

from sceneverse_amd._native import EPI_BIAS, EPI_BIAS_RELU, EPI_DRELU, EPI_F32, GEMM_NN, GEMM_NT, GEMM_TN
from sceneverse_amd.modules.layers import gemm

D, FF = 16, 32


def _emulate(q):
    """What gps_gemm_bf16 computes for the product q, on the tensors q.keep pins (p_drop = 0, no row extent)."""
    A, B, C, bias, aux, _aux_out, _ws, colsum, _seed, extent = q.keep
    a = q.args
    assert extent is None and a.p_drop == 0.0
    if q.form == GEMM_NT:                                    # C (M, N) = A (M, K) B (N, K)^T + bias
        assert A.shape == (a.M, a.K) and B.shape == (a.N, a.K) and q.epilogue in (EPI_BIAS, EPI_BIAS_RELU)
        acc = A.float() @ B.float().t()
        if bias is not None:
            acc = acc + bias.float()
        C.copy_(torch.relu(acc) if q.epilogue == EPI_BIAS_RELU else acc)
    elif q.form == GEMM_NN:                                  # C (M, N) = A (M, K) B (K, N) [x relu'(aux)]
        assert A.shape == (a.M, a.K) and B.shape == (a.K, a.N) and q.epilogue in (EPI_BIAS, EPI_DRELU) and bias is None
        acc = A.float() @ B.float()
        C.copy_(acc * (aux.float() > 0) if q.epilogue == EPI_DRELU else acc)
    else:                                                    # C (M, N) fp32 = A (K, M)^T B (K, N), colsum (M) = column sums of A
        assert q.form == GEMM_TN and q.epilogue == EPI_F32 and A.shape == (a.K, a.M) and B.shape == (a.K, a.N)
        C.copy_(A.float().t() @ B.float())
        if colsum is not None:
            colsum.copy_(A.float().sum(0))


def _desc(q):
    return (q.form, q.epilogue, q.args.M, q.args.N, q.args.K)


@pytest.fixture
def launches(monkeypatch):
    """-> the log of launches: one tuple of (form, epilogue, M, N, K) per call of `_launch_together` (and per lone
    `_launch`), in order."""
    log = []

    def launch(q):
        log.append((_desc(q),))
        _emulate(q)

    def launch_together(products):
        products = [q for q in products if q is not None]
        log.append(tuple(_desc(q) for q in products))
        for q in products:
            _emulate(q)

    monkeypatch.setattr(gemm, "_launch", launch)
    monkeypatch.setattr(gemm, "_launch_together", launch_together)
    monkeypatch.setattr(gemm, "twin_stacks", lambda: True)
    yield log
    gemm.set_twin_backward(True)
    gemm.clear_shadows()


def _stack(layers, seed):
    torch.manual_seed(seed)
    return torch.nn.ModuleList([torch.nn.ModuleDict({
        "qkv": torch.nn.Linear(D, 3 * D), "out": torch.nn.Linear(D, D), "l1": torch.nn.Linear(D, FF), "l2": torch.nn.Linear(FF, D)})
        for _ in range(layers)])


def _stack_gen(mods, x):
    for m in mods:
        p = yield gemm.LinearOp.of(x, [m["qkv"]])
        h = torch.tanh(p[..., :x.shape[-1]].float()).to(torch.bfloat16)
        o = yield gemm.LinearOp.of(h, [m["out"]])
        f = yield gemm.FFNOp(o, m["l1"], m["l2"], "relu", 0.0, False)
        x = (o.float() + f.float()).to(torch.bfloat16)
    return x


def _inputs():
    g = torch.Generator().manual_seed(5)
    return torch.randn(5, D, generator=g).to(torch.bfloat16), torch.randn(2, 3, D, generator=g).to(torch.bfloat16)


def _no_id_keyed_state():
    assert not getattr(gemm, "_PRECOMPUTED", None)


def _layer(form_rows, paired):
    """The forward (NT) or input-gradient (NN) launches of one layer, in launch order, for the row counts given."""
    def calls(form, epi, N, K):
        per_side = [(form, epi, M, N, K) for M in form_rows]
        return [tuple(per_side)] if paired else [(s,) for s in per_side]
    return calls


@pytest.mark.parametrize("twin_backward", [True, False], ids=["paired-backward", "forward-only"])
def test_lock_step_equals_sequential_and_pairs_its_launches(launches, twin_backward):
    gemm.set_twin_backward(twin_backward)
    sa, sb = _stack(1, 1), _stack(2, 2)
    params = list(sa.parameters()) + list(sb.parameters())
    xa0, xb0 = _inputs()
    res, logs = {}, {}
    for mode in ("sequential", "paired"):
        for p in params:
            p.grad = None
        xa, xb = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
        del launches[:]
        if mode == "paired":
            ya, yb = gemm.drive_pair(_stack_gen(sa, xa), _stack_gen(sb, xb))
        else:
            ya, yb = gemm.drive(_stack_gen(sa, xa)), gemm.drive(_stack_gen(sb, xb))
        forward = list(launches)
        del launches[:]
        (ya.float().square().mean() + yb.float().square().mean()).backward()
        logs[mode] = (forward, list(launches))
        res[mode] = [ya.detach(), yb.detach(), xa.grad, xb.grad] + [p.grad.clone() for p in params]
        _no_id_keyed_state()
    # (a) same numbers, exactly
    assert all(g is not None for g in res["paired"])
    for i, (s, p) in enumerate(zip(res["sequential"], res["paired"])):
        assert s.shape == p.shape and s.dtype == p.dtype and torch.equal(s, p), f"tensor {i}"
    forward, backward = logs["paired"]
    # (b) forward: the common layer's four stages as 2-product calls, stack b's second layer alone
    assert all(q[0] == GEMM_NT for call in forward for q in call)
    both, tail = _layer((5, 6), True), _layer((6,), False)
    assert forward == (both(GEMM_NT, EPI_BIAS, 3 * D, D) + both(GEMM_NT, EPI_BIAS, D, D)
                       + both(GEMM_NT, EPI_BIAS_RELU, FF, D) + both(GEMM_NT, EPI_BIAS, D, FF)
                       + tail(GEMM_NT, EPI_BIAS, 3 * D, D) + tail(GEMM_NT, EPI_BIAS, D, D)
                       + tail(GEMM_NT, EPI_BIAS_RELU, FF, D) + tail(GEMM_NT, EPI_BIAS, D, FF))
    assert all(len(call) == 1 for call in logs["sequential"][0])
    # (c) backward: stack b's second layer alone, then the common layer -- paired with a paired backward, else one by one
    dgrads = [call for call in backward if call[0][0] == GEMM_NN]
    assert all(q[0] == GEMM_NN for call in dgrads for q in call)
    assert all(len(call) == 1 and call[0][0] == GEMM_TN for call in backward if call not in dgrads)
    assert dgrads[:4] == (tail(GEMM_NN, EPI_DRELU, FF, D) + tail(GEMM_NN, EPI_BIAS, D, FF)
                          + tail(GEMM_NN, EPI_BIAS, D, D) + tail(GEMM_NN, EPI_BIAS, D, 3 * D))
    if twin_backward:
        assert dgrads[4:] == (both(GEMM_NN, EPI_DRELU, FF, D) + both(GEMM_NN, EPI_BIAS, D, FF)
                              + both(GEMM_NN, EPI_BIAS, D, D) + both(GEMM_NN, EPI_BIAS, D, 3 * D))
    else:
        assert all(len(call) == 1 for call in dgrads)
        for side in (_layer((5,), False), _layer((6,), False)):      # each stack's own chain, in its own order
            mine = side(GEMM_NN, EPI_DRELU, FF, D) + side(GEMM_NN, EPI_BIAS, D, FF) + side(GEMM_NN, EPI_BIAS, D, D) \
                + side(GEMM_NN, EPI_BIAS, D, 3 * D)
            rows = mine[0][0][2]
            assert [call for call in dgrads[4:] if call[0][2] == rows] == mine
        assert len(dgrads) == 12
    # every weight gradient once: 4 Linears per layer, 3 layers
    assert sum(1 for call in backward if call[0][0] == GEMM_TN) == 12


@pytest.mark.parametrize("twin_backward", [True, False], ids=["paired-node", "separate-nodes"])
def test_lock_step_backward_with_one_side_only(launches, twin_backward):
    gemm.set_twin_backward(twin_backward)
    sa, sb = _stack(1, 3), _stack(1, 4)
    xa0, xb0 = _inputs()
    xa, xb = xa0.clone().requires_grad_(True), xb0.clone().requires_grad_(True)
    ya, yb = gemm.drive_pair(_stack_gen(sa, xa), _stack_gen(sb, xb))
    _no_id_keyed_state()
    torch.autograd.backward(ya.float().sum(), inputs=[xa] + list(sa.parameters()), retain_graph=twin_backward)
    assert xa.grad is not None and all(p.grad is not None for p in sa.parameters())
    assert xb.grad is None and all(p.grad is None for p in sb.parameters())
    ga = [xa.grad.clone()] + [p.grad.clone() for p in sa.parameters()]
    torch.autograd.backward(yb.float().sum(), inputs=[xb] + list(sb.parameters()))
    assert xb.grad is not None and all(p.grad is not None for p in sb.parameters())
    for p in sa.parameters():
        p.grad = None
    xa2 = xa0.clone().requires_grad_(True)
    gemm.drive(_stack_gen(sa, xa2)).float().sum().backward()
    for i, (g, r) in enumerate(zip(ga, [xa2.grad] + [p.grad for p in sa.parameters()])):
        assert torch.equal(g, r), f"tensor {i}"
    _no_id_keyed_state()
