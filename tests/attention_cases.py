"""Host-side half of tests/test_gpu_attention_reference.py (the kernels) and tests/test_attention_cases_host.py (a torch
stand-in for them, right and deliberately wrong): fp64 references of the three attention forms, the one-hot read-out that
makes a kernel's probabilities and its dropout mask explicit, and the acceptance function.  Nothing here needs a GPU.

Layouts.  A *layout* describes one call: where q / k / v sit in its input tensors, which (query, head, key) pairs are
live, which rows are compared and which must be exact zeros.
  Fixed   packed (B, L, 3 D [+ 6 H]) = [q | k | v [| cond]], key-padding mask (B, L) (1 = padded key), optional pairwise
          tensor (B, L, L, 5): _FusedSelfAttention.
  Packed  packed (T, 3 D), sequences back to back at cu, capacity cap, optional q_limit: _FusedVarlenSelfAttention.  Rows
          past q_limit have no output to compare and their cotangent is zero; rows behind the last sequence belong to no
          one.  A zero-length sequence owns no rows: its contract is that its neighbours are what they are without it.
  Cross   q (B, Lq, D), kv (B, Lk, 2 D) = [k | v], key mask (B, Lk): _FusedCrossAttention.
A pair matrix is indexed [query row ..., head, key]: (B, Lq, H, Lk), packed (T, H, cap).

Read-out.  The dropout decision of pair (query l, key t) depends on the seed and the pair's index, not on V.  With V
replaced by the one-hot window j (v[t, 64 h + (t - 64 j)] = 1 for keys 64 j <= t < 64 j + 64, exact in bf16),
out[l, 64 h + c] IS the dropped, rescaled probability of pair (l, 64 j + c) of head h to output rounding; ceil(Lk / 64)
forward calls give the whole matrix.  The same trick on the cotangent (dout[l, 64 h + (l - 64 j)] = 1) makes
dv[t, 64 h + c] the probability of pair (64 j + c, t) as the BACKWARD drew it.  An entry is 0 (dropped) or P / (1 - p):
the non-zero pattern is the mask, and an fp64 reference out = ((P o M) / (1 - p)) V differentiated by autograd is exact
for out, dq, dk and dv with the real V.

Bars (tests/test_gpu_attention.py): out <= 2e-2 max|ref| and rel-L2 <= 1e-2; each of dq / dk / dv <= 4e-2 max|ref| and
rel-L2 <= 1e-2.  With a single live key dq and dk are zero in exact arithmetic while a kernel that takes delta =
rowsum(dout * out) from its bf16 output leaves the rounding of `out` times the cotangent there; a gradient whose
reference is identically zero is therefore measured against the scale of the whole gradient (dq | dk | dv), as
tests/test_gpu_attention_fused_bwd.py does.  Read-out: 2^-7 relative per entry (two bf16 roundings -- the probability, then the
output -- of at most 2^-8 each; the fast exponential adds 1e-6); keep rate within five binomial standard deviations + 2^-16 (the kernels compare 16-bit thresholds)."""
import math

import torch

H = 12
HD = 64
D = H * HD
READ_BAR = 2.0 ** -7
BARS = {"out": (2e-2, 1e-2), "dq": (4e-2, 1e-2), "dk": (4e-2, 1e-2), "dv": (4e-2, 1e-2), "dsw": (4e-2, None)}


# ---------------------------------------------------------------------------------------------------------------
# fp64 references
# ---------------------------------------------------------------------------------------------------------------
def _heads(x):
    """(B, L, D) -> (B, H, L, 64)"""
    return x.reshape(x.shape[0], x.shape[1], H, HD).transpose(1, 2)


def core(q, k, v, dead=None, keep=None, p=0.0, bias=None, scale=1.0 / math.sqrt(HD)):
    """q (B, Lq, D), k / v (B, Lk, D); dead (B, Lk) bool = keys with probability 0; keep (B, Lq, H, Lk) bool = the
    explicit dropout mask; bias (B, H, Lq, Lk) added to the logits.  -> out (B, Lq, D), P (B, Lq, H, Lk) (undropped)."""
    s = _heads(q) @ _heads(k).transpose(-1, -2) * scale
    if bias is not None:
        s = s + bias
    if dead is not None:
        s = s.masked_fill(dead[:, None, None, :], float("-inf"))
    P = torch.softmax(s, dim=-1)
    Pd = P if keep is None else P * keep.permute(0, 2, 1, 3).to(P.dtype) / (1.0 - p)
    out = (Pd @ _heads(v)).transpose(1, 2).reshape(q.shape[0], q.shape[1], D)
    return out, P.permute(0, 2, 1, 3)


def spatial_bias(sw, pl, dead):
    """log(clamp(sigmoid(w . pairwise + b), 1e-6)) of modules/layers/transformers.py:193-239; sw (B, L, H * 6), pl
    (B, L, L, 5) -> (B, H, L, L)"""
    B, L = sw.shape[:2]
    sw = sw.view(B, L, H, 6).permute(0, 2, 1, 3)
    loc = torch.sigmoid(torch.einsum("bhld,bltd->bhlt", sw[..., 1:], pl) + sw[..., :1])
    if dead is not None:
        loc = loc.masked_fill(dead[:, None, None, :], 0)
    return torch.log(torch.clamp(loc, min=1e-6))


def ref_self(packed, mask=None, keep=None, p=0.0, pl=None):
    """fixed-length self-attention with a key-padding mask (and the spatial term when `pl` is given)"""
    q, k, v = (packed[..., i * D:(i + 1) * D] for i in range(3))
    bias = spatial_bias(packed[..., 3 * D:], pl.to(packed.dtype), mask) if pl is not None else None
    return core(q, k, v, mask, keep, p, bias)


def ref_cross(q, kv, mask=None, keep=None, p=0.0):
    return core(q, kv[..., :D], kv[..., D:], mask, keep, p)


def ref_varlen(packed, lens, cap, q_limit=None, keep=None, p=0.0):
    """packed (T, 3 D), sequence s = the next lens[s] rows; keep (T, H, cap).  -> out (T, D) with zero rows where nothing
    is computed (past q_limit, behind the last sequence), P (T, H, cap) zero outside the sequences' own pairs."""
    T = packed.shape[0]
    outs, Ps, r0 = [], [], 0
    for s, n in enumerate(lens):
        n = int(n)
        if n == 0:
            continue
        nq = n if q_limit is None else min(n, max(int(q_limit[s]), 0))
        x = packed[r0:r0 + n][None]
        o, P = core(x[..., :D], x[..., D:2 * D], x[..., 2 * D:3 * D], None,
                    None if keep is None else keep[r0:r0 + n, :, :n][None], p)
        outs += [o[0, :nq], o.new_zeros(n - nq, D)]
        Pn = P.detach().new_zeros(n, H, cap)
        Pn[:nq, :, :n] = P[0, :nq].detach()
        Ps.append(Pn)
        r0 += n
    outs.append(packed.new_zeros(T - r0, D))
    Ps.append(packed.detach().new_zeros(T - r0, H, cap))
    return torch.cat(outs), torch.cat(Ps)


# ---------------------------------------------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------------------------------------------
class Fixed:
    vi, col0 = 0, 2 * D                     # V = inputs[vi][..., col0:col0 + D]

    def __init__(self, B, L, mask=None, pl=None):
        self.B, self.n_q, self.n_k, self.mask, self.pl = B, L, L, mask, pl
        self.k_index = self.q_index = torch.arange(L).expand(B, L)
        dead = mask if mask is not None else torch.zeros(B, L, dtype=torch.bool)
        self.live = (~dead)[:, None, None, :].expand(B, L, H, L)
        self.out_rows = self.grad_rows = torch.ones(B, L, dtype=torch.bool)
        self.zero_rows = {"dk": dead, "dv": dead} if dead.any() else {}

    def forward(self, inputs, keep, p):
        return ref_self(inputs[0], self.mask, keep, p, self.pl)

    def split(self, grads):
        g = grads[0]
        parts = {"dq": g[..., :D], "dk": g[..., D:2 * D], "dv": g[..., 2 * D:3 * D]}
        if self.pl is not None:
            parts["dsw"] = g[..., 3 * D:]
        return parts

    def query_major(self, mat):
        """(B, Lk, H, Lq) indexed [key row, head, query] -> [query row, head, key]"""
        return mat.transpose(1, 3)


class Cross(Fixed):
    vi, col0 = 1, D

    def __init__(self, B, Lq, Lk, mask=None):
        self.B, self.n_q, self.n_k, self.mask, self.pl = B, Lq, Lk, mask, None
        self.k_index, self.q_index = torch.arange(Lk).expand(B, Lk), torch.arange(Lq).expand(B, Lq)
        dead = mask if mask is not None else torch.zeros(B, Lk, dtype=torch.bool)
        self.live = (~dead)[:, None, None, :].expand(B, Lq, H, Lk)
        self.out_rows = torch.ones(B, Lq, dtype=torch.bool)
        self.grad_rows = None               # q and kv rows differ: everything is compared
        self.zero_rows = {"dk": dead, "dv": dead} if dead.any() else {}

    def forward(self, inputs, keep, p):
        return ref_cross(inputs[0], inputs[1], self.mask, keep, p)

    def split(self, grads):
        return {"dq": grads[0], "dk": grads[1][..., :D], "dv": grads[1][..., D:]}


class Packed:
    vi, col0 = 0, 2 * D

    def __init__(self, lens, cap, tail=0, q_limit=None):
        self.lens, self.cap, self.q_limit = [int(n) for n in lens], int(cap), q_limit
        assert max(self.lens) <= cap
        self.cu = [0]
        for n in self.lens:
            self.cu.append(self.cu[-1] + n)
        self.T = self.cu[-1] + tail
        self.n_q = self.n_k = cap
        self.k_index = torch.full((self.T,), -1, dtype=torch.long)
        self.out_rows = torch.zeros(self.T, dtype=torch.bool)
        self.live = torch.zeros(self.T, H, cap, dtype=torch.bool)
        for s, n in enumerate(self.lens):
            r0 = self.cu[s]
            nq = n if q_limit is None else min(n, max(int(q_limit[s]), 0))
            self.k_index[r0:r0 + n] = torch.arange(n)
            self.out_rows[r0:r0 + nq] = True
            self.live[r0:r0 + nq, :, :n] = True
        self.q_index = self.k_index
        self.grad_rows = self.k_index >= 0
        skipped = self.grad_rows & ~self.out_rows
        self.zero_rows = {"dq": skipped} if skipped.any() else {}

    def forward(self, inputs, keep, p):
        return ref_varlen(inputs[0], self.lens, self.cap, self.q_limit, keep, p)

    def split(self, grads):
        g = grads[0]
        return {"dq": g[..., :D], "dk": g[..., D:2 * D], "dv": g[..., 2 * D:3 * D]}

    def query_major(self, mat):
        """(T, H, cap) indexed [key row, head, query] -> [query row, head, key], sequence by sequence"""
        res = torch.zeros_like(mat)
        for s, n in enumerate(self.lens):
            r0 = self.cu[s]
            res[r0:r0 + n, :, :n] = mat[r0:r0 + n, :, :n].permute(2, 1, 0)
        return res


def padded_from_packed(packed, lens, cap):
    """the same sequences as one fixed-length batch: (B, cap, W) zero-padded, mask (B, cap) with 1 = padded key"""
    B = len(lens)
    out = packed.new_zeros(B, cap, packed.shape[-1])
    mask = torch.ones(B, cap, dtype=torch.bool)
    r0 = 0
    for s, n in enumerate(lens):
        out[s, :n] = packed[r0:r0 + n]
        mask[s, :n] = False
        r0 += n
    return out, mask


def reference(layout, inputs, dout, keep=None, p=0.0):
    """fp64 forward + autograd backward of the layout's operation on the SAME (bf16-exact) inputs.  Rows that are not
    computed take a zero cotangent, whatever `dout` holds there.  -> {"out", "dq", "dk", "dv" [, "dsw"], "P"}"""
    xs = [t.detach().cpu().double().requires_grad_(True) for t in inputs]
    out, P = layout.forward(xs, None if keep is None else keep.cpu(), p)
    go = torch.where(layout.out_rows[..., None], dout.detach().cpu().double(), torch.zeros((), dtype=torch.float64))
    grads = torch.autograd.grad(out, xs, go)
    res = {"out": out.detach(), "P": P.detach()}
    res.update(layout.split(grads))
    return res


# ---------------------------------------------------------------------------------------------------------------
# one-hot windows and the read-out
# ---------------------------------------------------------------------------------------------------------------
def one_hot_window(index, j, dtype=torch.bfloat16):
    """index (...) = a row's position inside its sequence (-1: none) -> (..., D) with [..., 64 h + (index - 64 j)] = 1
    for every head where 64 j <= index < 64 j + 64, zero elsewhere"""
    c = index - HD * j
    hit = (c >= 0) & (c < HD)
    win = torch.zeros(*index.shape, H, HD, dtype=dtype)
    win[hit] = torch.nn.functional.one_hot(c[hit], HD).to(dtype)[:, None, :].expand(-1, H, -1)
    return win.reshape(*index.shape, D)


def with_values(inputs, layout, window):
    """`inputs` with V replaced by the window (rows outside every sequence keep what they hold, NaN in the tests)"""
    res = [t.clone() for t in inputs]
    own = (layout.k_index >= 0).to(window.device)
    v = res[layout.vi][..., layout.col0:layout.col0 + D]
    res[layout.vi][..., layout.col0:layout.col0 + D] = torch.where(own[..., None], window.to(v.dtype), v)
    return res


def assemble(pieces, n):
    """pieces[j] (..., D) = what came back for window j -> (..., H, n): entry [..., h, 64 j + c] = pieces[j][..., 64 h + c]"""
    return torch.cat([x.reshape(*x.shape[:-1], H, HD) for x in pieces], dim=-1)[..., :n].float()


def n_windows(n):
    return (n + HD - 1) // HD


def read_forward(layout, run, inputs):
    """run(inputs, None) -> (out, None).  -> (query rows ..., H, n_k): the kernel's dropped, rescaled probabilities"""
    dev = inputs[0].device
    return assemble([run(with_values(inputs, layout, one_hot_window(layout.k_index, j).to(dev)), None)[0].detach()
                     for j in range(n_windows(layout.n_k))], layout.n_k)


def read_backward(layout, run, inputs):
    """run(inputs, dout) -> (out, grads).  The probabilities as the backward's dV product drew them, query-major."""
    dev = inputs[0].device
    dvs = []
    for j in range(n_windows(layout.n_q)):
        dout = one_hot_window(layout.q_index, j).to(dev)
        if (layout.q_index < 0).any():                           # rows of no sequence: NaN, never to be read
            dout[(layout.q_index < 0).to(dev)] = float("nan")
        dvs.append(layout.split(run(inputs, dout)[1])["dv"].detach())
    return layout.query_major(assemble(dvs, layout.n_q))


def check_readout(R, P, live, p=0.0):
    """R = a read-out, P = the fp64 softmax, live = the pairs that exist.  -> (mask, worst relative error of a non-zero
    entry, keep rate).  Asserts what tests/test_gpu_attention_reference.py's docstring states per read-out."""
    live = live.to(R.device)
    got, want = R[live].double(), P.to(R.device)[live] / (1.0 - p)
    kept = got != 0
    if p == 0.0:
        assert bool(kept.all()), ("read-out: live pairs read zero without dropout", int((~kept).sum()))
    assert bool(kept.any()), "read-out: nothing was kept"
    rel = ((got - want).abs() / want)[kept].max().item()
    assert rel <= READ_BAR, ("read-out: a non-zero entry is not P / (1 - p)", rel, READ_BAR)
    rate = kept.double().mean().item()
    if p > 0.0:
        slack = 5.0 * math.sqrt(p * (1.0 - p) / kept.numel()) + 2.0 ** -16
        assert abs(rate - (1.0 - p)) <= slack, ("read-out: keep rate", rate, 1.0 - p, slack)
    return (R != 0) & live, rel, rate


def same_mask(a, b, what):
    """bit for bit"""
    n = int((a != b.to(a.device)).sum())
    assert n == 0, (f"mask: {what}", n, "pairs differ")


# ---------------------------------------------------------------------------------------------------------------
# acceptance
# ---------------------------------------------------------------------------------------------------------------
class Missed(AssertionError):
    """what accept() raises: every bar that was missed, with all the figures it measured in .figures"""

    def __init__(self, failures, figures):
        super().__init__(failures)
        self.figures = figures


def accept(layout, got, ref):
    """got = {"out", "dq", "dk", "dv" [, "dsw"]} from the kernel, ref = reference(...).  Compared on the rows that exist
    (out: computed rows; gradients: rows of a sequence); exact zeros where the contract says so.  -> {name: (max error /
    max|ref|, rel-L2)}.  NaN or inf anywhere compared misses its bar.  Every quantity is measured before Missed lists
    the bars that were not met."""
    figures, failures = {}, []
    grads = [n for n in ("dq", "dk", "dv") if n in ref]
    for name, (bar_max, bar_l2) in BARS.items():
        if name not in ref:
            continue
        rows = layout.out_rows if name == "out" else layout.grad_rows
        a, b = got[name].detach().cpu().double(), ref[name]
        if rows is not None:
            a, b = a[rows], b[rows]
        scale, norm = b.abs().max().item(), b.norm().item()
        if scale == 0.0 and name in grads:          # single live key: see the module docstring
            scale = max(ref[n].abs().max().item() for n in grads)
            norm = math.sqrt(sum(ref[n].norm().item() ** 2 for n in grads))
        err, l2 = (a - b).abs().max().item() / scale, (a - b).norm().item() / norm
        if not err <= bar_max:
            failures.append((f"{name}: max error over max|ref|", err, bar_max))
        if bar_l2 is not None and not l2 <= bar_l2:
            failures.append((f"{name}: rel-L2", l2, bar_l2))
        figures[name] = (err, l2)
    for name, rows in layout.zero_rows.items():
        worst = got[name].detach().cpu()[rows].float().abs().max().item()
        if not worst == 0.0:
            failures.append((f"{name}: rows that must be exact zeros", worst))
    if failures:
        raise Missed(failures, figures)
    return figures


# ---------------------------------------------------------------------------------------------------------------
# a torch stand-in for the kernels (fp32 mathematics, bf16 results), right or wrong in one chosen way
# ---------------------------------------------------------------------------------------------------------------
class StandIn:
    """run(inputs, dout) like the kernels' drivers in tests/test_gpu_attention_reference.py: an explicit forward and an
    explicit backward that each take their own keep mask (query-major pair matrix, as the layouts index it).
      scale               logit scale (right: 1 / 8)
      bwd_keep            the backward's mask when it is not the forward's
      dk_ignores_q_limit  rows past q_limit still contribute to dk
      drop_last_block     the key block behind the last full 64 is never visited"""

    def __init__(self, layout, keep=None, p=0.0, scale=0.125, bwd_keep=None, dk_ignores_q_limit=False, drop_last_block=False):
        self.layout, self.keep, self.p, self.scale = layout, keep, p, scale
        self.bwd_keep = keep if bwd_keep is None else bwd_keep
        self.dk_ignores_q_limit, self.drop_last_block = dk_ignores_q_limit, drop_last_block

    def _sequences(self):
        """(input slices of q rows, of kv rows, computed queries, dead keys) per sequence"""
        lay = self.layout
        if isinstance(lay, Packed):
            for s, n in enumerate(lay.lens):
                if n:
                    r = slice(lay.cu[s], lay.cu[s] + n)
                    yield r, r, int(lay.out_rows[r].sum()), torch.zeros(n, dtype=torch.bool)
        else:
            for b in range(lay.B):
                dead = lay.mask[b] if lay.mask is not None else torch.zeros(lay.n_k, dtype=torch.bool)
                yield (b, slice(None)), (b, slice(None)), lay.n_q, dead

    def _qkv(self, inputs):
        if isinstance(self.layout, Cross):
            return inputs[0].float(), inputs[1][..., :D].float(), inputs[1][..., D:].float()
        x = inputs[0].float()
        return x[..., :D], x[..., D:2 * D], x[..., 2 * D:3 * D]

    def _probs(self, q, k, dead):
        n_k = k.shape[0]
        s = (q.view(-1, H, HD).transpose(0, 1) @ k.view(-1, H, HD).permute(1, 2, 0)) * self.scale     # (H, nq, nk)
        dead = dead.clone()
        if self.drop_last_block and n_k % HD:
            dead[n_k - n_k % HD:] = True
        return torch.softmax(s.masked_fill(dead[None, None, :], float("-inf")), dim=-1)

    def _keep_of(self, keep, rq, n_q, n_k):
        if keep is None:
            return 1.0
        return keep[rq][:n_q, :, :n_k].permute(1, 0, 2).float() / (1.0 - self.p)                       # (H, nq, nk)

    def __call__(self, inputs, dout=None):
        q, k, v = self._qkv(inputs)
        out = torch.full(q.shape, 3.0)                          # rows that are not computed keep their garbage
        dq, dk, dv = torch.full(q.shape, 5.0), torch.full(k.shape, 5.0), torch.full(v.shape, 5.0)
        for rq, rk, nq, dead in self._sequences():
            qs, ks, vs = q[rq], k[rk], v[rk]
            n_q, n_k = qs.shape[0], ks.shape[0]
            P = self._probs(qs, ks, dead)
            vh = vs.view(n_k, H, HD).transpose(0, 1)
            o = ((P * self._keep_of(self.keep, rq, n_q, n_k)) @ vh).transpose(0, 1).reshape(n_q, D)
            out[rq] = torch.cat([o[:nq], out[rq][nq:]])
            if dout is None:
                continue
            do = dout[rq].float().clone()
            do[nq:] = 0
            doh = do.view(n_q, H, HD).transpose(0, 1)
            Kb = self._keep_of(self.bwd_keep, rq, n_q, n_k)
            dv[rk] = ((P * Kb).transpose(1, 2) @ doh).transpose(0, 1).reshape(n_k, D)
            dPd = (doh @ vh.transpose(1, 2)) * Kb
            dS = P * (dPd - (dPd * P).sum(-1, keepdim=True))
            dq[rq] = (dS @ ks.view(n_k, H, HD).transpose(0, 1)).transpose(0, 1).reshape(n_q, D) * self.scale
            if self.dk_ignores_q_limit:
                raw = (dout[rq].float().view(n_q, H, HD).transpose(0, 1) @ vh.transpose(1, 2)) * Kb
                dS = P * (raw - (raw * P).sum(-1, keepdim=True))
            dk[rk] = (dS.transpose(1, 2) @ qs.view(n_q, H, HD).transpose(0, 1)).transpose(0, 1).reshape(n_k, D) * self.scale
        out = out.to(torch.bfloat16)
        if dout is None:
            return out, None
        dq, dk, dv = (g.to(torch.bfloat16) for g in (dq, dk, dv))
        if isinstance(self.layout, Cross):
            return out, [dq, torch.cat([dk, dv], dim=-1)]
        return out, [torch.cat([dq, dk, dv], dim=-1)]


def examine(layout, run, inputs, dout, p, P=None):
    """The checks of one kernel on one case, in the order tests/test_gpu_attention_reference.py runs them for one mode:
    forward read-out (entries, keep rate), the backward's mask against the forward's, then out / dq / dk / dv with the
    real V against the fp64 reference that applies the read-out mask.  -> (mask, figures)"""
    if P is None:
        P = reference(layout, inputs, dout)["P"]
    mask, rel, rate = check_readout(read_forward(layout, run, inputs), P, layout.live, p)
    if p > 0.0:
        back = read_backward(layout, run, inputs)
        same_mask((back != 0) & layout.live.to(back.device), mask, "the backward drew another mask than the forward")
    ref = reference(layout, inputs, dout, mask if p > 0.0 else None, p)
    out, grads = run(inputs, dout)
    got = {"out": out}
    got.update(layout.split(grads))
    figures = accept(layout, got, ref)
    figures["read-out"], figures["keep rate"] = rel, rate
    return mask, figures
