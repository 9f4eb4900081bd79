"""References, layouts and error bounds for the op tests of csrc/attention.hip (tests/test_hip_attention.py).

`attn_fwd` / `attn_bwd` are plain restatements of the operation that compute in the dtype of their `dt` argument:
torch.float64 gives the reference, torch.float32 the "plain fp32 torch restatement on the CPU" whose own error e_cpu
sizes the tolerance, as in chain_helpers.py.  tests/test_attention_refs_cpu.py checks the float64 forms against
torch.autograd without a GPU, and an fp32 emulation of the kernel's association order against the bound below.

Operands are [B, heads, T, D]; the score-shaped tensors of the kernel's interface keep its layouts: prev / dprev are
[B, query, key, heads].  Probabilities are returned query-major [B, heads, query, key]; the kernel saves them key-major,
so a test transposes what it reads back.

Tolerance: policy 3 of chain_helpers.py, max(4 e_cpu, 2^-22 scale), per SEGMENT = (sample, head, row class), where the
row class splits the rows of a head into those the mask keeps and those it drops (`seg_bound`).  The split is needed:
the -10000 of a masked row rounds its scores to a grid of 2^-10, and the error of that would otherwise set the bound
for the real rows of the same head.  Where an honest fp32 kernel does not stay inside that bound -- segments of a few
rows, whose e_cpu is the maximum of too few draws -- the output has an analytic per-element bound instead, derived in
the docstring of its function: prev_out on unmasked rows (`prev_bound`), the probabilities (`probs_bound`), out
(`out_bound`), dQ and dK (`dqk_bound`).  prev_out on masked rows, dV and dprev_out keep the segment bound."""
import ctypes as C

import numpy as np
import torch

from dropout_helpers import keep_tensor
from hip_helpers import U23, dot_ulps
from mmvqa_amd import _lib as L

F32, F64 = torch.float32, torch.float64
U24 = 2.0 ** -24
SLACK = 1.0 + 2.0 ** -10
TAIL = 32          # sentinel rows behind every allocation
NAN = float("nan")
MASK_POISON = 7    # tail of the mask allocation: a key read from there would get +60000 on its score


def f32(x):
    """a number as the float the kernel receives"""
    return float(np.float32(x))


# ----------------------------------------------------------------------------- references
def _keep_scale(B, heads, T, drop_p, seed, dt):
    """keep mask times 1 / (1 - p) over [B, heads, query, key]: index ((b heads + head) T + query) T + key"""
    return keep_tensor(seed, (B, heads, T, T), drop_p).to(dt) * (1.0 / (1.0 - f32(drop_p)))


def attn_fwd(q, k, v, mask, mask_on_query, prev_in, sqrt_d, drop_p, seed, dt):
    """(prev_out [B, T, T, heads], probs [B, heads, query, key] before dropout, out [B, heads, T, D]) in the op order of
    the kernel header: (q . k) / sqrt_d, then + prev, then - 10000 (1 - m); prev_out is that score; softmax over the
    keys; the dropout keep mask; . V"""
    q, k, v = q.to(dt), k.to(dt), v.to(dt)
    B, heads, T, _ = q.shape
    s = q @ k.transpose(-1, -2) / sqrt_d
    if prev_in is not None:
        s = s + prev_in.to(dt).permute(0, 3, 1, 2)
    m = mask.to(dt)
    m = m[:, None, :, None] if mask_on_query else m[:, None, None, :]
    s = s - 10000.0 * (1.0 - m)
    e = torch.exp(s - s.amax(-1, keepdim=True))
    probs = e / e.sum(-1, keepdim=True)
    pd = probs * _keep_scale(B, heads, T, drop_p, seed, dt) if drop_p > 0 else probs
    return s.permute(0, 2, 3, 1).contiguous(), probs, pd @ v


def attn_bwd(q, k, v, dout, probs, dprev_in, mask, mask_on_query, sqrt_d, drop_p, seed, dt):
    """(dq, dk, dv, dprev_out) written out, as a function of the saved probabilities `probs` [B, heads, query, key]:
    dP' = dO V^T, the dropout mask on dP, delta = sum_j dP P, dS = P (dP - delta) + dprev_in, dprev_out = dS,
    dQ = dS K / sqrt_d, dK = dS^T Q / sqrt_d, dV = P'^T dO.  The additive mask has no gradient: mask / mask_on_query are
    taken so that the call mirrors attn_fwd, and do not enter."""
    q, k, v, dout, probs = q.to(dt), k.to(dt), v.to(dt), dout.to(dt), probs.to(dt)
    B, heads, T, _ = q.shape
    dp = dout @ v.transpose(-1, -2)
    pd = probs
    if drop_p > 0:
        ks = _keep_scale(B, heads, T, drop_p, seed, dt)
        dp, pd = dp * ks, probs * ks
    delta = (dp * probs).sum(-1, keepdim=True)
    ds = probs * (dp - delta)
    if dprev_in is not None:
        ds = ds + dprev_in.to(dt).permute(0, 3, 1, 2)
    return (ds @ k) / sqrt_d, (ds.transpose(-1, -2) @ q) / sqrt_d, pd.transpose(-1, -2) @ dout, ds.permute(0, 2, 3, 1).contiguous()


# ----------------------------------------------------------------------------- bounds
def seg_bound(ref, cpu, rows_valid):
    """max(4 e_cpu, 2^-22 scale) per segment (sample, head, row class) of a [B, heads, rows, X] tensor: rows_valid
    [B, rows] (bool) splits the rows of each (sample, head) into two classes, and e_cpu = max |cpu - ref| and scale =
    max |ref| are taken over each class on its own.  A class without rows bounds nothing."""
    ref, cpu = ref.double(), cpu.double()
    e, s = (cpu - ref).abs(), ref.abs()
    sel = rows_valid[:, None, :, None].expand_as(ref)
    bound, zero = torch.zeros_like(ref), torch.zeros_like(ref)
    for c in (sel, ~sel):
        ec = torch.where(c, e, zero).amax((2, 3), keepdim=True)
        sc = torch.where(c, s, zero).amax((2, 3), keepdim=True)
        bound = torch.where(c, torch.maximum(4.0 * ec, 2.0 ** -22 * sc).expand_as(ref), bound)
    return bound


def prev_bound(q, k, prev_in, sqrt_d):
    """prev_out on rows the mask keeps, [B, query, key, heads]: s = fl(fl(dot / sqrt_d) + prev) - 10000 * 0.  The D-term
    dot product is within dot_ulps(D) 2^-23 sum |q_d k_d| in any association order (hip_helpers.dot_ulps), and stays so
    relative to the quotient; the division rounds 2^-24 |dot / sqrt_d|, the addition 2^-24 |s|; the mask term is an exact
    zero.  Times 1 + 2^-10 for the second-order terms."""
    q, k = q.double(), k.double()
    mag = q.abs() @ k.abs().transpose(-1, -2) / sqrt_d
    s0 = q @ k.transpose(-1, -2) / sqrt_d
    s = s0 if prev_in is None else s0 + prev_in.double().permute(0, 3, 1, 2)
    b = (dot_ulps(q.shape[-1]) * U23 * mag + U24 * (s0.abs() + s.abs())) * SLACK + 1e-30
    return b.permute(0, 2, 3, 1).contiguous()


def score_major(x):
    """[B, query, key, heads] -> [B, heads, query, key]"""
    return x.permute(0, 3, 1, 2)


def prev_out_bound(q, k, prev_in, sqrt_d, ref, cpu, rows_valid):
    """prev_out [B, query, key, heads]: prev_bound on the query rows the mask keeps, seg_bound on the masked ones (their
    -10000 makes them a segment of their own magnitude)"""
    seg = seg_bound(score_major(ref), score_major(cpu), rows_valid).permute(0, 2, 3, 1)
    return torch.where(rows_valid[:, :, None, None], prev_bound(q, k, prev_in, sqrt_d), seg)


def probs_bound(q, k, prev_in, mask, mask_on_query, sqrt_d):
    """Analytic, per element, for the saved probabilities [B, heads, query, key].  The segment bound does not hold for
    them on the MI355X: a class of few rows (the 16 masked query rows of a sample at T = 75, a sample of 9 tokens) makes
    e_cpu the maximum of a few hundred draws, and single elements of the honest kernel reached 1.04 .. 1.16 of it
    (BERT form D = 64 T = 75; RealFormer form D = 96 T = 9: errors of 5 to 6 ulp of the probability, where the 64- or
    96-term score alone is allowed 33 or 49).  With u = 2^-24, first order, sums in any association order
    (hip_helpers.dot_ulps):

    s = ((q . k) / sqrt_d + prev) - 10000 (1 - m)
        E_s = dot_ulps(D) 2u |q| . |k| / sqrt_d + u (|s0| + |s1|) + u |s| [key mask, m = 0]
                           (division, + prev, - 10000: exact where m = 1, and not part of the softmax at all under a
                           QUERY mask, where the kernel's softmax takes the unshifted row: see attention.hip)
    ex = expf(s - mx)      the kernel's own row maximum mx is a shift, not an error; the subtraction rounds u |s - mx|,
                           expf is within 1 ulp (HIP's device library): rel_ij = E_s + u |s - mx| + 2u
    sum = sum_j ex         relative: sum_j p_j rel_j + dot_ulps(T) 2u
    p = ex * (1 / sum)     two roundings, 2u in all
        |dp_ij| <= p_ij (rel_ij + sum_l p_il rel_il + (dot_ulps(T) + 1) 2u)
    times 1 + 2^-10 for the second-order terms (the largest first-order term is u 10000 = 6e-4 at a masked key)."""
    q, k = q.double(), k.double()
    T, D = q.shape[-2:]
    s0 = q @ k.transpose(-1, -2) / sqrt_d
    s1 = s0 if prev_in is None else s0 + prev_in.double().permute(0, 3, 1, 2)
    m = mask.double()
    m = m[:, None, :, None] if mask_on_query else m[:, None, None, :]
    s = s1 - 10000.0 * (1.0 - m)
    e_s = dot_ulps(D) * U23 * (q.abs() @ k.abs().transpose(-1, -2)) / sqrt_d + U24 * (s0.abs() + s1.abs())
    if not mask_on_query:
        e_s = e_s + U24 * s.abs() * (1.0 - m)
    mx = s.amax(-1, keepdim=True)
    rel = e_s + U24 * (s - mx).abs() + U23
    p = torch.softmax(s, -1)
    return p * (rel + (p * rel).sum(-1, keepdim=True) + (dot_ulps(T) + 1) * U23) * SLACK + 1e-30


def out_bound(v, e_probs, probs, drop_p, seed):
    """Analytic, per element, for out = P' V from the float64 probabilities `probs` and their bound `e_probs`
    (probs_bound).  The segment bound holds for it on the MI355X, but without any margin: the honest kernel reached 1.00
    of it (RealFormer form D = 96 T = 9, segments of 3 to 6 rows), and e_cpu belongs to the CPU at hand.  With u = 2^-24,
    first order: P' = K P with K the keep mask times ks rounds twice under dropout, E_P' = K E_P + 2u P' (p = 0: E_P);
    the T-term sum in any association order (hip_helpers.dot_ulps):
        E_out = E_P' |V| + dot_ulps(T) 2u P' |V|
    times 1 + 2^-10 for the second-order terms."""
    v, P, e = v.double(), probs.double(), e_probs.double()
    B, heads, T, _ = v.shape
    if drop_p > 0:
        ks = _keep_scale(B, heads, T, drop_p, seed, F64)
        P, e = P * ks, e * ks
        e = e + 2.0 * U24 * P
    return (e @ v.abs() + dot_ulps(T) * U23 * (P @ v.abs())) * SLACK + 1e-30


def dqk_bound(q, k, v, dout, probs, dprev_in, sqrt_d, drop_p, seed):
    """Analytic, per element, for (dQ, dK) as functions of the saved probabilities P (the isolated backward check).  The
    segment bound does not hold for them: the masked class of a sample cut one row short of T is a single row of D
    values, the "single row" that is too noisy for e_cpu.  The CPU emulation of an honest fp32 kernel reaches 1.04 of it
    in dK there (RealFormer form, D = 12, T = 33), and on the MI355X one element of dQ reached 1.13 (BERT form D = 64
    T = 9, the 6 masked rows of a sample).  With u = 2^-24, first order, every sum in any association order
    (hip_helpers.dot_ulps), K the keep mask times ks:

    dP0 = dO V^T                    E_dP0 = dot_ulps(D) 2u |dO| |V|^T
    dP  = K dP0                     E_dP  = K E_dP0 + 2u |dP|               (ks is rounded, so is the product; p = 0: E_dP0)
    delta_i = sum_j dP_ij P_ij      E_dl  = sum_j E_dP_ij P_ij + dot_ulps(T) 2u sum_j |dP_ij| P_ij
    dS = P dP - P delta (+ dprev)   E_dS  = P (E_dP + E_dl) + u (P |dP| + P |delta| + |P (dP - delta)|) + u |dS|
                                    (pass A's form; pass B's P (dP - delta) rounds twice on P |dP - delta|, which is less)
    g = dS / sqrt_d                 E_g   = E_dS / sqrt_d + u |g|
    dQ = g K                        E_dQ  = E_g |K| + dot_ulps(T) 2u |g| |K|
    dK = g^T Q                      E_dK  = E_g^T |Q| + dot_ulps(T) 2u |g|^T |Q|
    times 1 + 2^-10 for the second-order terms."""
    q, k, v, dout, P = q.double(), k.double(), v.double(), dout.double(), probs.double()
    B, heads, T, D = q.shape
    cD, cT = dot_ulps(D) * U23, dot_ulps(T) * U23
    dp = dout @ v.transpose(-1, -2)
    e_dp = cD * (dout.abs() @ v.abs().transpose(-1, -2))
    if drop_p > 0:
        ks = _keep_scale(B, heads, T, drop_p, seed, F64)
        dp, e_dp = dp * ks, e_dp * ks
        e_dp = e_dp + 2.0 * U24 * dp.abs()
    delta = (dp * P).sum(-1, keepdim=True)
    e_dl = (e_dp * P).sum(-1, keepdim=True) + cT * (dp.abs() * P).sum(-1, keepdim=True)
    ds = P * (dp - delta)
    e_ds = P * (e_dp + e_dl) + U24 * (P * dp.abs() + P * delta.abs() + ds.abs())
    if dprev_in is not None:
        ds = ds + dprev_in.double().permute(0, 3, 1, 2)
        e_ds = e_ds + U24 * ds.abs()
    g = ds / sqrt_d
    e_g = e_ds / sqrt_d + U24 * g.abs()
    return ((e_g @ k.abs() + cT * (g.abs() @ k.abs())) * SLACK + 1e-30,
            (e_g.transpose(-1, -2) @ q.abs() + cT * (g.abs().transpose(-1, -2) @ q.abs())) * SLACK + 1e-30)


def fwd_bounds(c, ref, cpu, drop_p=0.0, seed=0):
    """bounds of (prev_out, probs, out) for the float64 / fp32 results `ref` / `cpu` of attn_fwd on case c"""
    valid = c["mask"].bool()
    bp = probs_bound(c["q"], c["k"], c["prev_in"], c["mask"], c["mask_on_query"], c["sqrt_d"])
    return (prev_out_bound(c["q"], c["k"], c["prev_in"], c["sqrt_d"], ref[0], cpu[0], valid), bp,
            out_bound(c["v"], bp, ref[1], drop_p, seed))


def bwd_bounds(c, probs, ref, cpu, drop_p, seed):
    """bounds of (dq, dk, dv, dprev_out) for the float64 / fp32 results of attn_bwd on case c and the saved `probs`:
    dq and dk analytic (dqk_bound); segments by key row for dv, by query row for dprev_out"""
    valid = c["mask"].bool()
    bq, bk = dqk_bound(c["q"], c["k"], c["v"], c["dout"], probs, c["dprev_in"], c["sqrt_d"], drop_p, seed)
    return (bq, bk, seg_bound(ref[2], cpu[2], valid),
            seg_bound(score_major(ref[3]), score_major(cpu[3]), valid).permute(0, 2, 3, 1))


def fwd_args(c, drop_p=0.0, seed=0):
    return (c["q"], c["k"], c["v"], c["mask"], c["mask_on_query"], c["prev_in"], c["sqrt_d"], drop_p, seed)


def bwd_args(c, probs, drop_p=0.0, seed=0):
    return (c["q"], c["k"], c["v"], c["dout"], probs, c["dprev_in"], c["mask"], c["mask_on_query"], c["sqrt_d"], drop_p, seed)


# ----------------------------------------------------------------------------- layouts and descriptors
class Layout:
    """The two operand layouts engine.cpp hands to the attention kernels, with an optional gap of `pad` floats (a
    multiple of 4) behind every row of the q|k|v buffer and of the output buffer.

    bert: fused [B T][3 H], blocks q | k | v, head stride D          (bert_attn_desc)
    rf:   [B T][heads 3 es], k | q | v per head, head stride 3 es    (rf_attn_desc; the engine has heads = 8)
    Output / dout: [B T][heads D], head stride D, in both.  The gradients dq / dk / dv mirror q / k / v."""

    def __init__(self, form, heads, D, pad=0):
        assert form in ("bert", "rf") and pad % 4 == 0
        self.form, self.heads, self.D, self.pad = form, heads, D, pad
        if form == "bert":
            H = heads * D
            self.row, self.head, self.off = 3 * H + pad, D, dict(q=0, k=H, v=2 * H)
        else:
            self.row, self.head, self.off = heads * 3 * D + pad, 3 * D, dict(k=0, q=D, v=2 * D)
        self.out_row, self.out_head = heads * D + pad, D

    def _cols(self, which):
        base, hs = (0, self.out_head) if which == "out" else (self.off[which], self.head)
        return (base + torch.arange(self.heads)[:, None] * hs + torch.arange(self.D)[None]).reshape(-1)

    def _width(self, which):
        return self.out_row if which == "out" else self.row

    def blank(self, which, B, T):
        """an all-NaN allocation of B T + TAIL rows for operand kind `which` ('out' or any of 'q', 'k', 'v')"""
        return torch.full((B * T + TAIL, self._width(which)), NAN)

    def pack(self, B, T, **parts):
        """[B, heads, T, D] operands into one allocation; gap columns and tail rows hold NaN"""
        buf = self.blank(next(iter(parts)), B, T)
        for which, x in parts.items():
            buf[:B * T, self._cols(which)] = x.float().permute(0, 2, 1, 3).reshape(B * T, self.heads * self.D)
        return buf

    def unpack(self, buf, which, B, T):
        return buf.cpu()[:B * T][:, self._cols(which)].view(B, T, self.heads, self.D).permute(0, 2, 1, 3).contiguous()

    def owned(self, B, T, *which):
        """bool map of the allocation's elements that belong to the operands `which`"""
        m = torch.zeros(B * T + TAIL, self._width(which[0]), dtype=torch.bool)
        for w in which:
            m[:B * T, self._cols(w)] = True
        return m


def tail_rows(x, fill=NAN):
    """x with TAIL sentinel rows (of x's trailing shape) appended along dim 0"""
    return torch.cat([x, torch.full((TAIL,) + tuple(x.shape[1:]), fill, dtype=x.dtype)], 0)


def _attn_desc(lay, qkv, out, mask, probs, B, T, sqrt_d, prev_in, prev_out, drop_p, seed):
    a = L.AttnDesc()
    a.q, a.k, a.v = (qkv.data_ptr() + 4 * lay.off[w] for w in "qkv")
    a.row_stride, a.head_stride = lay.row, lay.head
    a.out, a.out_row_stride, a.out_head_stride = out.data_ptr(), lay.out_row, lay.out_head
    a.mask, a.mask_on_query, a.probs = mask.data_ptr(), int(lay.form == "rf"), probs.data_ptr()
    a.prev_in = None if prev_in is None else prev_in.data_ptr()
    a.prev_out = None if prev_out is None else prev_out.data_ptr()
    a.B, a.T, a.heads, a.sqrt_d, a.drop_p, a.seed = B, T, lay.heads, sqrt_d, drop_p, seed
    return a


def bert_attn_desc(lay, qkv, out, mask, probs, B, T, sqrt_d, drop_p=0.0, seed=0):
    """engine.cpp bert_attn_desc: key-axis mask, no score chain"""
    assert lay.form == "bert"
    return _attn_desc(lay, qkv, out, mask, probs, B, T, sqrt_d, None, None, drop_p, seed)


def rf_attn_desc(lay, kqv, out, mask, probs, B, T, sqrt_d, prev_in, prev_out, drop_p=0.0, seed=0):
    """engine.cpp rf_attn_desc: query-axis mask, prev_in (None in layer 0) / prev_out"""
    assert lay.form == "rf"
    return _attn_desc(lay, kqv, out, mask, probs, B, T, sqrt_d, prev_in, prev_out, drop_p, seed)


def set_bwd(a, lay, dout, dqkv, dprev_in=None, dprev_out=None):
    """the backward's fields: dout in the output layout, dq / dk / dv mirroring q / k / v"""
    a.dout = dout.data_ptr()
    a.dq, a.dk, a.dv = (dqkv.data_ptr() + 4 * lay.off[w] for w in "qkv")
    a.dprev_in = None if dprev_in is None else dprev_in.data_ptr()
    a.dprev_out = None if dprev_out is None else dprev_out.data_ptr()
    return a


def launch(a, D, bwd):
    L.check(L.lib().mmvqa_attention(C.byref(a), D, bwd, L.stream_ptr()))
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- the grid both test files walk
TS = (1, 9, 31, 32, 33, 64, 65, 75, 96, 97, 127, 128)
NJ_T = {1: 31, 2: 33, 3: 75, 4: 128}     # one T per key-tile count, for the cross pairings


def nj_of(T):
    return (T + 31) // 32


def ragged_lens(T):
    """valid lengths of three samples: all of T; a cut inside the last 32-row tile (on its first row where the tile has
    a single row); a cut in an earlier tile (for one tile: a shorter cut in it)"""
    t0 = 32 * (nj_of(T) - 1)
    return (T, max(1, T - max(1, (T - t0) // 2)), t0 - 5 if t0 else max(1, T // 3))


def make_case(form, D, T, lens, prev=True, dprev=True, heads=2, seed=0):
    """random operands of one case, on the CPU in fp32: dict with q k v dout [B, heads, T, D], mask [B, T] (long),
    prev_in / dprev_in [B, T, T, heads] or None (never for the BERT form), sqrt_d"""
    g = torch.Generator().manual_seed(100003 * D + 101 * T + seed)
    B = len(lens)
    c = {n: torch.randn(B, heads, T, D, generator=g) for n in ("q", "k", "v", "dout")}
    rf = form == "rf"
    c["prev_in"] = torch.randn(B, T, T, heads, generator=g) * 0.5 if rf and prev else None
    c["dprev_in"] = torch.randn(B, T, T, heads, generator=g) * 0.1 if rf and dprev else None
    mask = torch.zeros(B, T, dtype=torch.long)
    for b, n in enumerate(lens):
        mask[b, :n] = 1
    c["mask"], c["sqrt_d"], c["mask_on_query"] = mask, f32(D ** 0.5), int(rf)
    return c


def grid_cases():
    """(form, D, T, prev, dprev) of the instance grid: engine pairings at every T, cross pairings and the RealFormer
    form without prev_in / dprev_in at one T per tile count"""
    cases = [(f, D, T, True, True) for f, Ds in (("bert", (8, 64)), ("rf", (12, 96))) for D in Ds for T in TS]
    cases += [(f, D, T, True, True) for f, D in (("bert", 96), ("rf", 64)) for T in NJ_T.values()]
    cases += [("rf", D, T, False, False) for D in (12, 96) for T in NJ_T.values()]
    return cases
