"""References and error bounds for the op tests of the non-GEMM chain kernels (csrc/elementwise.hip): LayerNorm, the
embeddings, mean-pool, L2-norm, the vocabulary log-softmax and ASL losses, Adam, axpy, colsum and the BatchNorm
backward coefficients.

Every reference below is a plain restatement of the operation that computes in the dtype of its `dt` argument:
torch.float64 gives the reference, torch.float32 the "plain fp32 torch restatement on the CPU" whose own error e_cpu
sizes a tolerance.  tests/test_chain_refs_cpu.py checks the float64 forms against torch.autograd without a GPU.

One tolerance policy:

1. Integer outputs (pred, the counts of out3, nbt) and documented invariances (zeroed pad columns, untouched
   buffers, zero_grad, bit-equality across launch shapes, a single correctly rounded fp32 add) are exact: torch.equal,
   or `same_bits` where NaN sentinels take part.
2. Where the roundings can be read off the kernel the bound is analytic and per element, through
   hip_helpers.assert_within / dot_ulps: colsum, axpy, dgamma / dbeta of LayerNorm and of the embeddings, mean-pool,
   bn_coef_bwd, Adam.  Each derivation stands in the docstring of its bound function.
3. Everything else: the kernel's error against float64 must be <= max(4 * e_cpu, 2^-22 * scale) (`bound_4x`), where
   e_cpu is the error of the fp32 restatement against the same float64 values and scale the largest reference
   magnitude, both taken per segment of differing magnitude (per row for LayerNorm / embedding / L2-norm outputs, per
   table row for the embedding gradients).  For the LayerNorm output the scale is the magnitude of the row's INPUT
   carried to the output, max|s| rstd max|gamma|, where that is larger: the floor is four roundings of the values
   that are rounded, and with a common offset those are the inputs (see test_layernorm_fwd).  4x is the factor of
   test_hip_bertattn.py, max(4 e_cpu, 2^-22) the form of test_hip_bertscore.py.  The log-softmax and ASL gradients
   are bounded per element relative to the probability (`grad_bound`).  No tolerance is ever taken from the kernel's own output.

`check` asserts a bound and returns the worst err / bound ratio, which every test prints."""
import math

import torch

from hip_helpers import U23, assert_within, dot_ulps

U24 = 2.0 ** -24
F32, F64 = torch.float32, torch.float64
SLACK = 1.0 + 2.0 ** -10      # second-order terms of the first-order analytic bounds


# ----------------------------------------------------------------------------- policy
def bound_4x(ref, cpu, seg=None, scale=None):
    """max(4 e_cpu, 2^-22 scale) per segment: seg = dims reduced over (None: the whole tensor is one segment).  scale is
    the largest reference magnitude of the segment unless the caller gives one (shaped like the reduced reference): the
    floor stands for four roundings of the values the operation handles, and where those are larger than its results
    (LayerNorm of rows with a common offset) the caller carries their magnitude to the output."""
    ref, cpu = ref.double(), cpu.double()
    e, s = (cpu - ref).abs(), ref.abs()
    if seg is None:
        e, s = e.max(), s.max()
    else:
        e, s = e.amax(seg, keepdim=True), s.amax(seg, keepdim=True)
    if scale is not None:
        s = torch.maximum(s, scale.double())
    return torch.maximum(4.0 * e, 2.0 ** -22 * s).expand_as(ref).clone()


def check(out, ref, bound, what):
    """assert_within, then the worst err / bound (0 / 0 counts as 0)"""
    assert_within(out, ref, bound, what)
    err = (out.double().cpu() - ref.double().cpu()).abs()
    b = bound.double().cpu()
    r = torch.where(err > 0, err / b.clamp_min(1e-300), torch.zeros_like(err))
    return float(r.max()) if r.numel() else 0.0


def same_bits(a, b):
    """bit-for-bit equality of two fp32 tensors, NaN sentinels included"""
    return torch.equal(a.cpu().contiguous().view(torch.int32), b.cpu().contiguous().view(torch.int32))


def spread(sums, slots, total=16):
    """per-channel (sum, sum2) pairs scattered over the first `slots` of `total` statistic replicas, as the producers'
    atomics leave them (float64, CPU)"""
    Cc = sums.shape[0]
    stat = torch.zeros(total, Cc, 2, dtype=F64)
    w = torch.rand(slots, Cc, 2, dtype=F64)
    w = w / w.sum(0, keepdim=True)
    stat[:slots] = w * sums[None].double()
    return stat


# ----------------------------------------------------------------------------- LayerNorm
def ln_fwd(x, res, g, b, eps, dt):
    """(sum, mean, rstd, y) of y = LN(x + res) with biased variance; res may be None"""
    s = x.to(dt) if res is None else x.to(dt) + res.to(dt)
    mean = s.mean(-1, keepdim=True)
    var = ((s - mean) ** 2).mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    y = (s - mean) * rstd * g.to(dt) + b.to(dt)
    return s, mean.squeeze(-1), rstd.squeeze(-1), y


def ln_bwd(dy, s, g, mean, rstd, dres, dt):
    """(dx, dgamma, dbeta) from the saved sum / mean / rstd; dx includes dres when given"""
    dy, s, g = dy.to(dt), s.to(dt), g.to(dt)
    xh = (s - mean.to(dt)[:, None]) * rstd.to(dt)[:, None]
    dg = dy * g
    dx = rstd.to(dt)[:, None] * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    if dres is not None:
        dx = dx + dres.to(dt)
    return dx, (dy * xh).sum(0), dy.sum(0)


def colacc_bound(terms_abs_sum, prior, n, extra=0):
    """accumulation of n terms onto a prior value in any association order (register chains, LDS atomics, global
    atomics): a binary tree over n + 1 leaves, so |err| <= gamma_(n+1) (|prior| + sum |term|) as in dot_ulps; `extra`
    counts, in units of 2^-23, the roundings that produced each term beyond the one product rounding dot_ulps already
    holds (dy * xhat with xhat = (x - mean) * rstd: two more roundings = 1 unit; + 1 for safety)"""
    return (dot_ulps(n + 1) + extra) * U23 * (prior.double().abs() + terms_abs_sum.double()) + 1e-30


# ----------------------------------------------------------------------------- embeddings
def embed_fwd(ids, seg, word, pos, typ, g, b, vis, nv, eps, dt):
    """(out [B*T, H], xhat, rstd): row (b, t) = vis[t][b] for t < nv, else LN((word[id] + type[seg]) + pos[t]);
    xhat / rstd are meaningful on the text rows only"""
    B, T = ids.shape
    e = (word.to(dt)[ids] + typ.to(dt)[seg]) + pos.to(dt)[:T][None]
    mean = e.mean(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((e - mean) ** 2).mean(-1, keepdim=True) + eps)
    xh = (e - mean) * rstd
    out = xh * g.to(dt) + b.to(dt)
    if nv:
        out[:, :nv] = vis.to(dt).transpose(0, 1)
    H = word.shape[1]
    return out.reshape(B * T, H), xh.reshape(B * T, H), rstd.reshape(B * T)


def embed_bwd(dout, ids, seg, xhat, rstd, g, nword, npos, ntype, nv, pad_idx, dt):
    """gradient increments (dword, dpos, dtype, dgamma, dbeta, dvis) of embed_fwd from the saved xhat / rstd"""
    B, T = ids.shape
    H = dout.shape[-1]
    d, xh, rs = dout.to(dt).view(B, T, H), xhat.to(dt).view(B, T, H), rstd.to(dt).view(B, T, 1)
    text = torch.zeros(B, T, dtype=torch.bool)
    text[:, nv:] = True
    dg = d * g.to(dt)
    de = rs * (dg - dg.mean(-1, keepdim=True) - xh * (dg * xh).mean(-1, keepdim=True))
    de = torch.where(text[..., None], de, torch.zeros_like(de))
    dt_rows = torch.where(text[..., None], d, torch.zeros_like(d))
    dword, dpos, dtyp = torch.zeros(nword, H, dtype=dt), torch.zeros(npos, H, dtype=dt), torch.zeros(ntype, H, dtype=dt)
    keep = (text & (ids != pad_idx))[..., None]
    dword.index_add_(0, ids.reshape(-1), torch.where(keep, de, torch.zeros_like(de)).reshape(-1, H))
    dtyp.index_add_(0, seg.reshape(-1), de.reshape(-1, H))
    dpos[:T] = de.sum(0)
    dgamma, dbeta = (dt_rows * xh).sum((0, 1)), dt_rows.sum((0, 1))
    dvis = d[:, :nv].transpose(0, 1).contiguous()
    return dword, dpos, dtyp, dgamma, dbeta, dvis


# ----------------------------------------------------------------------------- mean-pool, L2-norm
def meanpool_fwd(h, mask, dt):
    m = mask.to(dt)[..., None]
    return (h.to(dt) * m).sum(1) / m.sum(1).clamp_min(1e-9)


def meanpool_bwd(dout, mask, dt):
    m = mask.to(dt)[..., None]
    return dout.to(dt)[:, None, :] * m / m.sum(1, keepdim=True).clamp_min(1e-9)


def meanpool_fwd_bound(h, mask):
    """T products h * mask (exact: the mask is 0 or 1) summed in order, then one division: dot_ulps(T) covers the sum
    (and a product rounding that does not occur), + 1 unit of 2^-23 the division"""
    m = mask.double()[..., None]
    return (dot_ulps(h.shape[1]) + 1) * U23 * (h.double().abs() * m).sum(1) / m.sum(1).clamp_min(1e-9) + 1e-30


def meanpool_bwd_bound(ref_inc, prior):
    """dout * mask is exact, the division rounds once, the accumulation onto dh once more"""
    b = U24 * ref_inc.double().abs()
    if prior is not None:
        b = b + U24 * (prior.double().abs() + ref_inc.double().abs())
    return b * SLACK + 1e-30


def l2norm_fwd(x, dt):
    n = x.to(dt).norm(dim=1, keepdim=True).clamp_min(1e-12)
    return x.to(dt) / n, n.squeeze(1)


def l2norm_bwd(dy, y, nrm, dt):
    dy, y = dy.to(dt), y.to(dt)
    return (dy - y * (dy * y).sum(1, keepdim=True)) / nrm.to(dt)[:, None]


# ----------------------------------------------------------------------------- vocabulary log-softmax
def lsm_fast_ok(ptr, ld, V):
    """the launcher's own condition for the float4 kernels, restated: a test asserts with it which kernel it reaches"""
    return ptr % 16 == 0 and ld % 4 == 0 and ld >= ((V + 3) & ~3)


def lsm_ref(x, tgt, dt, lse=None):
    """(lse, row_loss, p, pred): log-sum-exp per row (or the one supplied), lse - x[target], exp(x - lse) and the
    FIRST index of the row maximum"""
    x = x.to(dt)
    if lse is None:
        lse = torch.logsumexp(x, -1)
    lse = lse.to(dt)
    loss = lse - x.gather(1, tgt[:, None]).squeeze(1)
    p = torch.exp(x - lse[:, None])
    m = x.max(-1, keepdim=True).values
    V = x.shape[1]
    pred = torch.where(x == m, torch.arange(V)[None].expand_as(x), torch.full_like(x, V, dtype=torch.long)).min(-1).values
    return lse, loss, p, pred


def lsm_grad(p, tgt, gs):
    d = p.clone()
    d[torch.arange(p.shape[0]), tgt] -= 1.0
    return d * gs


def grad_rel(d32, ref, p64, tgt, gs, tscale=None):
    """worst error of the fp32 restatement's gradient relative to gs * p64_i over the elements with p64_i > 0 (the
    target column is left out for the log-softmax gradient, whose own term there is the 2^-23 of grad_bound; with
    tscale -- ASL -- it is measured against gs * tscale like any other element)"""
    w = p64.double().clone()
    rows = torch.arange(p64.shape[0])
    if tscale is None:
        w[rows, tgt] = 0.0
    else:
        w[rows, tgt] = tscale.double()
    ok = w > 0
    if not bool(ok.any()):
        return 0.0
    return float(((d32.double() - ref.double()).abs()[ok] / (abs(gs) * w[ok])).max())


def grad_bound(p64, tgt, gs, r, tscale=None):
    """|d_i - ref_i| <= |gs| (w_i r + [i == target] 2^-23), w_i = p64_i.  2^-23 at the target: the subtraction p - 1 and
    the product with gs round once each, 2^-24 of a magnitude <= 1 both.  ASL (tscale given): the target's gradient is
    not p - 1 but a sum of O(1) terms (w + lp dw and p * sum G), so there w_t = tscale = max(p_t, |ref_t| / gs)."""
    w = p64.double().clone()
    rows = torch.arange(p64.shape[0])
    hot = torch.zeros_like(w)
    hot[rows, tgt] = 1.0
    if tscale is not None:
        w[rows, tgt] = tscale.double()
    return abs(gs) * (w * r + hot * U23)


# ----------------------------------------------------------------------------- ASL (single label)
def asl_rows(x, tgt, gpos, gneg, eps, dt):
    """(row_loss, dlogits of sum(row_loss), p): models/asl_singlelabel.py restated per row with its closed-form
    gradient dlogit_k = G_k - p_k sum_j G_j, G_j = dL / d lp_j"""
    x = x.to(dt)
    Cc = x.shape[1]
    lp = x - torch.logsumexp(x, -1, keepdim=True)
    p = torch.exp(lp)
    t = torch.zeros_like(x)
    t[torch.arange(x.shape[0]), tgt] = 1.0
    ts = t * (1.0 - eps) + eps / Cc
    base = torch.where(t > 0, 1.0 - p, p)
    gam = torch.where(t > 0, torch.full_like(x, gpos), torch.full_like(x, gneg))
    w = torch.where(gam == 0, torch.ones_like(x), torch.pow(base, gam))
    dbase = torch.where(t > 0, -p, p)
    dw = torch.where(gam == 0, torch.zeros_like(x), gam * torch.pow(base, gam - 1.0) * dbase)
    G = -ts * (w + lp * dw)
    return (-ts * w * lp).sum(-1), G - p * G.sum(-1, keepdim=True), p


# ----------------------------------------------------------------------------- Adam
def adam_ref(p, g, m, v, step, lr, b1, b2, eps, gscale, dt):
    """one torch.optim.Adam step (no weight decay, no amsgrad) on grad * gscale; returns new (p, m, v)"""
    p, m, v = p.to(dt), m.to(dt), v.to(dt)
    gg = g.to(dt) * gscale
    m = m + (gg - m) * (1.0 - b1)
    v = v * b2 + gg * gg * (1.0 - b2)
    denom = v.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    return p - (lr / (1.0 - b1 ** step)) * (m / denom), m, v


def adam_bounds(p, g, m, v, step, lr, b1, b2, eps, gscale):
    """per-element bounds (bp, bm, bv) of one step from fp32 state, u = 2^-24, counted on the kernel's `upd`:

    gg = g * gscale                                    1 rounding
    m' = fma(gg - m, omb1, m)                          the subtraction, the constant (float)(1 - b1), the fma: 3 more
        |dm| <= u (|m'| + omb1 (|gg| + 2 |gg - m|))                                         [4 roundings]
    v' = fma(gg * gg, omb2, v * b2)                    gg twice, the square, (float)omb2: 4 on gg^2 omb2;
                                                       (float)b2, the product: 2 on v b2; the fma: 1 on v'
        |dv| <= u (4 gg^2 omb2 + 2 v b2 + v') <= 5 u v'                                     [7 roundings]
    denom = sqrtf(v') / bc2_sqrt + eps                 dv / (2 v'), sqrtf, (float)sqrt(bc2), the division, the add: 4 u
                                                       and (float)eps: u eps <= u denom
        |d denom| / denom <= dv / (2 v') + 5 u  (<= 7.5 u)
    p' = fma(-step_size, m' / denom, p)                the division, (float)(lr / bc1): 2 u on q = m' / denom, the fma: u |p'|
        |dp| <= u |p'| + step_size (dm / denom + |q| (dv / (2 v') + 7 u))   (<= u |p'| + step_size (dm / denom + 9.5 u |q|))
    each times 1 + 2^-10 for the second-order terms"""
    u = U24
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    omb1, omb2 = 1.0 - b1, 1.0 - b2
    gg = g * gscale
    p1, m1, v1 = adam_ref(p, g, m, v, step, lr, b1, b2, eps, gscale, F64)
    bm = u * (m1.abs() + omb1 * (gg.abs() + 2.0 * (gg - m).abs()))
    bv = u * (4.0 * gg * gg * omb2 + 2.0 * v * b2 + v1)
    denom = v1.sqrt() / math.sqrt(1.0 - b2 ** step) + eps
    q = (m1 / denom).abs()
    rel_v = torch.where(v1 > 0, bv / (2.0 * v1.clamp_min(1e-300)), torch.zeros_like(v1))
    bp = u * p1.abs() + (lr / (1.0 - b1 ** step)) * (bm / denom + q * (rel_v + 7.0 * u))
    return bp * SLACK + 1e-30, bm * SLACK + 1e-30, bv * SLACK + 1e-30


# ----------------------------------------------------------------------------- colsum, axpy
def colsum_bound(x, prior, rows):
    """out[c] = prior + sum_r x[r][c]: a sequential chain of <= 64 rows per block, then one float atomic per block onto
    out.  The chains and the atomics form a binary tree over the rows: dot_ulps(rows) 2^-23 sum_r |x|.  The prior value
    passes through one add per 64-row block (nb of them, not one: the blocks' atomics arrive one after another), each
    rounding 2^-24 of a partial sum <= |prior| + sum |x|."""
    nb = (rows + 63) // 64
    sa = x.double().abs().sum(0)
    return (dot_ulps(rows) * U23 * sa + nb * U24 * (prior.double().abs() + sa)) * SLACK + 1e-30


def axpy_bound(y0, x, a):
    """y + a * x: at most two roundings (the product, unless contracted into an fma, and the sum)"""
    ax = (float(a) * x.double()).abs()
    return U24 * (ax + (y0.double().abs() + ax)) * SLACK + 1e-30


# ----------------------------------------------------------------------------- BatchNorm backward coefficients
def bn_pqr(sg, sgx, count, gamma, mean, invstd, training):
    """P, Q, R of dz = P g + Q z + R in float64 from (sum g, sum g xhat); eval mode is the fixed affine map"""
    gamma, mean, invstd = gamma.double(), mean.double(), invstd.double()
    p = gamma * invstd
    if not training:
        return p, torch.zeros_like(p), torch.zeros_like(p)
    c1, c2 = sg.double() / count, sgx.double() / count
    return p, -p * c2 * invstd, p * (c2 * invstd * mean - c1)


def bn_pqr_bounds(sg, sgx, count, gamma, mean, invstd, training):
    """the kernel computes in double and rounds once to float: 2^-23 relative per coefficient (2^-24 would do; 2^-23
    leaves the headroom of one more rounding).  R = p (c2 invstd mean - c1) cancels, so the double arithmetic itself -- six operations
    and the four-level fold of the 16 replicas, each 2^-53 -- leaves up to 16 * 2^-53 = 2^-49 of |p c2 invstd mean| +
    |p c1|; the floor takes 2^-48 of it.  The same floor (of |Q|) covers Q."""
    P, Q, R = bn_pqr(sg, sgx, count, gamma, mean, invstd, training)
    if not training:
        return U23 * P.abs(), torch.zeros_like(P), torch.zeros_like(P)
    p = P.abs()
    c1, c2 = (sg.double() / count).abs(), (sgx.double() / count).abs()
    floor = 2.0 ** -48 * (p * c2 * invstd.double() * mean.double().abs() + p * c1)
    return U23 * p, U23 * Q.abs() + 2.0 ** -48 * Q.abs(), U23 * R.abs() + floor


def bn_acc_bound(s, prior):
    """dgamma[c] += (float)sum: the conversion and the add round once each"""
    s = s.double().abs()
    return U24 * (s + (prior.double().abs() + s)) * SLACK + 1e-30
