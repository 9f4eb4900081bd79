"""Shared pieces of the BERTScore tests: the score restated in plain torch, pair by pair and without padding, written
independently of mmvqa_amd; the bound every comparison uses; the input generators.

The restatement is the library's greedy_cos_idf with idf off for one candidate and one reference (the library itself is
not installed here, so it is restated, not pinned): states to unit length, S = all cosines over ALL positions of both
texts, P / R = the mean over the word pieces 1..len-2 of the row / column maxima, F = 2PR / (P + R) with NaN -> 0, an
empty text (len == 2) scores P = R = F = 0, then F <- (F - b) / (1 - b)."""
import torch

FLOOR = 2.0 ** -22           # four roundings of a value near 1
EPS = 1e-12


def unit(x):
    return x / x.norm(dim=-1, keepdim=True).clamp_min(EPS)


def pair(c, r, baseline=0.0):
    """(P, R, F) of one candidate c [la, D] against one reference r [lb, D] (raw states, [CLS] first, [SEP] last), in
    the tensors' dtype"""
    la, lb = c.shape[0], r.shape[0]
    zero = c.new_zeros(())
    if la == 2 or lb == 2:
        P = R = F = zero
    else:
        S = unit(c) @ unit(r).T
        P = S.max(dim=1).values[1:la - 1].mean()
        R = S.max(dim=0).values[1:lb - 1].mean()
        F = 2 * P * R / (P + R)
        if torch.isnan(F):
            F = zero
    if baseline != 0.0:
        F = (F - baseline) / (1 - baseline)
    return P, R, F


def bertscore(xa, la, xb, lb, baseline=0.0, dtype=torch.float64):
    """(P, R, F), each [n, n] in `dtype`, of candidates xa [n, T, D] with lengths la against references xb / lb: every
    pair alone, cut to its lengths, so no padded position is ever touched; unit diagonal; a length outside [2, T]
    gives NaN in its row (la) or column (lb)"""
    n, T, _ = xa.shape
    xa, xb = xa.to(dtype), xb.to(dtype)
    out = torch.ones(3, n, n, dtype=dtype)
    for i in range(n):
        for j in range(n):
            if i == j:
                continue
            a, b = int(la[i]), int(lb[j])
            if not (2 <= a <= T and 2 <= b <= T):
                out[:, i, j] = float("nan")
                continue
            out[:, i, j] = torch.stack(pair(xa[i, :a], xb[j, :b], baseline))
    return out[0], out[1], out[2]


def cpu_error(xa, la, xb, lb, baseline=0.0):
    """(float64 (P, R, F), e_cpu): e_cpu = max |fp32 CPU restatement - float64| over P, R and F on these inputs"""
    ref = bertscore(xa, la, xb, lb, baseline, torch.float64)
    f32 = bertscore(xa, la, xb, lb, baseline, torch.float32)
    e = 0.0
    for a, b in zip(f32, ref):
        ok = ~torch.isnan(b)
        e = max(e, float((a.double() - b)[ok].abs().max()))
    return ref, e


def bound(e_cpu):
    """the bound of every comparison: it comes from the CPU's own fp32 error, never from the kernel's output"""
    return max(4.0 * e_cpu, FLOOR)


def offdiag(n):
    return ~torch.eye(n, dtype=torch.bool)


def positive_states(n, T, D, seed, common=1.5):
    """candidates and references [n, T, D] fp32 = common direction + unit-size noise, so that every cosine is near
    common^2 / (common^2 + 1) and F is well conditioned"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(D, generator=g)
    u = u / u.norm()
    mk = lambda: (common * u + torch.randn(n, T, D, generator=g) / D ** 0.5) * 3.0   # noqa: E731  (not unit length)
    return mk(), mk()


def zero_mean_states(n, T, D, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, T, D, generator=g), torch.randn(n, T, D, generator=g)


def lens_cycle(n, choices, shift=0):
    return torch.tensor([choices[(k + shift) % len(choices)] for k in range(n)], dtype=torch.int32)


def assert_conditioned(ref, la, lb):
    """inputs compared on F: in float64 every off-diagonal pair of non-empty texts has P + R >= 0.5"""
    P, R, _ = ref
    n = P.shape[0]
    full = offdiag(n) & (la[:, None] > 2) & (lb[None, :] > 2)
    assert float((P + R)[full].min()) >= 0.5, float((P + R)[full].min())


def poison(x, lens, value):
    """a copy of x [n, T, D] with every position >= len filled with `value`"""
    y = x.clone()
    for b, n in enumerate(lens.tolist()):
        y[b, max(n, 0):] = value
    return y
