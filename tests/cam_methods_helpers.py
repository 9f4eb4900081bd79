"""Oracle-side helpers of the attribution-method tests (vqamed2019/grad_cam.py:65-72): every
formula restated twice in fp64 (tensor form and plain loops), Eigen-CAM through the symmetric eigenproblem of the Gram
matrix, the ablated visual tokens as "zero the channel, 1x1 convolution, activation, mean", and the oracle runs that zero
one channel of the deepest feature map through a forward hook.

The definitions are restated from the papers (Grad-CAM++: Chattopadhay et al. 2018; XGrad-CAM: Fu et al. 2020; Eigen-CAM:
Muhammad & Yeasin 2020; Ablation-CAM: Desai & Ramaswamy 2020), not pinned against pytorch_grad_cam."""
import copy

import numpy as np
import torch

import gradcam_helpers as GH

EPS = 1e-7


# ------------------------------------------------------------------------------------------------ channel weights
def weights_gradcampp(A, dA):
    """A, dA [B, H, W, C] -> w [B, C] fp64: sum_p relu(g) * g^2 / (2 g^2 + S_c g^3 + 1e-7), 0 where g == 0"""
    a, g = A.double().flatten(1, 2), dA.double().flatten(1, 2)
    S = a.sum(1, keepdim=True)
    g2 = g * g
    alpha = torch.where(g != 0, g2 / (2 * g2 + S * g2 * g + EPS), torch.zeros_like(g))
    return (g.clamp_min(0) * alpha).sum(1)


def weights_xgradcam(A, dA):
    """-> w [B, C] fp64: sum_p g * a / (S_c + 1e-7)"""
    a, g = A.double().flatten(1, 2), dA.double().flatten(1, 2)
    return (g * a).sum(1) / (a.sum(1) + EPS)


def weights_loops(A, dA, method):
    """the same arithmetic written element by element"""
    a, g = A.double().numpy(), dA.double().numpy()
    B, H, W, C = a.shape
    out = np.zeros((B, C))
    for b in range(B):
        for c in range(C):
            S = sum(a[b, y, x, c] for y in range(H) for x in range(W))
            acc = 0.0
            for y in range(H):
                for x in range(W):
                    gv, av = g[b, y, x, c], a[b, y, x, c]
                    if method == "gradcam++":
                        if gv != 0:
                            acc += max(gv, 0.0) * gv ** 2 / (2 * gv ** 2 + S * gv ** 3 + EPS)
                    else:
                        acc += gv * av / (S + EPS)
            out[b, c] = acc
    return torch.from_numpy(out)


def pole_margins(A, dA):
    """how far the inputs stay from the formulas' own poles: (min_c |S_c| / sum_p |a_pc|,
    min over g != 0 of |2 g^2 + S_c g^3| / (2 g^2))"""
    a, g = A.double().flatten(1, 2), dA.double().flatten(1, 2)
    S = a.sum(1, keepdim=True)
    m1 = (S.abs() / a.abs().sum(1, keepdim=True)).min().item()
    g2 = g * g
    ratio = torch.where(g != 0, (2 * g2 + S * g2 * g).abs() / (2 * g2).clamp_min(1e-300), torch.full_like(g, 1e30))
    return m1, ratio.min().item()


# ------------------------------------------------------------------------------------------------ the shared tail
def raw_from_weights(A, w):
    """raw[b, p] = (1 / C) sum_c w[b, c] A[b, p, c], fp64 [B, H, W]"""
    return (A.double() * w.double()[:, None, None, :]).mean(dim=3)


def cam_from_raw(raw):
    """ReLU, division by the per-sample maximum; zeros and valid = 0 where the maximum is not positive"""
    pos = raw.double().clamp_min(0.0)
    m = pos.flatten(1).max(dim=1).values
    valid = m > 0
    cam = torch.where(valid[:, None, None], pos / m.clamp_min(1e-300)[:, None, None], torch.zeros_like(pos))
    return cam, valid


def cam_from_weights(A, w):
    return cam_from_raw(raw_from_weights(A, w))


def cam_from_weights_loops(A, w):
    a, w = A.double().numpy(), w.double().numpy()
    B, H, W, C = a.shape
    out = np.zeros((B, H, W))
    for b in range(B):
        for y in range(H):
            for x in range(W):
                out[b, y, x] = max(sum(w[b, c] * a[b, y, x, c] for c in range(C)) / C, 0.0)
        m = out[b].max()
        out[b] = out[b] / m if m > 0 else 0.0
    return torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------ Eigen-CAM
def fix_sign(raw):
    """the entry of largest magnitude becomes positive (ties: lowest index); raw: 1-D numpy"""
    j = int(np.argmax(np.abs(raw)))          # argmax returns the first of equal maxima
    return -raw if raw[j] < 0 else raw


def centred(A_b):
    """one sample [H, W, C] -> X [HW, C] fp64 with every column centred over the positions"""
    X = A_b.double().numpy().reshape(-1, A_b.shape[-1])
    return X - X.mean(axis=0, keepdims=True)


def eigencam_raw(A):
    """A [B, H, W, C] -> (raw [B, H, W] fp64 = X v1 = sigma1 u1 with the sign rule, gap [B] = sigma2^2 / sigma1^2), through
    the symmetric eigenproblem of G = X X^T; zeros (gap 1) where X is all zero or H * W = 1"""
    B, H, W, _ = A.shape
    raw, gap = np.zeros((B, H * W)), np.ones(B)
    for b in range(B):
        X = centred(A[b])
        lam, U = np.linalg.eigh(X @ X.T)
        if H * W == 1 or lam[-1] <= 0:
            continue
        raw[b] = fix_sign(np.sqrt(lam[-1]) * U[:, -1])
        gap[b] = max(lam[-2], 0.0) / lam[-1]
    return torch.from_numpy(raw).view(B, H, W), torch.from_numpy(gap)


def eigencam_raw_svd(A_b):
    """one sample through numpy.linalg.svd: X v1 with the sign rule, 1-D"""
    X = centred(A_b)
    _, _, Vt = np.linalg.svd(X, full_matrices=False)
    return fix_sign(X @ Vt[0])


def sign_margin(raw_b):
    """largest |raw| entry over the largest entry of the opposite sign (inf when there is none); raw_b after fix_sign"""
    r = raw_b.double().flatten().numpy()
    neg = -r[r < 0]
    return float("inf") if neg.size == 0 else float(r.max() / neg.max())


def planted_rank1(B, H, W, C, seed, noise=0.2):
    """a planted rank-1 component with one dominant position, plus noise: [B, H, W, C] fp32"""
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, H * W, 1, generator=g)
    u[:, 0] = 4.0                                      # one position clearly above the rest: the sign rule has a margin
    v = torch.randn(B, 1, C, generator=g)
    X = u * v + noise * torch.randn(B, H * W, C, generator=g)
    return (X + 0.5).view(B, H, W, C).contiguous()


# ------------------------------------------------------------------------------------------------ Ablation-CAM
def serf(x):
    """models/serf.py:23-24 in the tensor's own precision: x * erf(softplus(min(x, 50)))"""
    return x * torch.erf(torch.log1p(torch.exp(x.clamp(max=50.0))))


def activation(x, act):
    return x.clamp_min(0) if act == "relu" else serf(x)


def ablated_tokens(A, Wt, act, c0, nc):
    """zero channel c of A [B, H, W, C], 1x1 convolution with Wt [hidden, C] (no bias), activation, mean over the
    positions -> [B, nc, hidden] fp64, for c = c0 .. c0 + nc - 1"""
    A, Wt = A.double(), Wt.double()
    out = []
    for c in range(c0, c0 + nc):
        Az = A.clone()
        Az[..., c] = 0.0
        out.append(activation(Az.flatten(1, 2) @ Wt.t(), act).mean(1))
    return torch.stack(out, dim=1)


def ablated_tokens_rank1(A, Wt, act, c0, nc):
    """the same tokens through u - W[n, c] A[p, c] with u = A W^T computed once, fp64 (the CPU test pins it to
    ablated_tokens; hundreds of channels at hidden 768 would take the direct form half a minute)"""
    A, Wt = A.double().flatten(1, 2), Wt.double()
    u = A @ Wt.t()
    return torch.stack([activation(u - A[:, :, c:c + 1] * Wt[None, None, :, c], act).mean(1) for c in range(c0, c0 + nc)], dim=1)


def ablated_tokens_loops(A, Wt, act, c0, nc):
    import math
    a, w = A.double().numpy(), Wt.double().numpy()
    B, H, W, C = a.shape
    hidden = w.shape[0]
    out = np.zeros((B, nc, hidden))
    for b in range(B):
        for j in range(nc):
            for n in range(hidden):
                acc = 0.0
                for y in range(H):
                    for x in range(W):
                        u = sum(w[n, k] * a[b, y, x, k] for k in range(C) if k != c0 + j)
                        acc += max(u, 0.0) if act == "relu" else u * math.erf(math.log1p(math.exp(min(u, 50.0))))
                out[b, j, n] = acc / (H * W)
    return torch.from_numpy(out)


def ablation_weights(s, s_abl):
    """s [B], s_abl [B, C] -> w [B, C] = (s - s_c) / s (fp64), zeros where s == 0"""
    s, s_abl = s.double(), s_abl.double()
    return torch.where(s[:, None] != 0, (s[:, None] - s_abl) / s[:, None].where(s[:, None] != 0, torch.ones_like(s[:, None])),
                       torch.zeros_like(s_abl))


def ablation_weights_loops(s, s_abl):
    s, s_abl = s.double().numpy(), s_abl.double().numpy()
    out = np.zeros_like(s_abl)
    for b in range(s_abl.shape[0]):
        for c in range(s_abl.shape[1]):
            out[b, c] = (s[b] - s_abl[b, c]) / s[b] if s[b] != 0 else 0.0
    return torch.from_numpy(out)


def oracle_ablated_scores(orc, img, ids, seg, mask, target, channels, double=False):
    """eval-mode oracle: -> (s [B] = logits[b, target[b]], s_abl [B, len(channels)]) with s_abl[:, i] the same logit when
    channel channels[i] of the deepest feature map is zeroed by a forward hook"""
    o = copy.deepcopy(orc)
    o = o.double() if double else o
    o.eval()
    x = img.double() if double else img
    rows = torch.arange(img.shape[0])
    state = {"c": None}

    def hook(_m, _i, out):
        if state["c"] is None:
            return None
        out = out.clone()
        out[:, state["c"]] = 0.0
        return out

    h = GH.deepest_map_module(o).register_forward_hook(hook)
    try:
        with torch.no_grad():
            s = o(x, ids, seg, mask)[0][rows, target]
            cols = []
            for c in channels:
                state["c"] = int(c)
                cols.append(o(x, ids, seg, mask)[0][rows, target])
    finally:
        h.remove()
    return s, torch.stack(cols, dim=1)


def border_channels(C, nc, n=32):
    """a fixed list of n channels: the first, the last, both sides of every chunk border, filled up evenly"""
    want = {0, C - 1}
    for lo in range(nc, C, nc):
        want.update((lo - 1, lo))
    lo_last = C - nc                                   # the last chunk is moved back to end at C
    if lo_last > 0:
        want.update((lo_last - 1, lo_last))
    want = sorted(c for c in want if 0 <= c < C)[:n]
    k = 0
    while len(want) < min(n, C):
        c = (k * 7919) % C
        if c not in want:
            want.append(c)
        k += 1
    return sorted(want)


# ------------------------------------------------------------------------------------------------ op-level inputs
WEIGHT_MAPS = [(7, 7, 512), (7, 7, 2048), (5, 9, 48), (16, 16, 8), (1, 1, 4)]
WEIGHT_KINDS = ("abs", "signed", "zeros")


def weight_inputs(H, W, C, kind, B=2):
    """A, dA [B, H, W, C] fp32.  abs: |A| with a signed dA; signed: A with both signs (mean 1, so that no column sum
    comes near the formulas' pole at S_c = 0); zeros: the abs case with exact zeros in a third of dA.  dA is scaled like the
    gradient through a mean over the positions (1 / HW), which keeps 2 + S_c g away from 0."""
    g = torch.Generator().manual_seed(10000 * H + 100 * W + C + 7 * WEIGHT_KINDS.index(kind))
    A = torch.randn(B, H, W, C, generator=g)
    A = A + 1.0 if kind == "signed" else A.abs()
    dA = torch.randn(B, H, W, C, generator=g) * (0.25 / (H * W))
    if kind == "zeros":
        dA[torch.rand(B, H, W, C, generator=g) < 0.33] = 0.0
    return A.contiguous(), dA.contiguous()


EIGEN_MAPS = [(7, 7, 512), (5, 9, 48), (16, 16, 8), (2, 2, 256)]


def eigen_inputs(H, W, C, B=2):
    return planted_rank1(B, H, W, C, seed=100 * H + W + C)
