"""Oracle-side helpers of the Grad-CAM tests: the formula of vqamed2019/grad_cam2.py:139-158 restated twice in fp64
(tensor form and plain loops), the half-pixel bilinear resize, the overlay formula, and the autograd run on the CPU oracle
that yields the deepest feature map and its gradient."""
import copy

import numpy as np
import torch


def raw_cam(A, dA):
    """A, dA [B, H, W, C] -> the map before ReLU / normalisation, fp64 [B, H, W]"""
    A, dA = A.double(), dA.double()
    w = dA.mean(dim=(1, 2))                          # per sample
    return (A * w[:, None, None, :]).mean(dim=3)


def reference_cam(A, dA):
    """-> (cam [B, H, W] fp64 in [0, 1], valid [B]); zeros where the raw map has no positive value"""
    raw = raw_cam(A, dA)
    pos = raw.clamp_min(0.0)
    m = pos.flatten(1).max(dim=1).values
    valid = m > 0
    cam = torch.where(valid[:, None, None], pos / m.clamp_min(1e-300)[:, None, None], torch.zeros_like(pos))
    return cam, valid


def reference_cam_loops(A, dA):
    """the same arithmetic written element by element"""
    A, dA = A.double().numpy(), dA.double().numpy()
    B, H, W, C = A.shape
    out = np.zeros((B, H, W))
    for b in range(B):
        w = [sum(dA[b, y, x, c] for y in range(H) for x in range(W)) / (H * W) for c in range(C)]
        for y in range(H):
            for x in range(W):
                out[b, y, x] = max(sum(w[c] * A[b, y, x, c] for c in range(C)) / C, 0.0)
        m = out[b].max()
        out[b] = out[b] / m if m > 0 else 0.0
    return torch.from_numpy(out)


def bilinear_resize(cam, IH, IW):
    """half-pixel centres, edge clamp (the INTER_LINEAR convention), fp64: cam [B, H, W] -> [B, IH, IW]"""
    cam = cam.double().numpy()
    B, H, W = cam.shape

    def axis(n_out, n_in):
        s = (np.arange(n_out) + 0.5) * (n_in / n_out) - 0.5
        s = np.maximum(s, 0.0)
        i0 = np.floor(s).astype(np.int64)
        f = s - i0
        edge = i0 >= n_in - 1
        i0 = np.where(edge, n_in - 1, i0)
        f = np.where(edge, 0.0, f)
        return i0, np.minimum(i0 + 1, n_in - 1), f

    y0, y1, fy = axis(IH, H)
    x0, x1, fx = axis(IW, W)
    top = cam[:, y0][:, :, x0] * (1 - fx) + cam[:, y0][:, :, x1] * fx
    bot = cam[:, y1][:, :, x0] * (1 - fx) + cam[:, y1][:, :, x1] * fx
    return torch.from_numpy(top * (1 - fy)[None, :, None] + bot * fy[None, :, None])


def overlay_formula(up, image_u8, jet, alpha):
    """up fp32 [B, IH, IW] (numpy), image uint8 [B, IH, IW, 3], jet uint8 [256, 3] -> uint8, in fp32 like the kernel"""
    q = (np.float32(255.0) * up.astype(np.float32)).astype(np.uint8)
    v = np.float32(alpha) * jet[q].astype(np.float32) + image_u8.astype(np.float32)
    return np.clip(v, 0, 255).astype(np.uint8)


def deepest_map_module(orc):
    m = orc.transformer.trans.model
    return m.layer4 if hasattr(m, "layer4") else m.blocks[-1]


def oracle_feature_gradient(orc, img, ids, seg, mask, target=None, double=False):
    """eval-mode oracle: -> (logits, A, dA, target) with A, dA NHWC, via a forward hook on the deepest map"""
    o = copy.deepcopy(orc)
    o = o.double() if double else o
    o.eval()
    kept = {}

    def hook(_m, _i, out):
        out.retain_grad()
        kept["A"] = out

    h = deepest_map_module(o).register_forward_hook(hook)
    try:
        logits = o(img.double() if double else img, ids, seg, mask)[0]
    finally:
        h.remove()
    if target is None:
        target = logits.argmax(1)
    logits[torch.arange(logits.shape[0]), target].sum().backward()
    A = kept["A"]
    return logits.detach(), A.detach().permute(0, 2, 3, 1).contiguous(), A.grad.permute(0, 2, 3, 1).contiguous(), target
