"""Grad-CAM for VQA answers (vqamed2019/grad_cam2.py:139-188, batched): where in the image an answer came from.

  grad_cam(model, img, ids, seg, mask, target=None, image_u8=None, alpha=0.4) -> GradCam
      eval forward + data-only backward to the deepest backbone feature map (Model.feature_gradient), then the HIP
      launches of csrc/gradcam.hip: channel weights, ReLU, normalisation, bilinear resize to the image size, JET colours
      blended over the uint8 image the model saw.  Everything stays on the device; nothing waits for it.
  cam_from_maps(A, dA, out_hw, image_u8=None, alpha=0.4)  the op entry mmvqa_gradcam on given maps
  attribute(model, img, ids, seg, mask, method=...) -> Attribution
      the other methods of vqamed2019/grad_cam.py:65-72: only the channel weights (or, for
      eigencam, the map before the ReLU) differ, the tail is Grad-CAM's
  jet_table()                                         the 256 x 3 uint8 colour table (host)

Decisions: the channel weights are per-sample means (the reference runs batch 1); a sample whose map
has no positive value gets zeros, valid = 0 and the plain image; the colour table is generated from the standard
piecewise-linear jet definition and the resize is the half-pixel bilinear rule -- both restated, not pinned against
OpenCV, which the reference calls for them.
"""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import _lib as L


class GradCam(NamedTuple):
    logits: torch.Tensor              # [B, classes]
    target: torch.Tensor              # [B] int64: the class each map explains
    cam: torch.Tensor                 # [B, H, W] fp32 in [0, 1] on the feature map's grid
    heatmap: torch.Tensor             # [B, IH, IW] fp32: cam resized to the image
    overlay: Optional[torch.Tensor]   # [B, IH, IW, 3] uint8 RGB, or None without image_u8
    valid: torch.Tensor               # [B] int32: 0 where the target class has no positive evidence (cam is zeros)


def jet_table():
    """256 x 3 uint8 RGB: channel value clamp(1.5 - |4x - k|, 0, 1) at x = i / 255 with k = 3 (red), 2 (green), 1 (blue)"""
    x = np.arange(256, dtype=np.float64) / 255.0
    rgb = [np.clip(1.5 - np.abs(4.0 * x - k), 0.0, 1.0) for k in (3.0, 2.0, 1.0)]
    return np.round(np.stack(rgb, axis=1) * 255.0).astype(np.uint8)


_JET_DEV = {}


def _jet_on(device):
    key = (device.type, device.index)
    if key not in _JET_DEV:
        _JET_DEV[key] = torch.from_numpy(jet_table()).to(device)     # uploaded once per device
    return _JET_DEV[key]


def _outputs(B, H, W, out_hw, image_u8, dev):
    """the output buffers every CAM launch fills -> (cam, up, valid, image_u8, jet, overlay, IH, IW)"""
    IH, IW = int(out_hw[0]), int(out_hw[1])
    cam = torch.empty(B, H, W, dtype=torch.float32, device=dev)
    up = torch.empty(B, IH, IW, dtype=torch.float32, device=dev)
    valid = torch.empty(B, dtype=torch.int32, device=dev)
    overlay = jet = None
    if image_u8 is not None:
        image_u8 = image_u8.to(dev).contiguous()
        if image_u8.dtype != torch.uint8 or tuple(image_u8.shape) != (B, IH, IW, 3):
            raise ValueError(f"image_u8 must be uint8 [B, {IH}, {IW}, 3]")
        overlay = torch.empty_like(image_u8)
        jet = _jet_on(dev)
    return cam, up, valid, image_u8, jet, overlay, IH, IW


def cam_from_maps(A, dA, out_hw, image_u8=None, alpha=0.4):
    """mmvqa_gradcam on A, dA [B, H, W, C] fp32 (device) -> (cam [B,H,W], heatmap [B,IH,IW], overlay or None, valid [B])"""
    if not A.is_cuda:
        raise L.MMVQAError("Grad-CAM runs on the GPU only (no CPU fallback)")
    A, dA = A.contiguous().float(), dA.contiguous().float()
    B, H, W, Cc = A.shape
    cam, up, valid, image_u8, jet, overlay, IH, IW = _outputs(B, H, W, out_hw, image_u8, A.device)
    L.check(L.lib().mmvqa_gradcam(L.stream_ptr(), L.ptr(A), L.ptr(dA), B, H, W, Cc, L.ptr(cam), L.ptr(valid), L.ptr(up),
                                  IH, IW, L.ptr(image_u8), L.ptr(jet), float(alpha), L.ptr(overlay)))
    return cam, up, overlay, valid


METHODS = ("gradcam", "gradcam++", "xgradcam", "eigencam", "ablationcam")    # vqamed2019/grad_cam.py:65-72 without scorecam
_WEIGHT_METHOD = {"gradcam": 0, "gradcam++": 1, "xgradcam": 2}
ABLATION_VARIANTS = 256    # rows of one forward_tokens call of Ablation-CAM


class Attribution(NamedTuple):
    logits: torch.Tensor
    target: torch.Tensor
    cam: torch.Tensor
    heatmap: torch.Tensor
    overlay: Optional[torch.Tensor]
    valid: torch.Tensor
    method: str
    weights: Optional[torch.Tensor]   # [B, C] channel weights, None for eigencam
    resid: Optional[torch.Tensor]     # [B] |G u - lambda u| / lambda of the power iteration (eigencam only)


def cam_weights(A, dA, method):
    """mmvqa_cam_weights: the channel weights w [B, C] of gradcam / gradcam++ / xgradcam from A, dA [B, H, W, C]"""
    if not A.is_cuda:
        raise L.MMVQAError("attribution runs on the GPU only (no CPU fallback)")
    A, dA = A.contiguous().float(), dA.contiguous().float()
    B, H, W, Cc = A.shape
    w = torch.empty(B, Cc, dtype=torch.float32, device=A.device)
    L.check(L.lib().mmvqa_cam_weights(L.stream_ptr(), _WEIGHT_METHOD[method], L.ptr(A), L.ptr(dA), B, H, W, Cc, L.ptr(w)))
    return w


def cam_from_weights(A, out_hw, w=None, raw=None, image_u8=None, alpha=0.4):
    """mmvqa_cam_from_weights: the tail of Grad-CAM with the channel weights w [B, C], or the map before the ReLU raw
    [B, H, W], from memory -> (cam, heatmap, overlay or None, valid)"""
    if not A.is_cuda:
        raise L.MMVQAError("attribution runs on the GPU only (no CPU fallback)")
    A = A.contiguous().float()
    B, H, W, Cc = A.shape
    w = None if w is None else w.contiguous().float()
    raw = None if raw is None else raw.contiguous().float()
    cam, up, valid, image_u8, jet, overlay, IH, IW = _outputs(B, H, W, out_hw, image_u8, A.device)
    L.check(L.lib().mmvqa_cam_from_weights(L.stream_ptr(), L.ptr(A), L.ptr(w), L.ptr(raw), B, H, W, Cc, L.ptr(cam),
                                           L.ptr(valid), L.ptr(up), IH, IW, L.ptr(image_u8), L.ptr(jet), float(alpha),
                                           L.ptr(overlay)))
    return cam, up, overlay, valid


def eigencam_raw(A):
    """mmvqa_eigencam_raw on A [B, H, W, C] -> (raw [B, H, W], resid [B])"""
    if not A.is_cuda:
        raise L.MMVQAError("attribution runs on the GPU only (no CPU fallback)")
    A = A.contiguous().float()
    B, H, W, Cc = A.shape
    gram = torch.empty(B, H * W, H * W, dtype=torch.float32, device=A.device)
    raw = torch.empty(B, H, W, dtype=torch.float32, device=A.device)
    resid = torch.empty(B, dtype=torch.float32, device=A.device)
    L.check(L.lib().mmvqa_eigencam_raw(L.stream_ptr(), L.ptr(A), B, H, W, Cc, L.ptr(gram), L.ptr(raw), L.ptr(resid)))
    return raw, resid


def ablated_tokens(A, Wt, act, c0, nc, u=None):
    """mmvqa_ablated_tokens: the tap's visual token with channel c of A [B, H, W, C] zeroed, for c in [c0, c0 + nc)
    -> (tokens [B, nc, hidden], u).  Wt [hidden, C]; u: the scratch an earlier chunk of the same pass returned."""
    A, Wt = A.contiguous().float(), Wt.contiguous().float()
    B, H, W, Cc = A.shape
    hidden = Wt.shape[0]
    first = u is None
    if first:
        u = torch.empty(B * H * W, hidden, dtype=torch.float32, device=A.device)
    tokens = torch.empty(B, nc, hidden, dtype=torch.float32, device=A.device)
    L.check(L.lib().mmvqa_ablated_tokens(L.stream_ptr(), L.ptr(A), L.ptr(Wt), L.ptr(u), B, H * W, Cc, hidden, int(act),
                                         int(c0), int(nc), 1 if first else 0, L.ptr(tokens)))
    return tokens, u


def ablation_weights(model, A, vis, ids, seg, mask, logits, target, variants=ABLATION_VARIANTS):
    """Ablation-CAM's w [B, C] = (s - s_c) / s with s = logits[b, target[b]] and s_c the same logit with channel c of A
    zeroed: the ablated visual tokens of a chunk of channels in one launch, forward_tokens on the B * chunk variants
    (the other four tokens and the text repeated), the target column gathered.  A last chunk that would be ragged is
    moved back to end at C (its first channels are computed twice)."""
    B, H, W, Cc = A.shape
    Wt, k, act = model.deepest_tap()
    nc = max(1, min(Cc, int(variants) // B))
    s_abl = torch.empty(B, Cc, dtype=torch.float32, device=A.device)
    rep = lambda t: t.repeat_interleave(nc, dim=0)
    ids_r, seg_r, mask_r = rep(ids), rep(seg), rep(mask)
    col = target.view(B, 1, 1).expand(B, nc, 1)
    u = None
    for lo in range(0, Cc, nc):
        c0 = min(lo, Cc - nc)
        tok, u = ablated_tokens(A, Wt, act, c0, nc, u)
        v = vis[:, None].repeat(1, nc, 1, 1)                        # [B, nc, num_vis, hidden]
        v[:, :, k] = tok
        out = model.forward_tokens(v.view(B * nc, *vis.shape[1:]), ids_r, seg_r, mask_r)[0]
        s_abl[:, c0:c0 + nc] = out.view(B, nc, -1).gather(2, col)[:, :, 0]
    s = logits.gather(1, target.view(B, 1))[:, 0].contiguous()
    w = torch.empty(B, Cc, dtype=torch.float32, device=A.device)
    L.check(L.lib().mmvqa_ablation_weights(L.stream_ptr(), L.ptr(s), L.ptr(s_abl), B, Cc, L.ptr(w)))
    return w


def attribute(model, img, input_ids, segment_ids, input_mask, method="gradcam", target=None, image_u8=None, alpha=0.4):
    """vqamed2019/grad_cam.py's --method switch: gradcam, gradcam++, xgradcam (one backward to the deepest map),
    eigencam (no backward, no target dependence) and ablationcam (C token forwards).  Every method ends in Grad-CAM's
    tail: ReLU, division by the per-sample maximum, valid, resize, overlay.  method="gradcam" gives what grad_cam gives."""
    if method == "scorecam":
        raise NotImplementedError("scorecam is not built: it needs C whole-model forwards per image (2 048 for ResNet-152) "
                                  "and no engine capability beyond forward_tokens and the weight kernels, so it can follow")
    if method not in METHODS:
        raise ValueError(f"method={method!r}: one of {', '.join(METHODS)}")
    w = resid = None
    if method in _WEIGHT_METHOD:
        logits, A, dA, target = model.feature_gradient(img, input_ids, segment_ids, input_mask, target)
        w = cam_weights(A, dA, method)
    else:
        logits, A = model.feature_map(img, input_ids, segment_ids, input_mask)
        B = logits.shape[0]
        target = logits.argmax(1) if target is None else torch.as_tensor(target, device=logits.device).long().reshape(B)
        if method == "ablationcam":
            vis = model._read_visual_tokens(B)
            w = ablation_weights(model, A, vis, input_ids, segment_ids, input_mask, logits, target)
    if method == "eigencam":
        raw, resid = eigencam_raw(A)
        cam, up, overlay, valid = cam_from_weights(A, img.shape[2:], raw=raw, image_u8=image_u8, alpha=alpha)
    else:
        cam, up, overlay, valid = cam_from_weights(A, img.shape[2:], w=w, image_u8=image_u8, alpha=alpha)
    return Attribution(logits, target, cam, up, overlay, valid, method, w, resid)


def grad_cam(model, img, input_ids, segment_ids, input_mask, target=None, image_u8=None, alpha=0.4):
    """image_u8: uint8 [B, IH, IW, 3], the Resize + CenterCrop image behind `img` (augment.DeviceAugment.last_uint8);
    None skips the overlay."""
    logits, A, dA, target = model.feature_gradient(img, input_ids, segment_ids, input_mask, target)
    cam, up, overlay, valid = cam_from_maps(A, dA, img.shape[2:], image_u8, alpha)
    return GradCam(logits, target, cam, up, overlay, valid)


def image_u8_from_normalised(img, mean=0.5, std=0.5):
    """the uint8 image behind a ToTensor + Normalize(mean, std) tensor [B, 3, H, W] -> [B, H, W, 3] (exact for images
    that came from bytes: the rounding undoes the two fp32 operations)"""
    return (img * std + mean).mul(255.0).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
