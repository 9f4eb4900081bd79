"""Grad-CAM for VQA answers (vqamed2019/grad_cam2.py:139-188, batched): where in the image an answer came from.

  grad_cam(model, img, ids, seg, mask, target=None, image_u8=None, alpha=0.4) -> GradCam
      eval forward + data-only backward to the deepest backbone feature map (Model.feature_gradient), then the HIP
      launches of csrc/gradcam.hip: channel weights, ReLU, normalisation, bilinear resize to the image size, JET colours
      blended over the uint8 image the model saw.  Everything stays on the device; nothing waits for it.
  cam_from_maps(A, dA, out_hw, image_u8=None, alpha=0.4)  the op entry mmvqa_gradcam on given maps
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


def cam_from_maps(A, dA, out_hw, image_u8=None, alpha=0.4):
    """mmvqa_gradcam on A, dA [B, H, W, C] fp32 (device) -> (cam [B,H,W], heatmap [B,IH,IW], overlay or None, valid [B])"""
    if not A.is_cuda:
        raise L.MMVQAError("Grad-CAM runs on the GPU only (no CPU fallback)")
    A, dA = A.contiguous().float(), dA.contiguous().float()
    B, H, W, Cc = A.shape
    IH, IW = int(out_hw[0]), int(out_hw[1])
    dev = A.device
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
    L.check(L.lib().mmvqa_gradcam(L.stream_ptr(), L.ptr(A), L.ptr(dA), B, H, W, Cc, L.ptr(cam), L.ptr(valid), L.ptr(up),
                                  IH, IW, L.ptr(image_u8), L.ptr(jet), float(alpha), L.ptr(overlay)))
    return cam, up, overlay, valid


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
