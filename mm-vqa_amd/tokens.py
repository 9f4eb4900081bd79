"""A device-resident cache of visual tokens: with the CNN body and its five taps frozen and the
backbone's BatchNorms on their running statistics, the num_vis tokens of an image are a function of the image alone, so
they are computed once and every later training step starts at the embedding (Model.forward_cached).

    cache = TokenCache(model, n_images, views=K)
    cache.fill(index, img, view=0)            # eval-mode backbone + taps on img, scattered into rows `index`
    logits, _, _ = model.forward_cached(cache, index, view, ids, seg, mask)
    cache.check(model)                        # MMVQAError once the backbone, a tap or a running statistic has moved
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L


def _fingerprint(model):
    """fp64 (sum, sum of squares) of the parameters under transformer.trans. and of the backbone's BatchNorm running
    buffers, as one device tensor [4]; nothing here waits for the device"""
    lo, hi = model.token_range()
    p = model.flat_params[lo:hi].double()
    bufs = [buf for name, buf in model.named_buffers() if name.startswith("transformer.trans.") and buf.dtype == torch.float32]
    b = torch.cat([t.reshape(-1) for t in bufs]).double() if bufs else p.new_zeros(1)
    return torch.stack([p.sum(), (p * p).sum(), b.sum(), (b * b).sum()])


class TokenCache:
    def __init__(self, model, n_images: int, views: int = 1):
        if n_images < 1 or views < 1:
            raise ValueError(f"a token cache holds at least one image and one view, not {n_images} images x {views} views")
        d = model._desc
        self.tokens = torch.zeros(int(n_images), int(views), d.num_vis, d.hidden, dtype=torch.float32,
                                  device=model.flat_params.device)
        self.fingerprint = None      # device fp64 [4], set by the first fill
        self._model = model          # the model whose backbone fills the cache

    @property
    def n_images(self):
        return self.tokens.shape[0]

    @property
    def views(self):
        return self.tokens.shape[1]

    @property
    def nbytes(self):
        return self.tokens.numel() * 4

    def _rows(self, index, B):
        """the distinct rows a fill writes, validated on the host -> int32 CPU tensor [B]"""
        from .model import _host_ints
        idx = _host_ints("index", index)
        if len(idx) != B:
            raise ValueError(f"index has {len(idx)} entries for {B} images")
        seen = {}
        for b, v in enumerate(idx):
            if not 0 <= v < self.n_images:
                raise ValueError(f"index[{b}] = {v} is outside the cache's {self.n_images} images (0 .. {self.n_images - 1})")
            if v in seen:
                raise ValueError(f"index[{b}] = {v} repeats index[{seen[v]}]: a fill writes every row once")
            seen[v] = b
        return torch.tensor(idx, dtype=torch.int32)

    def fill(self, index, img, view: int = 0):
        """The tokens of img [B, 3, H, W] -> rows index[b] of view `view`: the eval-mode backbone and its taps as
        Model.visual_tokens runs them (no_grad, model.training and the dropout counter restored), then one scatter from
        the workspace.  index: B distinct host integers."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("visual tokens (visual_tokens / forward_tokens) are fp32 in this version: call it "
                                      "outside torch.autocast")
        model = self._model
        if isinstance(view, bool) or int(view) != view or not 0 <= int(view) < self.views:
            raise ValueError(f"view = {view!r} is outside the cache's {self.views} views (0 .. {self.views - 1})")
        B = img.shape[0]
        rows = self._rows(index, B)
        model._refuse_after_grouped("TokenCache.fill")
        if self.fingerprint is None:
            self.fingerprint = _fingerprint(model)
        else:                        # every later fill: rows from other weights than the first fill's would pass check()
            self._compare(model, "TokenCache.fill: the model has changed since this cache's first fill")
        model._run_backbone_eval(img)
        vp = C.c_void_p()
        L.check(L.lib().mmvqa_engine_visual_tokens(model._handle, C.byref(vp)))
        pinned = torch.empty(B, dtype=torch.int32, pin_memory=True)
        pinned.copy_(rows)
        dev_rows = pinned.to(img.device, non_blocking=True)
        d = model._desc
        L.check(L.lib().mmvqa_tokens_scatter(L.stream_ptr(), vp, L.ptr(dev_rows), int(view), L.ptr(self.tokens),
                                             self.n_images, self.views, B, d.hidden, d.num_vis))
        return self

    def check(self, model):
        """raises MMVQAError when the model's backbone, taps or BatchNorm running statistics are not the ones the cache was
        filled from (one small read of the device)"""
        if self.fingerprint is None:
            raise L.MMVQAError("TokenCache.check: the cache has not been filled")
        self._compare(model, "the token cache is stale")

    def _compare(self, model, what):
        now = _fingerprint(model).to(self.fingerprint.device)
        if not bool((now == self.fingerprint).all()):
            raise L.MMVQAError(f"{what}: parameters under transformer.trans. or the backbone's BatchNorm "
                               f"running statistics have changed since it was filled (fingerprint {self.fingerprint.tolist()} "
                               f"then, {now.tolist()} now); fill it again")

    def save(self, path):
        """tokens and fingerprint -> one .npz"""
        if self.fingerprint is None:
            raise L.MMVQAError("TokenCache.save: the cache has not been filled")
        with open(path, "wb") as f:
            np.savez(f, tokens=self.tokens.cpu().numpy(), fingerprint=self.fingerprint.cpu().numpy())

    def load(self, path):
        """the .npz of save() -> this cache (same [N, K, num_vis, hidden]); check(model) then tells whether it is this
        model's"""
        with np.load(path) as z:
            tok, fp = z["tokens"], z["fingerprint"]
        if tuple(tok.shape) != tuple(self.tokens.shape) or tok.dtype != np.float32 or fp.shape != (4,):
            raise ValueError(f"{path} holds tokens {tuple(tok.shape)} {tok.dtype}, this cache is {tuple(self.tokens.shape)} float32")
        self.tokens.copy_(torch.from_numpy(tok))
        self.fingerprint = torch.from_numpy(fp.astype(np.float64)).to(self.tokens.device)
        return self
