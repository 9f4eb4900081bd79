"""Loss scaling for mixed-precision training: ``GradScaler`` with the API and defaults of ``torch.cuda.amp.GradScaler``
(pretrain/roco_utils.py:224-245, vqamed2019/utils.py:641-657), driving ``FusedAdam`` over the model's flat gradient
buffer.  torch's own scaler cannot drive it: it walks ``optimizer.param_groups[i]["params"]``.

Arithmetic equals torch's: ``inv_scale = float32(1 / double(scale))``; the non-finite check and the in-place unscale are
one HIP launch over the flat gradients (mmvqa_amp_unscale); the scale / growth-tracker update is a one-thread launch with
``torch._amp_update_scale_``'s semantics (mmvqa_amp_update_scale).  ``step`` reads the 4-byte found-inf flag on the host
once per step, as torch's ``GradScaler.step`` does, and skips the optimizer on a non-finite gradient: parameters, Adam
moments and ``FusedAdam.step_count`` stay untouched.  Under data parallelism call ``step`` after the gradient reducer has
finished, so that every rank checks the same (all-reduced) gradients and makes the same decision.
"""
from __future__ import annotations

import torch

from . import _lib as L

_READY, _UNSCALED, _STEPPED = 0, 1, 2


class GradScaler:
    def __init__(self, init_scale=2.0 ** 16, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000, enabled=True):
        self._enabled = bool(enabled)
        if self._enabled:
            if growth_factor <= 1.0:
                raise ValueError("The growth factor must be > 1.0.")
            if backoff_factor >= 1.0:
                raise ValueError("The backoff factor must be < 1.0.")
        self._init_scale = float(init_scale)
        self._growth_factor = float(growth_factor)
        self._backoff_factor = float(backoff_factor)
        self._growth_interval = int(growth_interval)
        self._init_growth_tracker = 0
        self._scale = None            # float32 [1] on the gradients' device
        self._growth_tracker = None   # int32 [1]
        self._found_inf = None        # float32 [1] of the current step
        self._inv_scale = None
        self._stage = _READY

    def is_enabled(self):
        return self._enabled

    def _lazy_init(self, device):
        if self._scale is None:
            self._scale = torch.full((1,), self._init_scale, dtype=torch.float32, device=device)
            self._growth_tracker = torch.full((1,), self._init_growth_tracker, dtype=torch.int32, device=device)

    # ------------------------------------------------------------------ torch.cuda.amp.GradScaler API
    def scale(self, outputs):
        """outputs * scale (a tensor, or an iterable of tensors); unchanged when disabled"""
        if not self._enabled:
            return outputs
        if isinstance(outputs, torch.Tensor):
            self._lazy_init(outputs.device)
            return outputs * self._scale.to(device=outputs.device, non_blocking=True)
        return type(outputs)(self.scale(o) for o in outputs)

    def unscale_(self, optimizer):
        """non-finite check of the model's flat gradients and grads *= float32(1 / double(scale)), once per step"""
        if not self._enabled:
            return
        if self._stage == _UNSCALED:
            raise RuntimeError("unscale_() has already been called on this optimizer since the last update().")
        if self._stage == _STEPPED:
            raise RuntimeError("unscale_() is being called after step().")
        grads = optimizer.model.flat_grads
        self._lazy_init(grads.device)
        self._inv_scale = self._scale.double().reciprocal().float()
        self._found_inf = torch.zeros(1, dtype=torch.float32, device=grads.device)
        L.check(L.lib().mmvqa_amp_unscale(L.stream_ptr(), L.ptr(grads), grads.numel(), L.ptr(self._inv_scale),
                                          L.ptr(self._found_inf), 1))
        self._stage = _UNSCALED

    def step(self, optimizer, *args, **kwargs):
        """unscale_ (unless done), then optimizer.step(*args, **kwargs) unless a gradient is inf / nan; returns the
        optimizer's return value, or None when the step was skipped"""
        if not self._enabled:
            return optimizer.step(*args, **kwargs)
        if self._stage == _STEPPED:
            raise RuntimeError("step() has already been called since the last update().")
        if getattr(optimizer, "_stream", None) is not None:
            raise RuntimeError("GradScaler: the optimizer updates ranges during backward (FusedAdam.overlap_backward); "
                               "the whole gradient must be checked before the first update")
        if self._stage == _READY:
            self.unscale_(optimizer)
        ret = None
        if not float(self._found_inf.item()):   # the one host read of the step
            ret = optimizer.step(*args, **kwargs)
        self._stage = _STEPPED
        return ret

    def update(self, new_scale=None):
        """scale / growth tracker after this step (torch._amp_update_scale_), or set the scale to new_scale"""
        if not self._enabled:
            return
        if self._scale is None:
            raise AssertionError("Attempted update but _scale is None: scale(loss) was never called.")
        if new_scale is None and self._found_inf is None:
            raise AssertionError("No inf checks were recorded prior to update.")
        if new_scale is not None:
            if isinstance(new_scale, torch.Tensor):
                self._scale.copy_(new_scale)
            else:
                self._scale.fill_(float(new_scale))
        elif self._found_inf is not None:
            L.check(L.lib().mmvqa_amp_update_scale(L.stream_ptr(), L.ptr(self._scale), L.ptr(self._growth_tracker),
                                                   L.ptr(self._found_inf), self._growth_factor, self._backoff_factor,
                                                   self._growth_interval))
        self._found_inf = None
        self._inv_scale = None
        self._stage = _READY

    def found_inf(self):
        """True when the current step saw a non-finite gradient (after unscale_ / step)"""
        return self._found_inf is not None and bool(self._found_inf.item())

    def get_scale(self):
        if not self._enabled:
            return 1.0
        return self._init_scale if self._scale is None else float(self._scale.item())

    def get_growth_factor(self):
        return self._growth_factor

    def get_backoff_factor(self):
        return self._backoff_factor

    def get_growth_interval(self):
        return self._growth_interval

    def _get_growth_tracker(self):
        if self._growth_tracker is None:
            return self._init_growth_tracker
        return int(self._growth_tracker.item())

    def state_dict(self):
        if not self._enabled:
            return {}
        return {"scale": self.get_scale(), "growth_factor": self._growth_factor, "backoff_factor": self._backoff_factor,
                "growth_interval": self._growth_interval, "_growth_tracker": self._get_growth_tracker()}

    def load_state_dict(self, state_dict):
        if not self._enabled:
            return
        if len(state_dict) == 0:
            raise RuntimeError("The source state dict is empty, possibly because it was saved from a disabled instance "
                               "of GradScaler.")
        self._init_scale = float(state_dict["scale"])
        if self._scale is not None:
            self._scale.fill_(self._init_scale)
        self._growth_factor = float(state_dict["growth_factor"])
        self._backoff_factor = float(state_dict["backoff_factor"])
        self._growth_interval = int(state_dict["growth_interval"])
        self._init_growth_tracker = int(state_dict["_growth_tracker"])
        if self._growth_tracker is not None:
            self._growth_tracker.fill_(self._init_growth_tracker)
