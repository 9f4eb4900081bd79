"""Fused Adam over the model's flat parameter / gradient buffers (one kernel per step, or -- overlap_backward() -- one
per finished gradient range, enqueued while the backward pass is still running: the update is 32 bytes of HBM traffic
per parameter and no matrix work, the backbone backward is the opposite).

Same update as ``optim.Adam(model.parameters(), lr)`` at pretrain/roco_train.py:90 and
vqamed2019/train.py:160 (betas (0.9, 0.999), eps 1e-8, no weight decay).  Parameters whose
gradient stays zero (the reference's never-used ``norm2`` / ``fc``) do not move, which equals the
reference's "grad is None => skipped".

Beyond the reference: optimizer groups (a learning rate / weight decay per set of tensors), weight decay in the
``torch.optim.AdamW`` (decoupled, the default) or ``torch.optim.Adam(weight_decay=)`` (L2) form, and frozen parameters
(``requires_grad=False``: neither the parameter nor its moments move).  All of it is one segment table in device
memory and still one launch per step or per range (``mmvqa_adam_groups``); the table is uploaded when a learning rate,
a weight decay or a parameter's ``requires_grad`` changes and not otherwise.  Built as before -- no groups, no weight
decay, nothing frozen -- the optimizer calls ``mmvqa_adam`` as before.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import operator
import re

import torch

from . import _lib as L

_REQUIRES_GRAD = operator.attrgetter("requires_grad")
_NORM_WEIGHT = re.compile(r"(^|\.)(LayerNorm|norm\d*|ln\d+|bn\d+|downsample\.1|classifier\.1|to_logits\.0)\.weight$")


def no_decay(name: str) -> bool:
    """ready ``match`` predicate of a group: the tensors that are customarily left out of weight decay -- every bias and
    the scale of every LayerNorm (the embedding LayerNorm included) and BatchNorm"""
    return name.endswith(".bias") or _NORM_WEIGHT.search(name) is not None


def _matches(match, name):
    if callable(match):
        return bool(match(name))
    if isinstance(match, str):
        match = (match,)
    return name.startswith(tuple(match))


def assign_groups(names, groups):
    """group index of every name: the first group of `groups` whose ``match`` (a prefix, a tuple of prefixes or a
    callable(name)) accepts it, counted from 1; 0 = the default group (no match)"""
    out = []
    for n in names:
        out.append(next((i + 1 for i, g in enumerate(groups) if _matches(g["match"], n)), 0))
    return out


def merge_segments(ranges):
    """[(lo, hi, lr, weight_decay, mode)] in buffer order -> the same with adjacent ranges of equal settings merged;
    a frozen range has no settings (lr = weight_decay = 0), so neighbouring frozen tensors merge whatever their group"""
    out = []
    for lo, hi, lr, wd, mode in ranges:
        if mode == L.ADAM_FROZEN:
            lr = wd = 0.0
        if out and out[-1][1] == lo and out[-1][2:] == [lr, wd, mode]:
            out[-1][1] = hi
        else:
            out.append([lo, hi, lr, wd, mode])
    if len(out) > L.ADAM_MAX_SEGS:
        raise L.MMVQAError(f"FusedAdam: the groups split the parameter buffer into {len(out)} segments, more than the "
                           f"{L.ADAM_MAX_SEGS} one launch takes")
    return [tuple(s) for s in out]


def ema_decay_at(ema_decay, updates, warmup):
    """decay of the averaging step after `updates` earlier ones: ema_decay, or with warm-up min(ema_decay, (1 + t) / (10 + t))
    -- 0.1 at first, so that the average follows the first steps instead of remembering the initial weights, 0.5 after
    8 updates, and ema_decay from t >= (10 ema_decay - 1) / (1 - ema_decay) on"""
    return min(ema_decay, (1.0 + updates) / (10.0 + updates)) if warmup else ema_decay


class FusedAdam:
    def __init__(self, model, lr=2e-5, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, groups=None,
                 ema_decay=None, ema_warmup=False):
        """groups: list of dicts {match: prefix | tuple of prefixes | callable(name), lr?, weight_decay?}; a parameter
        belongs to the first group that matches its name, the rest to the default group (lr, weight_decay), which is
        param_groups[0].  decoupled: weight decay as torch.optim.AdamW applies it (p *= 1 - lr wd), else as
        torch.optim.Adam(weight_decay=) does (g += wd p).  betas and eps are shared: a group that names its own is
        refused.  Parameters with requires_grad=False are skipped (read again at every step): they and their moments
        keep their values, also when they were frozen after some steps.
        ema_decay in [0, 1): keep self.ema, a copy of the flat parameter buffer that follows it in every step,
        ema += (p_new - ema) * (1 - decay), in the launch that updates the parameters; ema_warmup: the decay of
        ema_decay_at.  A step that amp.GradScaler skips leaves the average and its counter alone.  A frozen tensor's
        average is not touched: frozen from the start it stays equal to the tensor, frozen later it keeps the average it
        had at that moment (it does not go on approaching the now constant weights).  Only parameters are averaged:
        BatchNorm running statistics and num_batches_tracked are buffers, and averaged() evaluates the averaged weights
        with the live buffers -- torch.optim.swa_utils.AveragedModel(use_buffers=False) without the update_bn pass."""
        if ema_decay is None and ema_warmup:
            raise ValueError("FusedAdam: ema_warmup without ema_decay")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:    # (NaN fails the comparison too)
            raise ValueError(f"FusedAdam: ema_decay={ema_decay} is outside [0, 1)")
        self.model = model
        groups = [dict(g) for g in (groups or [])]
        for g in groups:
            extra = set(g) - {"match", "lr", "weight_decay"}
            if "match" not in g or extra:
                raise ValueError(f"FusedAdam: a group is {{match, lr?, weight_decay?}}, not {sorted(g)} (betas and eps are "
                                 "shared by all groups)")
        self.decoupled = bool(decoupled)
        # ReduceLROnPlateau-compatible: one dict per group, the default group first
        self.param_groups = [dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)]
        self.param_groups += [dict(lr=g.get("lr", lr), betas=betas, eps=eps, weight_decay=g.get("weight_decay", weight_decay))
                              for g in groups]
        # (name, parameter, lo, hi) per tensor; a bare pair of flat buffers (anything with flat_params / flat_grads) is one
        # tensor without a name that is never frozen
        table = getattr(model, "_param_ranges", None)
        self._ranges = table() if table is not None else [("", None, 0, model.flat_params.numel())]
        self._names = [name for name, _, _, _ in self._ranges]
        self._params = tuple(p for _, p, _, _ in self._ranges if p is not None)
        self._group_of = assign_groups(self._names, groups)
        self.m = torch.zeros_like(model.flat_params)
        self.v = torch.zeros_like(model.flat_params)
        self.step_count = 0
        self._for = model.flat_params.data_ptr()
        self._stream = None          # overlap_backward(): the stream the early updates run on
        self._done = []              # [lo, hi) ranges already updated in the current step
        self._grad_scale = 1.0
        self._plan_step = None       # the step number the plan below was made for
        self._key = None             # settings the uploaded table was built from
        self._segs = None            # (host ctypes array, device tensor, nseg) or None: the plain mmvqa_adam path
        self._uploaded = None        # event behind the last upload: launches on other streams wait for it
        self._retired = []           # the table before this one: a launch still queued may read it
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.ema = None if ema_decay is None else model.flat_params.detach().clone()
        self.ema_updates = 0         # steps the average has taken (skipped steps not counted): the warm-up's t
        self._averaged = False       # inside averaged(): flat_params holds the average, self.ema the live weights

    # ------------------------------------------------------------------ segment table
    def group_spec(self):
        """what has to agree between a checkpoint and the optimizer that resumes from it: the form of the weight decay
        and the parameter names of every group"""
        names = [[] for _ in self.param_groups]
        for n, g in zip(self._names, self._group_of):
            names[g].append(n)
        return dict(decoupled=self.decoupled, groups=names)

    def segments(self):
        """the merged table [(lo, hi, lr, weight_decay, mode)] of the current settings"""
        mode = L.ADAM_DECOUPLED if self.decoupled else L.ADAM_L2
        rows = []
        for (name, p, lo, hi), gi in zip(self._ranges, self._group_of):
            g = self.param_groups[gi]
            rows.append((lo, hi, float(g["lr"]), float(g["weight_decay"]), mode if p is None or p.requires_grad else L.ADAM_FROZEN))
        return merge_segments(rows)

    def _plan(self, step):
        """once per step: read the groups' settings and the parameters' requires_grad; build and upload the table when
        they differ from what the device holds"""
        if self._plan_step == step:
            return
        self._plan_step = step
        b0, e0 = self.param_groups[0]["betas"], self.param_groups[0]["eps"]
        if any(tuple(g["betas"]) != tuple(b0) or g["eps"] != e0 for g in self.param_groups):
            raise L.MMVQAError("FusedAdam: betas and eps are shared by all groups; per-group values are not supported")
        trained = tuple(map(_REQUIRES_GRAD, self._params))
        key = (tuple((float(g["lr"]), float(g["weight_decay"])) for g in self.param_groups), trained)
        if key == self._key:
            return
        self._key = key
        if len(self.param_groups) == 1 and key[0][0][1] == 0.0 and all(trained):
            self._segs = None        # one group, no decay, nothing frozen: mmvqa_adam, as always
            return
        segs = self.segments()
        host = (L.AdamSeg * len(segs))()
        for h, (lo, hi, lr, wd, mode) in zip(host, segs):
            h.begin, h.end, h.lr, h.weight_decay, h.mode = lo, hi, lr, wd, mode
        staged = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).pin_memory()
        dev = torch.empty(staged.numel(), dtype=torch.uint8, device=self.m.device)
        dev.copy_(staged, non_blocking=True)   # (pinned source: the copy is queued, nothing waits for the device)
        self._uploaded = torch.cuda.Event()
        self._uploaded.record()
        self._retired = [self._segs]           # a fresh buffer per upload: a queued launch keeps reading its own table
        self._segs = (host, dev, len(segs))

    # ------------------------------------------------------------------ update beside the backward pass
    def overlap_backward(self, reducer=None, grad_scale=1.0):
        """Update a parameter range as soon as its gradient is final instead of after the whole backward pass.
        Single process: the model's gradient-ready announcements (Model.set_grad_ready_hook) start the range's Adam on a
        stream of its own, ordered behind the announcement's event.  With a ddp.GradReducer that exchanges gradients
        (world > 1 or the native RCCL route) the reducer owns the hook and calls back per bucket: the update is ordered
        behind that bucket's all-reduce (work.wait() puts the wait on the update's stream, not on the host).
        step() then only updates what was never announced and joins the streams.  The arithmetic per element is the same
        kernel with the same step number: results are bit-identical to the one-launch form (tests/test_hip_train.py).
        With groups, weight decay or frozen parameters every ranged launch reads the one global table with its own
        [lo, hi).
        Contract: ONE backward per step (no gradient accumulation), zero_grad=True and this grad_scale in step()."""
        self._stream = torch.cuda.Stream()
        self._grad_scale = float(grad_scale)
        self._done = []
        if reducer is not None and reducer.exchanges():
            reducer.after_bucket = self._after_bucket
        else:
            self.model.set_grad_ready_hook(self._on_ready, with_event=True)

    def _adam(self, lo, hi, step, grad_scale, zero_grad, stream_ptr):
        if self._averaged:
            raise L.MMVQAError("FusedAdam: an update inside averaged() would train the averaged weights; leave the context first")
        self._plan(step)
        g = self.param_groups[0]
        p = self.model.flat_params
        # the averaging forms take the step's decay by value: ema_updates moves at the end of step(), so every ranged
        # launch of one step gets the same one
        ema = self.ema is not None
        decay = (ema_decay_at(self.ema_decay, self.ema_updates, self.ema_warmup),) if ema else ()
        if self._segs is None:
            fn = L.lib().mmvqa_adam_ema if ema else L.lib().mmvqa_adam
            avg = (L.ptr(self.ema[lo:hi]),) if ema else ()
            L.check(fn(stream_ptr, L.ptr(p[lo:hi]), L.ptr(self.model.flat_grads[lo:hi]), L.ptr(self.m[lo:hi]),
                       L.ptr(self.v[lo:hi]), *avg, hi - lo, g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                       step, grad_scale, 1 if zero_grad else 0, *decay))
            return
        host, dev, nseg = self._segs
        torch.cuda.current_stream().wait_event(self._uploaded)   # (a no-op on the stream that uploaded)
        fn = L.lib().mmvqa_adam_groups_ema if ema else L.lib().mmvqa_adam_groups
        avg = (L.ptr(self.ema),) if ema else ()
        L.check(fn(stream_ptr, L.ptr(p), L.ptr(self.model.flat_grads), L.ptr(self.m), L.ptr(self.v), *avg,
                   lo, hi - lo, C.cast(host, C.c_void_p), L.ptr(dev), nseg, g["betas"][0],
                   g["betas"][1], g["eps"], step, grad_scale, 1 if zero_grad else 0, *decay))

    def _early(self, lo, hi, ready=None, work=None, stream=None):
        if hi <= lo or any(a < hi and lo < b for a, b in self._done):
            return   # (a second backward before step(): this range already moved in this step)
        s = stream if stream is not None else self._stream
        if ready is not None:
            s.wait_event(ready)
        with torch.cuda.stream(s):
            if work is not None:
                work.wait()
            self._adam(lo, hi, self.step_count + 1, self._grad_scale, True, L.stream_ptr())
        if stream is not None:
            self._stream.wait_stream(stream)   # step() joins ONE stream
        self._done.append((lo, hi))

    def _on_ready(self, lo, hi, ready):
        self._early(lo, hi, ready=ready)

    def _after_bucket(self, lo, hi, work=None, stream=None):
        self._early(lo, hi, work=work, stream=stream)

    def zero_grad(self, set_to_none=False):
        self.model.flat_grads.zero_()

    def step(self, grad_scale=1.0, zero_grad=True):
        """p -= lr * m_hat / (sqrt(v_hat) + eps); grads are multiplied by grad_scale first
        (1/world_size under DDP) and zeroed in the same pass when zero_grad is set."""
        if self.model.flat_params.data_ptr() != self._for:
            raise L.MMVQAError("FusedAdam: the model was re-laid out (.to()/re-head) after the optimizer was built")
        if self._averaged:
            raise L.MMVQAError("FusedAdam.step inside averaged(): the model holds the averaged weights; leave the context first")
        self.step_count += 1
        n = self.model.flat_params.numel()
        if not self._done:
            self._adam(0, n, self.step_count, grad_scale, zero_grad, L.stream_ptr())
            self.ema_updates += 1 if self.ema is not None else 0
            return
        if not zero_grad or abs(grad_scale - self._grad_scale) > 1e-12 * abs(self._grad_scale):
            raise L.MMVQAError("FusedAdam.step: ranges were already updated during backward with zero_grad=True and "
                               f"grad_scale={self._grad_scale}; step(grad_scale={grad_scale}, zero_grad={zero_grad}) does not match")
        pos = 0
        for lo, hi in sorted(self._done):      # whatever backward never announced
            if lo > pos:
                self._adam(pos, lo, self.step_count, grad_scale, True, L.stream_ptr())
            pos = max(pos, hi)
        if pos < n:
            self._adam(pos, n, self.step_count, grad_scale, True, L.stream_ptr())
        torch.cuda.current_stream().wait_stream(self._stream)   # the next forward reads the updated parameters
        self._done = []
        self.ema_updates += 1 if self.ema is not None else 0

    # ------------------------------------------------------------------ the averaged weights
    def _swap(self):
        p = self.model.flat_params
        L.check(L.lib().mmvqa_swap(L.stream_ptr(), L.ptr(p), L.ptr(self.ema), p.numel()))

    def averaged(self):
        """with opt.averaged(): the model computes with the averaged weights.  The contents of model.flat_params and
        self.ema are exchanged by one launch on the current stream (the engine stays bound to the same pointers, every
        parameter view stays valid) and exchanged back on exit, also on an exception; step() inside raises.  Buffers are
        not averaged: the averaged weights run with the live BatchNorm statistics (see __init__).  Without ema_decay
        this is a null context."""
        if self.ema is None:
            return contextlib.nullcontext()
        return self._averaged_weights()

    @contextlib.contextmanager
    def _averaged_weights(self):
        if self._averaged:
            raise L.MMVQAError("FusedAdam.averaged() is already active")
        if self._done:
            raise L.MMVQAError("FusedAdam.averaged() between a backward pass whose ranges were already updated and its step()")
        self._swap()
        self._averaged = True
        try:
            yield self
        finally:
            self._swap()
            self._averaged = False

    def state_dict(self):
        sd = dict(m=self.m, v=self.v, step=self.step_count, param_groups=self.param_groups, group_spec=self.group_spec())
        if self.ema is not None:
            if self._averaged:
                raise L.MMVQAError("FusedAdam.state_dict inside averaged(): self.ema holds the live weights there")
            sd.update(ema=self.ema, ema_decay=self.ema_decay, ema_warmup=self.ema_warmup, ema_updates=self.ema_updates)
        return sd

    def load_state_dict(self, sd):
        mine = self.group_spec()
        theirs = sd.get("group_spec")
        if theirs is None:           # written before there were groups: one group over everything, no weight decay
            theirs = dict(decoupled=self.decoupled, groups=[list(self._names)])
        if theirs != mine:
            raise L.MMVQAError("FusedAdam.load_state_dict: the checkpoint's optimizer groups (which tensors belong to which "
                               "group, or the form of the weight decay) differ from this optimizer's; build it with the "
                               "groups the checkpoint was written with")
        self.m.copy_(sd["m"]); self.v.copy_(sd["v"])
        self.step_count = int(sd["step"])
        # in place: a scheduler built on this optimizer keeps pointing at the SAME list/dicts, so a later
        # ReduceLROnPlateau step still reaches the kernel after --resume
        for mine_g, theirs_g in zip(self.param_groups, sd["param_groups"]):
            mine_g.update(theirs_g)
        self._plan_step = None
        if self.ema is None:         # a plain optimizer ignores a checkpoint's average
            return
        if "ema" in sd:
            self.ema.copy_(sd["ema"])
            self.ema_decay, self.ema_warmup = float(sd["ema_decay"]), bool(sd["ema_warmup"])
            self.ema_updates = int(sd["ema_updates"])
        else:
            self.ema.copy_(self.model.flat_params)
            self.ema_updates = 0
            print("FusedAdam: the checkpoint holds no weight average; it starts from the current parameters", flush=True)
