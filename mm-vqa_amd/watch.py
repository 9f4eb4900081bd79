"""A per-tensor view of a training run: what ``wandb.watch(model, log='all')`` gives the reference's two scripts
(pretrain/roco_train.py:80, vqamed2019/train.py:157) -- a 64-bin histogram of every parameter tensor and of its gradient
every ``log_freq`` steps -- plus counts of non-finite values, exact extrema and fp64 sums, written to a JSON-lines file.

Every parameter and every gradient lives in one flat fp32 buffer with a name table, so the statistics of all tensors are
one call of ``mmvqa_tensor_stats`` per buffer: at most three launches whatever the number of tensors (DESIGN.md section
23), where the hook behind ``wandb.watch`` runs min, max, histc and a host read per tensor.

``TensorStats(model)`` owns the segment table on the device, the workspace and a pool of record buffers with pinned host
mirrors.  ``grads()`` / ``params()`` enqueue the launches and a device-to-host copy on the current stream and return a
handle; nothing waits.  ``Watcher`` is the loop-side object of ``train.py --watch``: it decides which steps are logged,
collects finished handles at the start of later steps and writes one line per logged step.
"""
from __future__ import annotations

import atexit
import ctypes as C
import json
import math
import os

import numpy as np
import torch

from . import _lib as L

RECORD = np.dtype([("sum", "<f8"), ("sumsq", "<f8"), ("n_finite", "<i8"), ("n_nan", "<i8"), ("n_posinf", "<i8"),
                   ("n_neginf", "<i8"), ("n_zero", "<i8"), ("min", "<f4"), ("max", "<f4"),
                   ("hist", "<u4", (L.TENSOR_HIST_BINS,))])
assert RECORD.itemsize == C.sizeof(L.TensorStat)
COUNTS = ("n_finite", "n_nan", "n_posinf", "n_neginf", "n_zero")


def segment_table(rows):
    """[(offset, numel)] ascending -> (host table with chunk0 filled, workspace bytes); raises when it is refused"""
    host = (L.StatSeg * len(rows))()
    for h, (off, n) in zip(host, rows):
        h.offset, h.numel = int(off), int(n)
    ws = L.lib().mmvqa_tensor_stats_workspace(C.cast(host, C.c_void_p), len(rows))
    if ws == 0:
        msg = L.lib().mmvqa_last_error()
        raise L.MMVQAError(f"mmvqa error {L.ERR_ARG}: {msg.decode() if msg else '?'}")
    return host, int(ws)


class Handle:
    """the records of one call, on their way to the host"""

    def __init__(self, owner, names, bufs, event, moments_only):
        self._owner, self._names, self._bufs, self._event = owner, names, bufs, event
        self.moments_only = moments_only
        self._out = None

    def ready(self):
        return self._out is not None or self._event.query()

    def result(self):
        """{name: record}; record = dict of the counts (int), min, max, sum, sumsq (float) and hist (uint32 [64] array, or
        None for a moments-only call).  Waits for the copy when it has not arrived."""
        if self._out is None:
            self._event.synchronize()
            rec = np.frombuffer(self._bufs[1].numpy(), dtype=RECORD).copy()
            self._owner._give_back(self._bufs)       # the buffers serve the next call
            self._bufs = None
            out = {}
            for name, r in zip(self._names, rec):
                d = {k: int(r[k]) for k in COUNTS}
                d.update(min=float(r["min"]), max=float(r["max"]), sum=float(r["sum"]), sumsq=float(r["sumsq"]),
                         hist=None if self.moments_only else r["hist"].copy())
                out[name] = d
            self._out = out
        return self._out


class TensorStats:
    def __init__(self, model):
        """model: a mmvqa_amd.Model, or anything with flat_params / flat_grads (one unnamed tensor, as FusedAdam takes it)"""
        self.model = model
        self._for = None
        self._pool = []
        self._sync_layout()

    def _layout_key(self):
        return (self.model.flat_params.data_ptr(), id(getattr(self.model, "_table", None)))

    def _sync_layout(self):
        """(re)build and upload the table when the model was re-laid out (.to(), classifier[2] surgery)"""
        key = self._layout_key()
        if key == self._for:
            return
        self._for = key
        table = getattr(self.model, "_param_ranges", None)
        if table is not None:
            rows = [(name, p, lo, p.numel()) for name, p, lo, _hi in table()]
        else:
            rows = [("", None, 0, self.model.flat_params.numel())]
        self.names = [r[0] for r in rows]
        self.tensors = [r[1] for r in rows]      # the Parameters (None for the unnamed tensor)
        self.numel = [r[3] for r in rows]
        self._host, ws_bytes = segment_table([(r[2], r[3]) for r in rows])
        dev = self.model.flat_params.device
        staged = torch.frombuffer(bytearray(bytes(self._host)), dtype=torch.uint8).pin_memory()
        self._dev = torch.empty(staged.numel(), dtype=torch.uint8, device=dev)
        self._dev.copy_(staged, non_blocking=True)
        self._staged = staged                     # (alive until the copy has run)
        self._ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
        self._pool = []

    def _buffers(self):
        if self._pool:
            return self._pool.pop()
        nbytes = len(self.names) * RECORD.itemsize
        return (torch.zeros(nbytes, dtype=torch.uint8, device=self._dev.device),
                torch.zeros(nbytes, dtype=torch.uint8).pin_memory())

    def _give_back(self, bufs):
        if bufs[1].numel() == len(self.names) * RECORD.itemsize and bufs[0].device == self._dev.device:
            self._pool.append(bufs)

    def _run(self, flat, moments_only):
        self._sync_layout()
        bufs = self._buffers()
        L.check(L.lib().mmvqa_tensor_stats(L.stream_ptr(), L.ptr(flat), flat.numel(), C.cast(self._host, C.c_void_p),
                                           L.ptr(self._dev), len(self.names), L.ptr(bufs[0]), L.ptr(self._ws),
                                           self._ws.numel(), L.TENSOR_STATS_MOMENTS_ONLY if moments_only else 0))
        bufs[1].copy_(bufs[0], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return Handle(self, self.names, bufs, ev, moments_only)

    def grads(self, moments_only=False):
        """statistics of the flat gradient buffer by tensor (a tensor without a gradient reads as the zeros it holds)"""
        return self._run(self.model.flat_grads, moments_only)

    def params(self, moments_only=False):
        return self._run(self.model.flat_params, moments_only)


# ------------------------------------------------------------------------------------------------- the JSON lines
def _num(x):
    return x if math.isfinite(x) else None


def record_json(r):
    """a record as the line holds it: the counts, sum, sumsq, edges = [min, max] (null without a finite value) and the
    histogram as 64 ints (absent for a moments-only record)"""
    d = {k: r[k] for k in COUNTS}
    d.update(sum=_num(r["sum"]), sumsq=_num(r["sumsq"]), edges=[_num(r["min"]), _num(r["max"])])
    if r["hist"] is not None:
        d["hist"] = [int(v) for v in r["hist"]]
    return d


def step_line(step, epoch, loop, grad_scale, loss_scale, names, numel, frozen, grad=None, param=None):
    """the line of a logged step; grad / param: {name: record} or None"""
    tensors = {}
    for name, n, fz in zip(names, numel, frozen):
        t = {"numel": int(n)}
        if fz:
            t["frozen"] = True
        if grad is not None and not fz:
            t["grad"] = record_json(grad[name])
        if param is not None:
            t["param"] = record_json(param[name])
        tensors[name] = t
    return json.dumps(dict(step=step, epoch=epoch, loop=loop, grad_scale=grad_scale, loss_scale=loss_scale, tensors=tensors),
                      allow_nan=False)


def skipped_line(step, epoch, loop, loss_scale, grad):
    """the line of a step the loss scaler skipped: the tensors that hold a non-finite gradient, in buffer order"""
    bad = {name: [r["n_nan"], r["n_posinf"], r["n_neginf"]] for name, r in grad.items()
           if r["n_nan"] or r["n_posinf"] or r["n_neginf"]}
    return json.dumps(dict(step=step, epoch=epoch, loop=loop, loss_scale=loss_scale, skipped=True, nonfinite=bad),
                      allow_nan=False)


class Watcher:
    """train.py --watch: statistics of the gradients Adam is about to consume and / or of the parameters before the
    update, every `freq`-th step (steps count from 1 over the whole run), one JSON line each in `path`.  A logged step
    enqueues and returns; its line is written once the records have arrived, which poll() checks at the start of later
    steps and flush() waits for (end of an epoch, exit)."""

    def __init__(self, model, what, freq, path, loop):
        if what not in ("gradients", "parameters", "all"):
            raise ValueError(f"watch: {what!r} is none of gradients, parameters, all")
        if freq < 1:
            raise ValueError(f"watch: freq={freq} must be at least 1")
        self.stats = TensorStats(model)
        self.what, self.freq, self.path, self.loop = what, int(freq), path, loop
        self.step, self.epoch = 0, 0
        self._pending = []
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        self._file = open(path, "a")
        atexit.register(self.close)              # a run that ends early still writes what it has enqueued

    @property
    def wants_grads(self):
        return self.what in ("gradients", "all")

    def begin_step(self):
        """count the step, write what has arrived -> whether this step is logged"""
        self.step += 1
        self.poll()
        return self.step % self.freq == 0

    def log(self, grad_scale, loss_scale=None):
        """enqueue the statistics of this step (between the gradient all-reduce and the optimizer step)"""
        st = self.stats
        g = st.grads() if self.wants_grads else None
        p = st.params() if self.what in ("parameters", "all") else None
        frozen = [q is not None and not q.requires_grad for q in st.tensors]
        self._pending.append(dict(step=self.step, epoch=self.epoch, grad_scale=float(grad_scale), loss_scale=loss_scale,
                                  grad=g, param=p, frozen=frozen, names=list(st.names), numel=list(st.numel)))

    def set_loss_scale(self, loss_scale):
        """the loss scale of this step, known to the host once the scaler has made its decision"""
        if self._pending and self._pending[-1]["step"] == self.step:
            self._pending[-1]["loss_scale"] = loss_scale

    def log_skipped(self, loss_scale=None):
        """the loss scaler skipped this step: which tensors hold the non-finite gradients (moments only)"""
        self._pending.append(dict(step=self.step, epoch=self.epoch, loss_scale=loss_scale, skipped=self.stats.grads(True)))

    def _write(self, e):
        if "skipped" in e:
            grad = e["skipped"].result()
            self._file.write(skipped_line(e["step"], e["epoch"], self.loop, e["loss_scale"], grad) + "\n")
            first = next((n for n, r in grad.items() if r["n_nan"] or r["n_posinf"] or r["n_neginf"]), None)
            if first is not None:
                r = grad[first]
                print(f"step {e['step']} skipped: the gradient of {first or 'the flat buffer'} holds {r['n_nan']} nan, "
                      f"{r['n_posinf']} +inf and {r['n_neginf']} -inf values", flush=True)
            return
        grad = e["grad"].result() if e["grad"] is not None else None
        param = e["param"].result() if e["param"] is not None else None
        self._file.write(step_line(e["step"], e["epoch"], self.loop, e["grad_scale"], e["loss_scale"], e["names"],
                                   e["numel"], e["frozen"], grad, param) + "\n")

    @staticmethod
    def _ready(e):
        return all(h.ready() for h in (e.get("grad"), e.get("param"), e.get("skipped")) if h is not None)

    def poll(self):
        """write the lines whose records have arrived, in step order; waits for nothing"""
        while self._pending and self._ready(self._pending[0]):
            self._write(self._pending.pop(0))

    def flush(self):
        while self._pending:
            self._write(self._pending.pop(0))
        self._file.flush()

    def close(self):
        if self._file is not None:
            self.flush()
            self._file.close()
            self._file = None
