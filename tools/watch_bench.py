#!/usr/bin/env python3
"""What --watch costs on the config-2 model (bench.py's flagship: ResNet-152 + BERT-style encoder, 16 x 224^2 images,
T 32), after one real backward, all forms alternating on the same device, RUNS timed repetitions each.  Writes
profiles/watch_cfg2.json (or argv[1]).

  (a) fused      mmvqa_tensor_stats over the gradients and over the parameters (watch.TensorStats: 3 + 3 launches)
  (b) per_tensor what the reference's wandb.watch hook amounts to: min, max, torch.histc(bins=64) and one host read per
                 tensor, over the same tensors of both buffers
  (c) read_pass  mmvqa_amp_unscale with mul = 0 over the gradient buffer: one plain read of one buffer, the yardstick
  (d) step       train.mlm_step on a synthetic batch with a Watcher (--watch all --watch_freq 1) against none
  (e) histogram forms: one call over one 32 M-float tensor of N(0, 1e-4) with two outliers (what gradients look like:
                 nearly everything in 4 bins) and over uniform data (every bin equally likely), and one call over the
                 real gradients, with the ballot-aggregated histogram pass and with the form that issues one LDS atomic
                 per element (MMVQA_TENSOR_STATS_PEEL=0)

(a) reads each buffer twice (moments pass, histogram pass): bytes = 2 buffers x 2 reads x 4 n.  Device times are HIP
events around the enqueued work; (b) and (d) are host wall time around a synchronised region, because their cost is the
host's."""
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd import synth  # noqa: E402
from mmvqa_amd import train as TR  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from mmvqa_amd.watch import TensorStats, Watcher  # noqa: E402

RUNS, STEPS = int(os.environ.get("WATCH_BENCH_RUNS", "5")), int(os.environ.get("WATCH_BENCH_STEPS", "5"))


def device_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def enqueue_ms(call):
    """device time of what call() enqueues; its handles are read afterwards, so their buffers return to the pool"""
    hs = []

    def run():
        h = call()
        hs.extend(h if isinstance(h, tuple) else (h,))
    t = device_ms(run)
    for h in hs:
        h.result()
    return t


def median(v):
    return sorted(v)[len(v) // 2]


class Flat:
    def __init__(self, x):
        self.flat_params, self.flat_grads = x, x


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "watch_cfg2.json")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1234)
    model = mmvqa_amd.Model(bench.make_args()).to(dev).train()
    model.set_seed(1234)
    opt = mmvqa_amd.FusedAdam(model, lr=2e-5)
    red = GradReducer(model.flat_grads)
    batch = synth.roco_batch(bench.B_PER_GPU, bench.T, bench.HW, bench.VOCAB, seed=1234, device=dev)
    model.tune(*batch[:4])
    for _ in range(2):
        TR.mlm_step(model, opt, red, 1, batch)
    opt.zero_grad()
    mmvqa_amd.mlm_loss(model(*batch[:4]), batch[4])[0].backward()      # one real backward: the gradients measured below
    torch.cuda.synchronize()

    ts = TensorStats(model)
    n = model.flat_params.numel()
    views = [(model.flat_grads[lo:lo + p.numel()], model.flat_params[lo:lo + p.numel()]) for _, p, lo, _ in model._param_ranges()]
    found = torch.zeros(1, device=dev)

    def fused():
        hg, hp = ts.grads(), ts.params()
        return hg, hp

    def fused_and_read():
        hg, hp = fused()
        hg.result(), hp.result()

    def per_tensor():
        for pair in views:
            for t in pair:
                lo, hi = float(t.min()), float(t.max())            # (histc needs the range on the host)
                torch.histc(t, bins=64, min=lo, max=hi).cpu()

    def read_pass():
        L.check(L.lib().mmvqa_amp_unscale(L.stream_ptr(), L.ptr(model.flat_grads), n, None, L.ptr(found), 0))

    for f in (fused_and_read, per_tensor, read_pass):
        f()
    torch.cuda.synchronize()
    ms = {"fused_device": [], "fused_with_read_host": [], "per_tensor_host": [], "read_pass_device": []}
    for _ in range(RUNS):
        ms["fused_device"].append(enqueue_ms(fused))
        torch.cuda.synchronize()
        ms["fused_with_read_host"].append(host_ms(fused_and_read))
        ms["per_tensor_host"].append(host_ms(per_tensor))
        ms["read_pass_device"].append(device_ms(read_pass))
        torch.cuda.synchronize()

    # the two histogram forms on the real gradients: one call over the gradient buffer each
    real = {}
    for key, env in (("ballot", None), ("atomic_per_element", "0")):
        if env is not None:
            os.environ["MMVQA_TENSOR_STATS_PEEL"] = env
        real[key] = median([enqueue_ms(ts.grads) for _ in range(RUNS)])
        os.environ.pop("MMVQA_TENSOR_STATS_PEEL", None)
    real["moments_only"] = median([enqueue_ms(lambda: ts.grads(moments_only=True)) for _ in range(RUNS)])

    # (d) the step with and without the watcher
    tmp = tempfile.mkdtemp()
    watch = Watcher(model, "all", 1, os.path.join(tmp, "watch_mlm.jsonl"), "mlm")
    step_ms = {"plain": [], "watched": []}
    for w in (None, watch):
        TR.mlm_step(model, opt, red, 1, batch, watch=w)
    for _ in range(RUNS):
        for key, w in (("plain", None), ("watched", watch)):
            def steps():
                for _ in range(STEPS):
                    TR.mlm_step(model, opt, red, 1, batch, watch=w)
            step_ms[key].append(host_ms(steps) / STEPS)
    watch.close()

    # (e) the histogram pass on concentrated and on uniform data, one tensor of 32 M floats
    m = 32 * 2 ** 20
    g = torch.Generator(device=dev).manual_seed(7)
    conc = torch.randn(m, device=dev, generator=g) * 1e-4
    conc[12345], conc[m - 6789] = 0.05, -0.05
    unif = torch.rand(m, device=dev, generator=g)
    forms = {}
    for name, x in (("concentrated", conc), ("uniform", unif)):
        st = TensorStats(Flat(x))
        rec = st.params().result()[""]
        full = [enqueue_ms(st.params) for _ in range(RUNS)]
        mom = [enqueue_ms(lambda: st.params(moments_only=True)) for _ in range(RUNS)]
        os.environ["MMVQA_TENSOR_STATS_PEEL"] = "0"       # the form with one LDS atomic per element, for comparison
        same = bool((st.params().result()[""]["hist"] == rec["hist"]).all())
        plain = [enqueue_ms(st.params) for _ in range(RUNS)]
        del os.environ["MMVQA_TENSOR_STATS_PEEL"]
        f, mo, pl = median(full), median(mom), median(plain)
        forms[name] = {"floats": m, "nonzero_bins": int((rec["hist"] > 0).sum()), "full_ms": f, "moments_only_ms": mo,
                       "histogram_pass_ms": f - mo, "atomic_per_element_full_ms": pl,
                       "atomic_per_element_histogram_pass_ms": pl - mo, "same_counts": same}

    med = {k: median(v) for k, v in ms.items()}
    fused_bytes, pass_bytes = 2 * 2 * 4 * n, 4 * n
    res = {
        "config": 2, "runs": RUNS, "tensors": len(views), "floats_per_buffer": n,
        "ms": ms, "median_ms": med,
        "fused": {"launches": 6, "bytes_read": fused_bytes, "GBps": fused_bytes / (med["fused_device"] * 1e-3) / 1e9},
        "read_pass": {"bytes_read": pass_bytes, "GBps": pass_bytes / (med["read_pass_device"] * 1e-3) / 1e9},
        "fused_over_four_read_passes": med["fused_device"] / (4 * med["read_pass_device"]),
        "per_tensor_over_fused": med["per_tensor_host"] / med["fused_with_read_host"],
        "step_ms": step_ms, "step_median_ms": {k: median(v) for k, v in step_ms.items()},
        "steps_per_run": STEPS, "histogram_forms_of_data": forms, "gradients_call_ms": real,
    }
    res["step_overhead_ms"] = res["step_median_ms"]["watched"] - res["step_median_ms"]["plain"]
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
