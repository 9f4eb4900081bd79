"""One case of tests/test_hip_schedule.py in a process of its own.

The engine's schedule switches (MMVQA_TAP_STREAM_OFF, MMVQA_TAP_FIRST, MMVQA_ENC_SIDE_OFF, MMVQA_SIDE_PRIO_OFF,
MMVQA_NO_SIDE_STREAM) and the lag injection (MMVQA_SIDE_LAG_US, MMVQA_MAIN_LAG_US) are read once per process, so each
variant runs here under the environment the parent test gives it.  Usage: schedule_child.py CASE.pt RESULT.json.

CASE.pt (torch.save of a dict, written by the parent):
  mode    "values" | "finality" | "adam"
  args    the Model(args) fields;  kind  "mlm" | "supcon" | "vqa";  B
  state   state_dict to load, or None: seeded initialisation (torch.manual_seed(seed); Model(args))
  inputs  list of (img, ids, seg, mask, tgt) on the CPU;  tune  run Model.tune() on inputs[0] first
  check   (values) the oracle's results: logits / feat / loss, per-parameter gradient truth, running statistics
RESULT.json: what was measured (relative errors, announced ranges, mismatches) -- the parent asserts -- or
{"error": ..., "gpu": bool} when the case raised.
"""
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import mmvqa_amd  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402

NEG_ZERO = -(2 ** 31)   # bit pattern of -0.0 as int32


def relerr(a, b):   # (tests/hip_helpers.py: relative to the reference's largest magnitude)
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def make_model(case, dev):
    if case["state"] is None:
        torch.manual_seed(case["seed"])
        m = mmvqa_amd.Model(O.make_args(**case["args"]))
    else:
        m = mmvqa_amd.Model(O.make_args(**case["args"]))
        m.load_state_dict(case["state"])
    m.to(dev).train()
    return m


def loss_of(kind, out, tgt, B):
    if kind == "vqa":
        return out[0], None, mmvqa_amd.asl_loss(out[0], tgt)
    if kind == "supcon":
        logits, feat = out
        return logits, feat, mmvqa_amd.mlm_loss(logits, tgt)[0] + mmvqa_amd.supcon_loss(mmvqa_amd.split_feat(feat, B // 2))
    return out, None, mmvqa_amd.mlm_loss(out, tgt)[0]


def step(case, m, batch):
    img, ids, seg, mask, tgt = batch
    logits, feat, loss = loss_of(case["kind"], m(img, ids, seg, mask), tgt, case["B"])
    loss.backward()
    return logits, feat, loss


def run_values(case, dev, batches):
    """forward, loss, backward, BatchNorm running statistics: relative errors against the oracle's truth"""
    m = make_model(case, dev)
    if case["tune"]:
        m.tune(*batches[0][:4])
    logits, feat, loss = step(case, m, batches[0])
    torch.cuda.synchronize()
    chk = case["check"]
    res = {"logits": relerr(logits, chk["logits"]), "loss": float(loss), "feat": None, "grads": {}, "no_grad": {},
           "stats": {}, "nbt": {}}
    if feat is not None:
        res["feat"] = relerr(feat, chk["feat"])
    hp = dict(m.named_parameters())
    for name, truth in chk["grads"].items():
        g = hp[name].grad
        res["grads"][name] = None if g is None else relerr(g, truth)
    for name in chk["no_grad"]:
        g = hp[name].grad
        res["no_grad"][name] = 0.0 if g is None else float(g.abs().max())
    hsd = m.state_dict()
    for k, v in chk["stats"].items():
        res["stats"][k] = relerr(hsd[k], v)
    for k in chk["nbt"]:
        res["nbt"][k] = int(hsd[k])
    return res


def run_finality(case, dev, batches):
    """Announcement finality.  Pass 1: a stream that waits only on an announcement's `ready` event snapshots the range;
    every snapshot must be bit-equal to the range's final contents.  Pass 2: that stream overwrites the range with -0.0
    instead; a writer that lands after the announcement leaves something other than -0.0 (an atomic add of g gives g,
    of +0.0 gives +0.0; NaN would hide atomic adds)."""
    m = make_model(case, dev)
    batch = batches[0]
    if case["tune"]:
        m.tune(*batch[:4])
    step(case, m, batch)   # warm-up: streams, events and workspaces exist
    torch.cuda.synchronize()
    third = torch.cuda.Stream()
    fg = m.flat_grads
    n = fg.numel()
    res = {"n": n}

    def one_pass(poison):
        seen = []

        def hook(lo, hi, ready):
            with torch.cuda.stream(third):
                third.wait_event(ready)
                if poison:
                    fg[lo:hi].view(torch.int32).fill_(NEG_ZERO)
                    seen.append((lo, hi, None))
                else:
                    seen.append((lo, hi, fg[lo:hi].clone()))

        fg.zero_()
        m.set_grad_ready_hook(hook, with_event=True)
        try:
            step(case, m, batch)
            torch.cuda.synchronize()
        finally:
            m.set_grad_ready_hook(None)
        return seen

    seen = one_pass(False)
    res["ranges"] = [(lo, hi) for lo, hi, _ in seen]
    bad = []
    for lo, hi, snap in seen:
        fin = fg[lo:hi]
        if not torch.equal(snap.view(torch.int32), fin.view(torch.int32)):
            d = (snap - fin).abs()
            bad.append((lo, hi, int((snap.view(torch.int32) != fin.view(torch.int32)).sum()), float(d.max()),
                        float(fin.abs().max())))
    res["snapshot_mismatch"] = bad
    del seen
    seen = one_pass(True)
    res["poison_ranges"] = [(lo, hi) for lo, hi, _ in seen]
    bad = []
    for lo, hi, _ in seen:
        k = int((fg[lo:hi].view(torch.int32) != NEG_ZERO).sum())
        if k:
            bad.append((lo, hi, k))
    res["poison_overwritten"] = bad
    fg.zero_()
    return res


def run_adam(case, dev, batches):
    """FusedAdam.overlap_backward() on model b: per step, the gradients each ranged update reads are copied on the update's
    stream right before it; the one-launch optimizer (model a) applied to the same starting point and to those gradients
    must land on b's parameters and moments bit for bit, and step() must leave no gradient behind (a late atomic add
    after the early update zeroed its range would)"""
    lr = case["lr"]
    b = make_model(case, dev)
    a = mmvqa_amd.Model(O.make_args(**case["args"]))
    a.load_state_dict(b.state_dict())
    a.to(dev).train()
    if case["tune"]:
        b.tune(*batches[0][:4])
    opt_a, opt_b = mmvqa_amd.FusedAdam(a, lr=lr), mmvqa_amd.FusedAdam(b, lr=lr)
    opt_b.overlap_backward()
    seen = []
    early = opt_b._early

    def early_copy(lo, hi, ready=None, work=None, stream=None):
        s = opt_b._stream
        if ready is not None:
            s.wait_event(ready)
        with torch.cuda.stream(s):
            seen.append((lo, hi, b.flat_grads[lo:hi].clone()))
        early(lo, hi, ready=ready, work=work, stream=stream)

    opt_b._early = early_copy
    n = b.flat_params.numel()
    res = {"n": n, "done": [], "grads_left": [], "same": []}
    for batch in batches:
        torch.cuda.synchronize()
        p0, m0, v0, s0 = b.flat_params.clone(), opt_b.m.clone(), opt_b.v.clone(), opt_b.step_count
        seen.clear()
        opt_b.zero_grad()
        step(case, b, batch)
        res["done"].append(sorted(opt_b._done))
        opt_b.step()
        torch.cuda.synchronize()
        res["grads_left"].append(float(b.flat_grads.abs().max()))
        g = torch.zeros_like(b.flat_grads)
        for lo, hi, snap in seen:
            g[lo:hi] = snap
        a.flat_params.copy_(p0)
        opt_a.m.copy_(m0)
        opt_a.v.copy_(v0)
        opt_a.step_count = s0
        a.flat_grads.copy_(g)
        opt_a.step()
        torch.cuda.synchronize()
        res["same"].append([torch.equal(a.flat_params, b.flat_params), torch.equal(opt_a.m, opt_b.m),
                            torch.equal(opt_a.v, opt_b.v)])
        del p0, m0, v0, g
    return res


def main():
    case_path, out_path = sys.argv[1], sys.argv[2]
    try:
        case = torch.load(case_path, weights_only=False)
        dev = torch.device("cuda:0")
        batches = [tuple(t.to(dev) for t in b) for b in case["inputs"]]
        res = {"values": run_values, "finality": run_finality, "adam": run_adam}[case["mode"]](case, dev, batches)
        torch.cuda.synchronize()
    except BaseException as ex:   # reported to the parent, which fails the test (and stops the module on a GPU error)
        msg = "".join(traceback.format_exception(ex))
        low = str(ex).lower()
        res = {"error": msg, "gpu": any(w in low for w in ("hip", "cuda", "device", "gpu", "hsa"))}
    with open(out_path, "w") as f:
        json.dump(res, f)
    return 2 if "error" in res else 0


if __name__ == "__main__":
    sys.exit(main())
