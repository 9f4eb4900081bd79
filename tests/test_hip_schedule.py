"""The engine's cross-stream ordering at full size, with the streams forced out of step.

The backward pass runs on up to three streams (caller's chain, side stream, tap stream) ordered only by the fork() /
mark() / need() / SideReads::write() calls of csrc/engine.cpp, and the gradient-ready announcements rest on them.  On
the bench shapes the streams overlap, but a missing edge still loses its race only now and then.  The test-only lag
switches make it lose every time: MMVQA_SIDE_LAG_US delays the side / tap stream behind every fork, MMVQA_MAIN_LAG_US
delays the caller's stream behind every fork's event.  Both, like the schedule switches, are read once per process:
each variant runs in a child process of its own (tests/schedule_child.py), one at a time, under its own time limit.

(a) announcement finality at the bench shapes: every range is bit-equal, read through its `ready` event, to its final
    contents; a -0.0 poison written through the event survives (late atomic adds cannot hide under it as under NaN).
(b) values of every schedule against the fp64 oracle, with the bounds of test_hip_model.run_case / compare_grads: a
    missing need() / write() leaves a wrong value that is final, which (a) cannot see.
(c) FusedAdam.overlap_backward() at the bench shape, tuned, under side lag, against the one-launch optimizer."""
import copy
import json
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import synth  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import relerr  # noqa: E402
from test_hip_model import TOL, build_oracle, oracle_loss  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
CHILD = os.path.join(HERE, "schedule_child.py")

# the per-process switches this module sets; nothing else of the parent's environment is changed
SWITCHES = ("MMVQA_TAP_STREAM_OFF", "MMVQA_TAP_FIRST", "MMVQA_ENC_SIDE_OFF", "MMVQA_SIDE_PRIO_OFF", "MMVQA_NO_SIDE_STREAM",
            "MMVQA_SIDE_LAG_US", "MMVQA_MAIN_LAG_US")
SCHEDULES = {"default": None, "tap_stream_off": "MMVQA_TAP_STREAM_OFF", "tap_first": "MMVQA_TAP_FIRST",
             "enc_side_off": "MMVQA_ENC_SIDE_OFF", "side_prio_off": "MMVQA_SIDE_PRIO_OFF",
             "no_side_stream": "MMVQA_NO_SIDE_STREAM"}
# a lag well above the duration of one chain launch at these shapes, so that the lagging stream is always behind
LAGS = {"nolag": None, "sidelag": ("MMVQA_SIDE_LAG_US", "300"), "mainlag": ("MMVQA_MAIN_LAG_US", "300")}

NO_DROPOUT = dict(hidden_dropout_prob=0.0, emb_dropout_prob=0.0, rf_dropout_prob=0.0)
CONFIGS = {   # (Model args, kind, bench batch, T)
    "config2": (dict(**NO_DROPOUT), "mlm", 16, 32),
    "config3": (dict(cnn_encoder="tf_efficientnetv2_m", transformer_model="realformer", heads=8, supcon=True, **NO_DROPOUT),
                "supcon", 8, 32),
    "config1": (dict(dataset="VQA-Med", vocab_size=1552, emb_vocab=30522, **NO_DROPOUT), "vqa", 4, 28),
}

_halted = []   # a child that died by a signal, ran out of time or hit a GPU error: no further child is started


def batch(cfg, B, seed):
    args, kind, _, T = CONFIGS[cfg]
    a = O.make_args(**args)
    if kind == "vqa":
        return synth.vqa_batch(B, T, 224, vocab=a.emb_vocab, n_classes=a.vocab_size, seed=seed)
    return synth.roco_batch(B, T, 224, vocab=a.vocab_size, seed=seed, mlm_prob=0.3)


def run_child(case_path, tmp_path, env_on, timeout):
    """one child under its own time limit; returns its JSON result (fails the test -- and halts the module -- on a
    signal, a time-out or a GPU error)"""
    if _halted:
        pytest.fail(f"not started: an earlier child of this module failed hard ({_halted[0]})")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_on)
    out = os.path.join(str(tmp_path), "result.json")
    if os.path.exists(out):
        os.remove(out)
    argv = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [CHILD, str(case_path), out]
    what = " ".join(f"{k}={v}" for k, v in sorted(env_on.items())) or "default schedule"
    try:
        p = subprocess.run(argv, env=env, timeout=timeout, capture_output=True, text=True)
    except subprocess.TimeoutExpired:
        _halted.append(f"{what}: time-out after {timeout} s")
        pytest.fail(_halted[-1])
    tail = (p.stdout[-2000:] + p.stderr[-3000:]).strip()
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
        _halted.append(f"{what}: exit status {p.returncode}")
        pytest.fail(f"{_halted[-1]}\n{tail}")
    if not os.path.exists(out):
        pytest.fail(f"{what}: no result (exit status {p.returncode})\n{tail}")
    with open(out) as f:
        res = json.load(f)
    if "error" in res:
        if res.get("gpu"):
            _halted.append(f"{what}: GPU error")
        pytest.fail(f"{what}: the child raised\n{res['error']}\n{tail}")
    assert p.returncode == 0, (p.returncode, tail)
    return res


def env_of(schedule, lag):
    env = {}
    if SCHEDULES[schedule]:
        env[SCHEDULES[schedule]] = "1"
    if LAGS[lag]:
        env[LAGS[lag][0]] = LAGS[lag][1]
    return env


def assert_partition(ranges, n, what):
    cover = sorted(tuple(r) for r in ranges)
    assert len(cover) >= 4 and cover[0][0] == 0 and cover[-1][1] == n, (what, cover)
    assert all(a[1] == b[0] for a, b in zip(cover[:-1], cover[1:])), (what, cover)


# --------------------------------------------------------------------------- (a) announcement finality
FINALITY = (
    [("config2", s, "sidelag", False) for s in ("default", "tap_stream_off", "tap_first", "enc_side_off", "side_prio_off")]
    + [("config2", "default", lag, False) for lag in ("nolag", "mainlag")]
    + [("config2", "default", lag, True) for lag in ("nolag", "sidelag", "mainlag")]
    + [(cfg, "default", lag, False) for cfg in ("config3", "config1") for lag in ("nolag", "sidelag")]
)


@pytest.mark.parametrize("cfg,schedule,lag,tuned", FINALITY,
                         ids=[f"{c}-{s}-{l}{'-tuned' if t else ''}" for c, s, l, t in FINALITY])
def test_announced_ranges_are_final(tmp_path, cfg, schedule, lag, tuned):
    """bench shape: the announced ranges partition the buffer, each is final when its `ready` event fires (bit-equal
    snapshot) and nothing writes into it afterwards (-0.0 poison survives bit for bit)"""
    args, kind, B, _ = CONFIGS[cfg]
    case = dict(mode="finality", args=args, kind=kind, B=B, state=None, seed=21, tune=tuned,
                inputs=[batch(cfg, B, seed=7)])
    path = tmp_path / "case.pt"
    torch.save(case, path)
    res = run_child(path, tmp_path, env_of(schedule, lag), timeout=300 if tuned else 200)
    n = res["n"]
    assert_partition(res["ranges"], n, "snapshot pass")
    assert_partition(res["poison_ranges"], n, "poison pass")
    assert not res["snapshot_mismatch"], \
        "ranges changed after their announcement ([lo, hi), elements changed, max |change|, max |final|): " + \
        str(res["snapshot_mismatch"][:8])
    assert not res["poison_overwritten"], \
        "written after their announcement ([lo, hi), elements no longer -0.0): " + str(res["poison_overwritten"][:8])


# --------------------------------------------------------------------------- (b) values against the fp64 oracle
VALUE_B = {"config2": 2, "config3": 4}   # (batches the CPU oracle, fp32 and fp64, runs in seconds; (a) covers the bench grids)
_truth = {}


def truth_case(cfg, tmp_path_factory):
    """the oracle of a (b) case, evaluated once per module: fp32 and fp64 as run_case does, written for the children"""
    if cfg in _truth:
        return _truth[cfg]
    args_kw, kind, _, T = CONFIGS[cfg]
    B = VALUE_B[cfg]
    args = O.make_args(**args_kw)
    orc = build_oracle(args, seed=0)
    img, ids, seg, mask, tgt = batch(cfg, B, seed=5)
    init_sd = {k: v.detach().clone() for k, v in orc.state_dict().items()}
    orc64 = copy.deepcopy(orc).double().train()
    orc.train()
    out_ref = orc(img, ids, seg, mask)
    loss_ref = oracle_loss(kind, out_ref, tgt, B)
    loss_ref.backward()
    oracle_loss(kind, orc64(img.double(), ids, seg, mask), tgt, B).backward()
    p64 = dict(orc64.named_parameters())
    grads, tol, no_grad = {}, {}, []
    for name, p in orc.named_parameters():
        if p.grad is None:
            no_grad.append(name)
            continue
        truth = p64[name].grad
        tol[name] = max(TOL, 5 * relerr(p.grad, truth))   # compare_grads: 5 x the fp32 oracle's own error
        grads[name] = truth.float()
    osd = orc.state_dict()
    logits_ref = out_ref if kind == "mlm" else out_ref[0]
    check = dict(logits=logits_ref.detach(), feat=out_ref[1].detach() if kind == "supcon" else None,
                 grads=grads, no_grad=no_grad,
                 stats={k: v for k, v in osd.items() if "running_" in k},
                 nbt={k: int(v) for k, v in osd.items() if k.endswith("num_batches_tracked")})
    case = dict(mode="values", args=args_kw, kind=kind, B=B, state=init_sd, tune=False,
                inputs=[(img, ids, seg, mask, tgt)], check=check)
    path = tmp_path_factory.mktemp(f"truth_{cfg}") / "case.pt"
    torch.save(case, path)
    _truth[cfg] = (path, float(loss_ref.detach()), tol, check["stats"].keys(), check["nbt"])
    del orc, orc64, case
    return _truth[cfg]


VALUES = ([("config2", s, lag) for s in SCHEDULES for lag in LAGS]
          + [("config3", "default", lag) for lag in ("sidelag", "mainlag")])


@pytest.mark.parametrize("cfg,schedule,lag", VALUES, ids=[f"{c}-{s}-{l}" for c, s, l in VALUES])
def test_schedule_values_match_the_oracle(tmp_path, tmp_path_factory, cfg, schedule, lag):
    """logits, loss, every gradient, running statistics and num_batches_tracked of one training step under this
    schedule / lag, with the bounds of run_case (stat_tol = TOL as for the full-size cases)"""
    path, loss_ref, tol, stat_keys, nbt_ref = truth_case(cfg, tmp_path_factory)
    res = run_child(path, tmp_path, env_of(schedule, lag), timeout=200)
    assert res["logits"] <= TOL, f"logits rel err {res['logits']:.2e}"
    assert abs(res["loss"] - loss_ref) <= TOL * abs(loss_ref), (res["loss"], loss_ref)
    if res["feat"] is not None:
        assert res["feat"] <= TOL, f"feat {res['feat']:.2e}"
    bad = [(n, res["grads"][n], t) for n, t in tol.items() if res["grads"][n] is None or not res["grads"][n] <= t]
    assert not bad, "gradient mismatches: " + ", ".join(
        f"{n} {'missing' if e is None else f'{e:.2e}'} (tol {t:.1e})" for n, e, t in bad[:12])
    assert all(v == 0.0 for v in res["no_grad"].values()), {k: v for k, v in res["no_grad"].items() if v}
    assert sorted(res["stats"]) == sorted(stat_keys)
    bad = {k: e for k, e in res["stats"].items() if not e <= TOL}
    assert not bad, f"running statistics: {bad}"
    assert res["nbt"] == nbt_ref


# --------------------------------------------------------------------------- (c) overlapped Adam at the bench shape
def test_adam_beside_the_backward_pass_bench_shape_lagged(tmp_path):
    """config 2, batch 16, tuned, side stream lagging, two steps of FusedAdam.overlap_backward(): the ranges updated during
    backward partition the buffer, step() leaves no gradient behind (a late atomic add after an early update zeroed its
    range would), and the one-launch optimizer applied to the same state and to the gradients each ranged update read
    lands on the same parameters and moments bit for bit.  (Two independent full-depth runs are not a yardstick here:
    150 train-mode BatchNorms amplify the order of the float atomics, and Adam's first steps move by lr x sign(g).)"""
    args, kind, B, _ = CONFIGS["config2"]
    case = dict(mode="adam", args=args, kind=kind, B=B, state=None, seed=23, tune=True, lr=1e-3,
                inputs=[batch("config2", B, seed=40 + i) for i in range(2)])
    path = tmp_path / "case.pt"
    torch.save(case, path)
    res = run_child(path, tmp_path, env_of("default", "sidelag"), timeout=400)
    n = res["n"]
    for done in res["done"]:
        pos = 0
        for lo, hi in done:
            assert lo == pos, (lo, pos, done)
            pos = hi
        assert pos == n and len(done) >= 4, done
    assert res["grads_left"] == [0.0, 0.0], res["grads_left"]
    assert res["same"] == [[True, True, True]] * 2, \
        f"ranged updates differ from the one-launch optimizer on the same gradients (params, m, v per step): {res['same']}"
