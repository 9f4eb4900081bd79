"""FusedAdam(ema_decay=) over real training steps of a mini model, the averaged() context, the optimizer state dict
and the wiring of --ema_decay in the loops of mmvqa_amd.train."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import mmvqa_amd  # noqa: E402
from mmvqa_amd import _lib as L, synth, train  # noqa: E402
from mmvqa_amd.amp import GradScaler  # noqa: E402
from mmvqa_amd.ddp import GradReducer  # noqa: E402
from oracle import mmbert_oracle as O  # noqa: E402
from hip_helpers import relerr  # noqa: E402
from ema_helpers import ema_bound, ema_f64_step, magnitude, same_bits  # noqa: E402

BACKBONE = "transformer.trans.model."
DECAY, STEPS = 0.9, 6


def mini_args():
    return O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12, vocab_size=64,
                       emb_vocab=64, bert_max_pos=32, hidden_dropout_prob=0.0, emb_dropout_prob=0.0)


def mini(frozen=False, overlap=False, **kw):
    torch.manual_seed(0)
    model = mmvqa_amd.Model(mini_args()).to("cuda").train()
    model.set_seed(0)
    if frozen:
        for name, p in model.named_parameters():
            if name.startswith(BACKBONE):
                p.requires_grad_(False)
                p.grad = None
    opt = mmvqa_amd.FusedAdam(model, lr=1e-3, ema_decay=DECAY, **kw)
    red = GradReducer(model.flat_grads)
    if overlap:
        opt.overlap_backward(red, grad_scale=1.0)
    batch = synth.roco_batch(2, 16, 32, 64, seed=1, device="cuda")
    return model, opt, red, batch


class Flat:
    """what FusedAdam needs of a model: the flat parameter and gradient buffers"""

    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.flat_params = torch.randn(n, generator=g).cuda()
        self.flat_grads = torch.zeros(n, device="cuda")


# ----------------------------------------------------------------------------- the average over real steps
@pytest.mark.parametrize("form", ["plain", "frozen", "overlap"])
def test_average_over_real_steps(form):
    """six mlm_steps: opt.ema against the float64 recurrence over snapshots of flat_params, at ema_bound(6, M).  frozen:
    the backbone has requires_grad=False (the segment-table launch) and its range of ema keeps the bits of its initial
    copy.  overlap: the ranged launches of overlap_backward()."""
    model, opt, red, batch = mini(frozen=form == "frozen", overlap=form == "overlap")
    e0 = opt.ema.clone()
    assert same_bits(e0, model.flat_params) and opt.ema_updates == 0
    E = e0.double().cpu()
    M = magnitude(e0)
    for k in range(STEPS):
        train.mlm_step(model, opt, red, 1, batch)
        torch.cuda.synchronize()
        E = ema_f64_step(E, model.flat_params, DECAY)
        M = max(M, magnitude(model.flat_params, opt.ema))
    assert opt.ema_updates == STEPS == opt.step_count
    dist = (opt.ema.double().cpu() - E).abs().max().item()
    bound = ema_bound(STEPS, M)
    lag = (opt.ema - model.flat_params).abs().max().item()
    print(f"{form}: |ema - f64| {dist:.3e}, bound {bound:.3e}, |ema - p| {lag:.3e}")
    assert dist <= bound
    assert lag > 100 * bound           # the average is not the parameters
    if form == "frozen":
        rows = [(lo, hi) for name, _, lo, hi in model._param_ranges() if name.startswith(BACKBONE)]
        assert rows and opt._segs is not None
        for lo, hi in rows:
            assert same_bits(opt.ema[lo:hi], e0[lo:hi]) and same_bits(model.flat_params[lo:hi], e0[lo:hi])
        assert not same_bits(opt.ema, e0)


# ----------------------------------------------------------------------------- a step the scaler skips
def test_skipped_step_leaves_the_average_alone():
    n = 4100
    flat = Flat(n, 0)
    opt = mmvqa_amd.FusedAdam(flat, lr=1e-3, ema_decay=DECAY, ema_warmup=True)
    sc = GradScaler(init_scale=2.0 ** 10, growth_interval=3)
    gen = torch.Generator().manual_seed(3)

    def step(plant=None):
        grad = torch.randn(n, generator=gen) * 1e3
        if plant is not None:
            grad[plant[0]] = plant[1]
        flat.flat_grads.copy_(grad.cuda())
        sc.step(opt)
        skipped = sc.found_inf()
        sc.update()
        return skipped

    assert not step() and opt.ema_updates == 1
    for plant in ((0, float("inf")), (n - 1, float("-inf")), (n - 2, float("nan"))):
        e0, p0, c0 = opt.ema.clone(), flat.flat_params.clone(), opt.step_count
        assert step(plant)
        assert same_bits(opt.ema, e0) and same_bits(flat.flat_params, p0)
        assert opt.ema_updates == 1 and opt.step_count == c0
    e0 = opt.ema.clone()
    assert not step() and opt.ema_updates == 2 and not same_bits(opt.ema, e0)


# ----------------------------------------------------------------------------- with opt.averaged():
def test_averaged_context():
    model, opt, red, batch = mini()
    for _ in range(STEPS):
        train.mlm_step(model, opt, red, 1, batch)
    live, avg = model.flat_params.clone(), opt.ema.clone()
    ptr = model.flat_params.data_ptr()
    model.eval()
    with torch.no_grad():
        out_live = model(*batch[:4])
        with opt.averaged():
            assert model.flat_params.data_ptr() == ptr            # the engine stays bound to the same buffer
            assert same_bits(model.flat_params, avg) and same_bits(opt.ema, live)
            out_avg = model(*batch[:4])
            with pytest.raises(L.MMVQAError, match="averaged"):
                opt.step()
            with pytest.raises(L.MMVQAError, match="averaged"):
                opt.state_dict()
        assert same_bits(model.flat_params, live) and same_bits(opt.ema, avg)
        # a second model with the averaged parameters and the first model's live buffers
        other = mmvqa_amd.Model(mini_args()).to("cuda")
        other.load_state_dict(model.state_dict())
        other.flat_params.copy_(avg)
        other.eval()
        out_other = other(*batch[:4])
    err, moved = relerr(out_avg, out_other), relerr(out_avg, out_live)
    print(f"averaged forward against the second model: {err:.3e}; against the live weights: {moved:.3e}")
    assert err < 1e-5
    assert moved > 1e-4                # the averaged model is another model than the live one
    # an exception inside the context: the weights come back all the same
    with pytest.raises(RuntimeError, match="inside"):
        with opt.averaged():
            raise RuntimeError("inside")
    assert same_bits(model.flat_params, live) and same_bits(opt.ema, avg)
    model.train()
    train.mlm_step(model, opt, red, 1, batch)                     # ... and training goes on
    assert opt.ema_updates == STEPS + 1


# ----------------------------------------------------------------------------- state dict
def test_state_dict_round_trip(capsys):
    n = 4100
    a = Flat(n, 1)
    opt_a = mmvqa_amd.FusedAdam(a, lr=1e-3, ema_decay=0.99, ema_warmup=True)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        a.flat_grads.copy_(torch.randn(n, generator=gen).cuda())
        opt_a.step()
    sd = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in opt_a.state_dict().items()}
    assert sd["ema_updates"] == 3 and sd["ema_decay"] == 0.99 and sd["ema_warmup"] is True
    b = Flat(n, 2)
    b.flat_params.copy_(a.flat_params)
    opt_b = mmvqa_amd.FusedAdam(b, lr=1e-3, ema_decay=0.5)
    opt_b.load_state_dict(sd)
    assert (opt_b.ema_decay, opt_b.ema_warmup, opt_b.ema_updates) == (0.99, True, 3) and same_bits(opt_b.ema, opt_a.ema)
    g = torch.randn(n, generator=gen).cuda()
    for f, o in ((a, opt_a), (b, opt_b)):
        f.flat_grads.copy_(g)
        o.step()
    torch.cuda.synchronize()
    assert same_bits(a.flat_params, b.flat_params) and same_bits(opt_a.ema, opt_b.ema)
    assert not same_bits(opt_a.ema, sd["ema"])
    # a checkpoint without an average into an averaging optimizer: the average starts from the current parameters
    plain = {k: v for k, v in sd.items() if not k.startswith("ema")}
    c = Flat(n, 3)
    opt_c = mmvqa_amd.FusedAdam(c, lr=1e-3, ema_decay=0.9)
    opt_c.ema.fill_(7.0)
    opt_c.ema_updates = 5
    capsys.readouterr()
    opt_c.load_state_dict(plain)
    assert same_bits(opt_c.ema, c.flat_params) and opt_c.ema_updates == 0 and opt_c.ema_decay == 0.9
    said = capsys.readouterr().out
    assert said.count("\n") == 1 and "starts from the current parameters" in said
    # ... and a checkpoint with one into a plain optimizer: ignored
    d = Flat(n, 4)
    opt_d = mmvqa_amd.FusedAdam(d, lr=1e-3)
    opt_d.load_state_dict(sd)
    assert opt_d.ema is None and opt_d.step_count == 3


# ----------------------------------------------------------------------------- the loops
MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--emb_vocab", "64", "--image_size", "32", "--steps_per_epoch", "2", "--val_steps", "1",
        "--epochs", "5", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--lr", "1e-3",
        "--ema_decay", "0.9", "--ema_warmup"]


def spy_on_loop(monkeypatch):
    """wrap what the loop calls; every wrapper snapshots the model's flat_params (and the optimizer's ema) on entry.
    -> the list of (what, flat_params, ema) and, per optimizer step, (live weights, average) right after it"""
    seen, after_step, built = [], [], {}
    real_build = train.build

    def build(args, ctx, n_classes=None):
        out = real_build(args, ctx, n_classes=n_classes)
        model, opt = out[0], out[1]
        built.update(model=model, opt=opt)
        real_step = opt.step

        def step(*a, **kw):
            seen.append(("step", model.flat_params.clone(), opt.ema.clone(), len(after_step)))
            real_step(*a, **kw)
            after_step.append((model.flat_params.clone(), opt.ema.clone()))
        opt.step = step
        return out

    def spy(owner, name):
        real = getattr(owner, name)

        def wrapper(*a, **kw):
            seen.append((name, built["model"].flat_params.clone(), built["opt"].ema.clone(), len(after_step)))
            return real(*a, **kw)
        monkeypatch.setattr(owner, name, wrapper)

    monkeypatch.setattr(train, "build", build)
    spy(train, "validate")
    spy(train.evaluate, "test")
    spy(train, "save_model")
    spy(train, "save_recorder")
    return seen, after_step


@pytest.mark.parametrize("mode", ["vqa", "mlm"])
def test_loop_wiring(monkeypatch, tmp_path, mode):
    """validation (and a per-epoch test, were one run) and save_model see the averaged weights, bit-equal to the average
    after the last optimizer step and different from the live weights; training steps and save_recorder see the live
    weights, and the recorder's optimizer state holds the average"""
    seen, after_step = spy_on_loop(monkeypatch)
    extra = ["--batch_size", "8", "--num_classes", "11"] if mode == "vqa" else ["--batch_size", "4"]
    train.main([mode, "--save_dir", str(tmp_path)] + extra + MINI)
    kinds = [s[0] for s in seen]
    assert kinds.count("step") == 10 and kinds.count("validate") == 5 and kinds.count("save_recorder") == 1
    assert kinds.count("save_model") >= 1
    for what, params, ema, steps_done in seen:
        if what == "step":
            if steps_done:
                live, avg = after_step[steps_done - 1]
                assert same_bits(params, live) and same_bits(ema, avg), "a training step began on other than the live weights"
            continue
        live, avg = after_step[steps_done - 1]
        assert not same_bits(live, avg)
        if what == "save_recorder":
            assert same_bits(params, live) and same_bits(ema, avg), "save_recorder must see the live weights"
        else:
            assert same_bits(params, avg) and same_bits(ema, live), f"{what} must see the averaged weights"
    rec = torch.load(tmp_path / "recorder_2.pt", weights_only=False)
    live, avg = after_step[-1]
    assert same_bits(rec["optimizer"]["ema"], avg) and rec["optimizer"]["ema_updates"] == 10
    assert rec["optimizer"]["ema_decay"] == 0.9 and rec["optimizer"]["ema_warmup"] is True
