"""The training loops under --mixed_precision on the GPU: the CLI runs of mlm and vqa (with and without --clip), one
vqa_step under the reference's scaler quirk against the explicit sequence, and two data-parallel ranks (gloo, one GPU)
with an inf injected on ONE rank only: the check runs after the all-reduce, so both ranks skip and keep equal scales."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

MINI = ["--resnet_layers", "1", "1", "1", "1", "--resnet_width", "8", "--hidden_size", "96", "--n_layers", "2",
        "--vocab_size", "64", "--emb_vocab", "64", "--image_size", "32", "--steps_per_epoch", "3", "--val_steps", "1",
        "--epochs", "1", "--max_position_embeddings", "16", "--hidden_dropout_prob", "0.1", "--mixed_precision"]


def test_mlm_cli_mixed_precision_three_steps(tmp_path):
    from mmvqa_amd import train
    best = train.main(["mlm", "--lr", "1e-3", "--batch_size", "4", "--save_dir", str(tmp_path)] + MINI)
    assert math.isfinite(best) and best < 10.0


@pytest.mark.parametrize("clip", [False, True])
def test_vqa_cli_mixed_precision_three_steps(tmp_path, clip):
    from mmvqa_amd import train
    best = train.main(["vqa", "--lr", "1e-3", "--batch_size", "8", "--num_classes", "11", "--save_dir", str(tmp_path)]
                      + MINI + (["--clip"] if clip else []))
    assert best == best


def test_vqa_step_quirk_equals_explicit_sequence():
    """vqa_step with a scaler = autocast forward, UNSCALED backward, grad x inv_scale, FusedAdam (utils.py:641-657).
    The reducer stand-in records the gradient the backward left (the all-reduce point), so that the explicit sequence
    runs on exactly that gradient: parameters and Adam moments must then be bit-equal."""
    import mmvqa_amd
    from mmvqa_amd import synth, train
    from mmvqa_amd.amp import GradScaler
    from test_hip_model import build_pair, mini_args
    args = mini_args(dataset="VQA-Med", vocab_size=23)
    _, a = build_pair(args, seed=3)
    _, b = build_pair(args, seed=3)
    a.train(); b.train()
    batch = tuple(t.cuda() for t in synth.vqa_batch(4, 10, 32, vocab=50, n_classes=23, seed=6))
    crit = lambda lg, t: mmvqa_amd.mlm_loss(lg, t)[0]   # noqa: E731
    opt_a, opt_b = mmvqa_amd.FusedAdam(a, lr=1e-3), mmvqa_amd.FusedAdam(b, lr=1e-3)
    scaler = GradScaler(init_scale=1024.0)

    class Snap:   # one rank: the all-reduce is the identity; keep what the backward produced
        def allreduce(self):
            self.g = a.flat_grads.clone()

    red = Snap()
    loss_a, _ = train.vqa_step(a, opt_a, red, 1, batch, crit, scaler=scaler)
    # the explicit sequence on model b: autocast forward, unscaled backward ...
    img, ids, seg, mask, tgt = batch
    opt_b.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16):
        logits, _, _ = b(img, ids, seg, mask)
        loss_b = crit(logits, tgt)
    loss_b.backward()
    torch.cuda.synchronize()
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())   # noqa: E731
    assert abs(float(loss_a.detach()) - float(loss_b.detach())) <= 1e-5 * abs(float(loss_b.detach()))
    assert rel(red.g, b.flat_grads) < 1e-2          # the recorded gradient is the UNSCALED one (scaled: 1024 x)
    # ... then grad x inv_scale and FusedAdam, on the gradient vqa_step saw
    b.flat_grads.copy_(red.g)
    inv = torch.tensor([1024.0]).double().reciprocal().float().item()
    b.flat_grads.mul_(inv)
    opt_b.step(grad_scale=1.0, zero_grad=True)
    torch.cuda.synchronize()
    assert torch.equal(opt_a.m, opt_b.m) and torch.equal(opt_a.v, opt_b.v)
    assert torch.equal(a.flat_params, b.flat_params)
    assert opt_a.step_count == opt_b.step_count == 1
    assert scaler.get_scale() == 1024.0   # one finite step, growth interval 2000


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import mmvqa_amd
        from mmvqa_amd import synth
        from mmvqa_amd.amp import GradScaler
        from mmvqa_amd.ddp import GradReducer
        from oracle import mmbert_oracle as O
        dev = torch.device("cuda", 0)
        args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=16, hidden_size=96, n_layers=2, heads=12, vocab_size=64,
                           emb_vocab=64, bert_max_pos=32, hidden_dropout_prob=0.0, emb_dropout_prob=0.0, rf_dropout_prob=0.0)
        torch.manual_seed(0)
        model = mmvqa_amd.Model(args).to(dev).train()
        opt = mmvqa_amd.FusedAdam(model, lr=1e-3)
        red = GradReducer(model.flat_grads, bucket_mb=0.02)
        scaler = GradScaler(init_scale=2.0 ** 12, growth_interval=3)
        out = []
        for step in range(3):
            img, ids, seg, mask, tgt = synth.roco_batch(3, 16, 64, vocab=64, seed=40 + 7 * step + rank, device=dev, mlm_prob=0.4)
            opt.zero_grad()
            with torch.autocast("cuda", dtype=torch.float16):
                loss = mmvqa_amd.mlm_loss(model(img, ids, seg, mask), tgt)[0]
            scaler.scale(loss).backward()
            if step == 1 and rank == 1:
                model.flat_grads[5] = float("inf")      # this rank only
            red.allreduce()
            p0 = model.flat_params.clone()
            scaler.step(opt, grad_scale=1.0 / world, zero_grad=True)
            skipped = scaler.found_inf()
            scaler.update()
            torch.cuda.synchronize()
            out.append((skipped, scaler.get_scale(), bool(torch.equal(p0, model.flat_params)), opt.step_count,
                        float(model.flat_params.double().sum())))
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_two_ranks_skip_together_when_one_rank_sees_inf():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 33500 + (os.getpid() % 2000)
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = dict(q.get(timeout=300) for _ in range(2))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    a, b = res[0], res[1]
    assert [s[0] for s in a] == [False, True, False] == [s[0] for s in b]
    assert [s[1] for s in a] == [s[1] for s in b] == [2.0 ** 12, 2.0 ** 11, 2.0 ** 11]
    assert a[1][2] and b[1][2], "a skipped step moved the parameters"
    assert [s[3] for s in a] == [s[3] for s in b] == [1, 1, 2]
    assert [s[4] for s in a] == [s[4] for s in b], "replicas diverged"
