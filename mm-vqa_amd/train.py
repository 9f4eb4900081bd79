"""Training loops (callers of the hot path) -- build-owned counterparts of the reference's scripts,
which never ship to the GPU box (SURVEY.md 8(b) "Callers the build must supply"):

  mlm      pretrain/roco_train.py:155-197 + pretrain/roco_utils.py:207-372 (train_one_epoch / validate)
  supcon   pretrain/roco_supcon_train.py:137,168-202 + models/SupConLoss/supcon_utils.py:253-379
  distill  the same two files with --task distillation: the headless model against the teacher's per-token states
           (roco_utils.py:112-132, 230-238), read from --teacher_states, or computed per batch by the BERT teacher on the
           device (--teacher_weights, teacher.BertTeacher)
  vqa      vqamed2019/train.py:125-296 + vqamed2019/utils.py:625-767
  eval     vqamed2019/eval.py:99-180 + vqamed2019/utils.py:769-843 (test-set run: metrics, <model>_preds.csv, <model>_res.txt)
  gradcam  vqamed2019/grad_cam2.py:99-188 over the test split (one overlay PNG per row + gradcam_index.csv)

Kept from the reference: option names and defaults, Adam(lr) + ReduceLROnPlateau(patience, factor) on the
validation loss, zero_grad -> forward -> loss -> backward -> step order, loss / accuracy definitions,
half-batch x 2 views for SupCon, best-val-loss checkpoint, the 5-epoch "recorder" dict
{epoch, optimizer, scheduler, scaler, model}, --resume, the VQA early-stop counter and classifier[2] surgery.
Data: with --data_dir (and --vocab_file, a local WordPiece vocab.txt) every loop reads ROCO or VQA-Med 2019 from
disk through mmvqa_amd.data (host decode + tokenisation in worker processes, the image transforms on the GPU in a
DeviceFeeder); without it they run on synthetic batches of the same layout (mmvqa_amd.synth).  SupCon reads the ROCO
train table with its back-translations and makes both views of each image on the device in one launch
(roco_supcon_train.py:83-85,137; supcon_utils.py:218-256).  Not kept (out of scope): wandb, BLEU.  One process per GPU under
torch.distributed (RCCL).

    python -m mmvqa_amd.train mlm    --run_name r --mlm_prob 0.15 --epochs 2 --steps_per_epoch 20
    python -m mmvqa_amd.train supcon --run_name r --mlm_prob 0.15 --batch_size 32
    python -m mmvqa_amd.train distill --run_name r --emb_vocab 28996 --epochs 2 --steps_per_epoch 20
    python -m mmvqa_amd.train distill --data_dir roco-dataset/data --emb_vocab 28996 --bert_weights clinicalbert.pt \\
                                      --teacher_states roco_train_teacher.npz --val_teacher_states roco_val_teacher.npz
    python -m mmvqa_amd.train distill --data_dir roco-dataset/data --emb_vocab 28996 --bert_weights clinicalbert.pt \\
                                      --teacher_weights clinicalbert.pt --teacher_vocab_file clinicalbert_vocab.txt
    python -m mmvqa_amd.train vqa    --run_name r --loss ASLSingleLabel --batch_size 64
    python -m mmvqa_amd.train vqa    --run_name r --smoothing 0.1 --batch_size 64
    python -m mmvqa_amd.train vqa    --run_name r --group_by_image --batch_size 64     # each image once for its questions
    python -m mmvqa_amd.train vqa    --run_name r --cache_tokens --cache_views 4       # frozen backbone: encode every image once
    python -m mmvqa_amd.train vqa    --cache_tokens --cache_views 4 --data_dir VQA-Med --vocab_file vocab.txt
    python -m mmvqa_amd.train eval   --model_dir save/MLM/r.pt --num_classes 1552 --batch_size 16
    python -m mmvqa_amd.train mlm    --watch all --watch_freq 100     # per-tensor statistics -> save/watch_mlm.jsonl
    python -m mmvqa_amd.train vqa    --ema_decay 0.999 --ema_warmup   # validate and save the averaged weights
    python -m mmvqa_amd.train mlm    --data_dir roco-dataset/data --vocab_file vocab.txt --num_workers 4
    python -m mmvqa_amd.train supcon --data_dir roco-dataset/data --vocab_file vocab.txt --batch_size 32
    python -m mmvqa_amd.train supcon --data_dir roco-dataset/data --vocab_file vocab.txt --supcon_mask jaccard
    python -m mmvqa_amd.train supcon --data_dir roco-dataset/data --vocab_file vocab.txt --supcon_mask embeddings \\
                                     --caption_embeddings roco_train_embeddings.npz
    python -m mmvqa_amd.train supcon --data_dir roco-dataset/data --vocab_file vocab.txt --supcon_mask cosine \\
                                     --teacher_weights clinicalbert.pt --teacher_vocab_file clinicalbert_vocab.txt
    python -m mmvqa_amd.train supcon --data_dir roco-dataset/data --vocab_file vocab.txt --supcon_mask bert_score \\
                                     --teacher_weights scibert.pt --teacher_vocab_file scibert_vocab.txt \\
                                     --teacher_lower_case --bert_score_layer 8 --max_token_length 64
"""
from __future__ import annotations

import argparse
import contextlib
import os
import sys

import numpy as np
import torch
import torch.distributed as dist
from torch.optim import lr_scheduler

from . import (CategorySmoothing, FusedAdam, LabelSmoothing, Model, asl_loss, checkpoint, distill_loss, embedding_mask,
               evaluate, jaccard_mask, mlm_loss, no_decay, split_feat, supcon_loss, synth)
from . import data as D
from .amp import GradScaler
from .ddp import (GradReducer, comm_info, global_supcon_means, global_supcon_pairs, global_supcon_states, global_supcon_views,
                  sync_replicas)
from .ddp import world as ddp_world
from .teacher import BertTeacher, bertscore_mask_unit, cosine_mask_from_means, normalize_states_


def common_args(p):
    p.add_argument("-r", "--run_name", type=str, default="run")
    p.add_argument("--save_dir", type=str, default="save")
    p.add_argument("--batch_size", type=int, default=16)
    p.add_argument("--patience", type=int, default=5)
    p.add_argument("--factor", type=float, default=0.1)
    p.add_argument("--epochs", type=int, default=10)
    p.add_argument("--steps_per_epoch", type=int, default=50, help="synthetic batches per epoch")
    p.add_argument("--val_steps", type=int, default=5)
    p.add_argument("--n_layers", type=int, default=4)
    p.add_argument("--heads", type=int, default=12)
    p.add_argument("--type_vocab_size", type=int, default=2)
    p.add_argument("--vocab_size", type=int, default=30522)
    p.add_argument("--hidden_size", type=int, default=768)
    p.add_argument("--hidden_dropout_prob", type=float, default=0.3)
    p.add_argument("--cnn_encoder", type=str, default="resnet152")
    p.add_argument("--transformer_model", type=str, default="transformer",
                   choices=["transformer", "realformer", "feedback-transformer"])
    p.add_argument("--num_vis", type=int, default=5)
    p.add_argument("--use_relu", action="store_true", default=False)
    p.add_argument("--resume", action="store_true", default=False)
    p.add_argument("--image_size", type=int, default=224)
    p.add_argument("--seed", type=int, default=1234)
    p.add_argument("--state_dict", type=str, default=None, help="local checkpoint to start from")
    p.add_argument("--backbone_weights", type=str, default=None,
                   help="local torchvision resnet152 / timm tf_efficientnetv2_m state_dict (what pretrained=True fetches, image_encoding.py:20-26)")
    p.add_argument("--bert_weights", type=str, default=None,
                   help="local HF bert-base-uncased state_dict: its embeddings are used (mmbert.py:52-56)")
    # reduced backbones for smoke tests
    p.add_argument("--resnet_layers", type=int, nargs=4, default=[3, 8, 36, 3])
    p.add_argument("--resnet_width", type=int, default=64)
    p.add_argument("--emb_vocab", type=int, default=30522)
    p.add_argument("--bucket_mb", type=float, default=64.0, help="all-reduce bucket size (data parallel)")
    p.add_argument("--mixed_precision", action="store_true", default=False,
                   help="fp16 autocast + loss scaling (mmvqa_amd.amp.GradScaler): every conv / linear contraction of the "
                        "ResNet encoders, the transformer and the heads rounds both operands to fp16 (fp32 accumulation, "
                        "everything else fp32).  vqa reproduces the reference's loop (utils.py:651-657): scaler.scale(loss) is "
                        "computed and discarded, the backward is unscaled, --clip acts on those gradients and scaler.step "
                        "then divides them by the scale.  supcon: accepted, runs fp32 (the reference's SupCon loop has no "
                        "autocast).  Not with --overlap_adam")
    p.add_argument("--overlap_adam", action="store_true", help="Adam per finished gradient range beside the backward pass (measured time-neutral; not with --clip)")
    # beyond the reference (its --weight_decay stays commented out, vqamed2019/train.py:53; its freeze too,
    # models/image_encoding.py:50-51): the defaults reproduce a run without these options
    p.add_argument("--weight_decay", type=float, default=0.0, help="decoupled (AdamW) weight decay")
    p.add_argument("--adam_l2", action="store_true", help="weight decay as torch.optim.Adam(weight_decay=): added to the gradient")
    p.add_argument("--decay_all", action="store_true", help="decay biases, LayerNorm and BatchNorm parameters too (default: they get 0)")
    p.add_argument("--backbone_lr", type=float, default=None, help="learning rate of the CNN body (transformer.trans.model.*)")
    p.add_argument("--freeze_backbone", action="store_true", help="the CNN body gets no gradient; its backward pass is not run")
    p.add_argument("--freeze_bn_stats", action="store_true",
                   help="with --freeze_backbone: its BatchNorms use and keep their running statistics (backbone.eval())")
    p.add_argument("--cache_tokens", action="store_true", default=False,
                   help="vqa: freeze the CNN body and the five taps, encode every image once into a device-resident "
                        "cache of visual tokens (mmvqa_amd.tokens.TokenCache) and train the fusion encoder, the heads and "
                        "the embeddings from it (Model.forward_cached): no image is touched after the fill.  Not with "
                        "--mixed_precision, --group_by_image or more than one process")
    p.add_argument("--cache_views", type=int, default=None, metavar="K",
                   help="with --cache_tokens: K views per train image (default 1): view 0 is the evaluation transform, "
                        "views 1..K-1 are draws of the training augmentation; every sample of a step takes one at random")
    p.add_argument("--cache_images", type=int, default=None, metavar="N",
                   help="with --cache_tokens and without --data_dir: the synthetic train set has N images (default 8 x "
                        "--batch_size); with --data_dir the caches hold every distinct image of the train and validation tables")
    p.add_argument("--ema_decay", type=float, default=None, metavar="D",
                   help="mlm, supcon, distill, vqa: keep an exponential moving average of the weights, avg += (w - avg)(1 - D) "
                        "per optimizer step, in the launch that updates them (FusedAdam(ema_decay=)).  Every validation "
                        "and every saved .pt file then uses the averaged weights with the live BatchNorm "
                        "statistics, so the scheduler, the best-checkpoint choices and the early stop follow the "
                        "averaged model; the recorder keeps the live weights and, in the optimizer state, the average")
    p.add_argument("--ema_warmup", action="store_true", default=False,
                   help="with --ema_decay: the decay of update t is min(D, (1 + t) / (10 + t))")
    p.add_argument("--watch", type=str, default=None, choices=["gradients", "parameters", "all"],
                   help="mlm, supcon, distill, vqa: the reference's wandb.watch(model, log=...) (roco_train.py:80, "
                        "train.py:157): every --watch_freq steps, per-tensor counts of non-finite and zero values, min, "
                        "max, sum, sum of squares and a 64-bin histogram of the gradients Adam consumes and / or of the "
                        "parameters before the update, one JSON line per logged step in <save_dir>/watch_<loop>.jsonl.  "
                        "Under --mixed_precision a skipped step also names the tensors that overflowed.  All tensors "
                        "in at most three launches per buffer, off the step's critical path.  Not gradients with "
                        "--overlap_adam")
    p.add_argument("--watch_freq", type=int, default=1000, help="with --watch: log every N-th step (wandb's log_freq)")
    p.add_argument("--data_dir", type=str, default=None,
                   help="ROCO (mlm, supcon) or VQA-Med 2019 (vqa, eval) tree on disk; without it the batches are synthetic")
    p.add_argument("--vocab_file", type=str, default=None, help="WordPiece vocab.txt (with --data_dir)")
    p.add_argument("--num_workers", type=int, default=None, help="decode / tokenise worker processes (default min(4, usable cores))")
    p.add_argument("--feeder_depth", type=int, default=2, help="device batches prepared ahead of the step")


def feeder(args, ctx, dataset, train, aug=None, batch_size=None, views=1, pairs=False, category=False, teacher=False,
           grouped=False):
    """DeviceFeeder over one split (shuffled and augmented for training, file order and val transforms otherwise)"""
    host = D.HostLoader(dataset, batch_size or args.batch_size, shuffle=train, seed=args.seed, rank=ctx.rank,
                        world=ctx.world, num_workers=args.num_workers, aug=aug if train else None, size=args.image_size,
                        views=views)
    return D.DeviceFeeder(host, ctx.dev, train=train, depth=args.feeder_depth, pairs=pairs, category=category, teacher=teacher,
                          grouped=grouped)


def tokenizer(args):
    if not args.vocab_file:
        raise ValueError("--data_dir needs --vocab_file (a local WordPiece vocab.txt; nothing is downloaded)")
    return D.text.BertWordPiece(args.vocab_file)


def teacher_tokenizer(args):
    """the teacher's own WordPiece (--teacher_vocab_file), cased unless --teacher_lower_case: the clinical checkpoints
    the reference names are cased"""
    return D.text.BertWordPiece(args.teacher_vocab_file, do_lower_case=bool(args.teacher_lower_case))


def load_teacher(args, ctx):
    """the frozen BERT teacher of --teacher_weights on the step's device"""
    teacher = BertTeacher.from_state_dict(args.teacher_weights).to(ctx.dev)
    if args.max_token_length > min(512, teacher.max_pos):
        raise ValueError(f"--max_token_length {args.max_token_length} is more than the teacher takes "
                         f"(min(512, its {teacher.max_pos} positions))")
    return teacher


def roco_feeders(args, ctx):
    """(train, validation) feeders of the ROCO tree: roco_utils.py:71-97, 567-587"""
    tok, kw = tokenizer(args), D.load_keywords(args.data_dir)
    ds = lambda split: D.RocoDataset(D.roco_table(args.data_dir, split), tok, kw, args.num_vis,   # noqa: E731
                                     args.max_position_embeddings, args.mlm_prob, args.seed)
    return feeder(args, ctx, ds("train"), True, D.ROCO_AUG), feeder(args, ctx, ds("validation"), False)


def roco_supcon_feeders(args, ctx, pairs):
    """(train, validation) feeders of SupCon: `pairs` samples x 2 views per train batch (roco_supcon_train.py:134-139,
    drop_last=False), the plain ROCO validation split at the full --batch_size.  With --supcon_mask jaccard or
    embeddings the train batches carry each sample's (row, translation column) and the third value is what the mask is
    built from, on the device: the table's word sets, or its caption embeddings read from --caption_embeddings and
    normalised (else None).  With --supcon_mask cosine the workers tokenise caption and drawn translation with the
    teacher's WordPiece, the train batches carry those ids and the third value is the BERT teacher."""
    tok, kw = tokenizer(args), D.load_keywords(args.data_dir)
    table = D.roco_supcon_table(args.data_dir)
    kind = getattr(args, "supcon_mask", "none")
    masked = kind in ("jaccard", "embeddings")
    words, ttok = None, None
    if kind == "jaccard":
        words = D.WordSets.from_table(table).to(ctx.dev)
    elif kind == "embeddings":
        words = D.CaptionEmbeddings.from_file(args.caption_embeddings, table).to(ctx.dev)
    elif kind in ("cosine", "bert_score"):
        words, ttok = load_teacher(args, ctx), teacher_tokenizer(args)
        if kind == "bert_score" and not 1 <= args.bert_score_layer <= words.layers:
            raise ValueError(f"--bert_score_layer {args.bert_score_layer} is outside 1..{words.layers}, the depth of "
                             f"{args.teacher_weights}")
    tr = D.RocoSupConDataset(table, tok, kw, args.num_vis, args.max_position_embeddings, args.mlm_prob, args.seed,
                             report_aug_col=masked, teacher_tokenizer=ttok,
                             max_token_length=getattr(args, "max_token_length", 512))
    va = D.RocoDataset(D.roco_table(args.data_dir, "validation"), tok, kw, args.num_vis, args.max_position_embeddings,
                       args.mlm_prob, args.seed)
    return (feeder(args, ctx, tr, True, D.ROCO_AUG, batch_size=pairs, views=2, pairs=masked, teacher=ttok is not None),
            feeder(args, ctx, va, False), words)


def epoch_batches(fd, epoch, synthetic):
    """the batches of one epoch: from the feeder (--data_dir) or synthetic(i) for i < --steps_per_epoch"""
    if fd is None:
        for b in synthetic:
            yield b
        return
    fd.set_epoch(epoch)
    yield from fd


def train_seeds(args, ctx, epoch):
    """seeds of one epoch's synthetic train batches: another one for every epoch, step and rank"""
    return (args.seed + 7919 * (epoch * 100003 + i) + ctx.rank for i in range(args.steps_per_epoch))


def val_seeds(args, rank=0):
    """seeds of the synthetic validation batches, the same every epoch (run_vqa: and on every rank)"""
    return (10 ** 6 + i + rank for i in range(args.val_steps))


def synthetic_roco(args, ctx, seed, batch_size=None):
    return synth.roco_batch(batch_size or args.batch_size, args.max_position_embeddings, args.image_size,
                            min(args.vocab_size, args.emb_vocab), seed=seed, device=ctx.dev, mlm_prob=args.mlm_prob)


class Ctx:
    def __init__(self, args):
        self.world = int(os.environ.get("WORLD_SIZE", "1"))
        self.rank = int(os.environ.get("RANK", "0"))
        local = int(os.environ.get("LOCAL_RANK", "0"))
        rehearse = bool(os.environ.get("MMVQA_REHEARSE_GLOO"))   # every rank on cuda:0 over gloo: one-GPU rehearsal only
        if rehearse:
            local = 0
        if self.world > 1:
            os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
            os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            torch.cuda.set_device(local)
            if rehearse:
                dist.init_process_group("gloo")
            else:
                dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        self.dev = torch.device("cuda", local if self.world > 1 else 0)
        torch.cuda.set_device(self.dev)

    def mean(self, x: float) -> float:
        if self.world == 1:
            return x
        t = torch.tensor([x], device=self.dev, dtype=torch.float64)
        dist.all_reduce(t)
        return float(t) / self.world


def check_optimizer_args(args):
    """the rules between the optimizer options; raises ValueError with the rule that is broken"""
    if getattr(args, "freeze_bn_stats", False) and not getattr(args, "freeze_backbone", False):
        raise ValueError("--freeze_bn_stats requires --freeze_backbone")
    if getattr(args, "freeze_backbone", False) and getattr(args, "backbone_lr", None) is not None:
        raise ValueError("--freeze_backbone with --backbone_lr: a frozen backbone has no learning rate")
    if getattr(args, "weight_decay", 0.0) < 0:
        raise ValueError("--weight_decay must not be negative")
    ema = getattr(args, "ema_decay", None)
    if ema is not None and not 0.0 <= ema < 1.0:
        raise ValueError(f"--ema_decay {ema} is outside [0, 1)")
    if getattr(args, "ema_warmup", False) and ema is None:
        raise ValueError("--ema_warmup requires --ema_decay")


def optimizer_groups(args):
    """FusedAdam's keyword arguments from the options; all defaults -> none but lr: one group, no decay, mmvqa_adam"""
    kw = dict(lr=args.lr, weight_decay=getattr(args, "weight_decay", 0.0), decoupled=not getattr(args, "adam_l2", False))
    groups = []
    blr = getattr(args, "backbone_lr", None)
    wd = kw["weight_decay"]
    spare = wd != 0.0 and not getattr(args, "decay_all", False)
    if blr is not None and spare:     # first match wins: the backbone's BatchNorm parameters take its rate and no decay
        groups.append(dict(match=lambda n: n.startswith("transformer.trans.model.") and no_decay(n), lr=blr, weight_decay=0.0))
    if blr is not None:
        groups.append(dict(match="transformer.trans.model.", lr=blr))
    if spare:
        groups.append(dict(match=no_decay, weight_decay=0.0))
    if groups:
        kw["groups"] = groups
    if getattr(args, "ema_decay", None) is not None:
        kw.update(ema_decay=args.ema_decay, ema_warmup=bool(getattr(args, "ema_warmup", False)))
    return kw


def build(args, ctx, n_classes=None):
    check_optimizer_args(args)
    torch.manual_seed(args.seed)          # identical replicas
    model = Model(args)
    if args.backbone_weights:
        checkpoint.load_backbone(model, args.backbone_weights)
    if args.bert_weights:
        checkpoint.load_bert_embeddings(model, args.bert_weights)
    if args.state_dict:
        sd = checkpoint.read_state_dict(args.state_dict)
        own = model.state_dict()
        model.load_state_dict({k: v for k, v in sd.items() if k in own and own[k].shape == v.shape}, strict=False)
    if getattr(args, "use_pretrained", False):          # vqamed2019/train.py:125-135
        checkpoint.load_roco_pretrained(model, args.model_dir)
    if n_classes is not None:              # vqamed2019/train.py:137,141,149
        model.classifier[2] = torch.nn.Linear(args.hidden_size, n_classes)
    if getattr(args, "resume_training", False):         # vqamed2019/train.py:139-144
        checkpoint.load_model(model, args.resume_dir)
    model.to(ctx.dev)
    model.set_seed(args.seed + ctx.rank)
    cs = sync_replicas(model)              # rank 0's replica everywhere, checksum compared across ranks
    if getattr(args, "freeze_backbone", False):
        model.freeze_backbone("running" if args.freeze_bn_stats else "batch")
    if getattr(args, "cache_tokens", False):   # requires_grad = False: FusedAdam marks them ADAM_FROZEN, weight decay cannot move them
        model.freeze_visual()
    opt = FusedAdam(model, **optimizer_groups(args))
    sched = lr_scheduler.ReduceLROnPlateau(_SchedShim(opt), patience=args.patience, factor=args.factor)
    red = GradReducer(model.flat_grads, bucket_mb=getattr(args, "bucket_mb", 64.0))
    if ctx.world > 1:
        model.set_grad_ready_hook(red.start, with_event=True)
        if ctx.rank == 0:
            print(f"data parallel: {comm_info(red)} replica checksum {cs}", flush=True)
    # opt-in: Adam per finished (all-reduced) gradient range, beside the rest of the backward pass -- not with gradient
    # clipping, which needs the norm of the WHOLE gradient before the first update (vqamed2019/utils.py:663-664)
    if getattr(args, "overlap_adam", False) and not getattr(args, "clip", False):
        opt.overlap_backward(red, grad_scale=1.0 / ctx.world)
    return model, opt, sched, red


def averaged(args, opt):
    """--ema_decay: the context in which the model computes with, and saves, the averaged weights (FusedAdam.averaged);
    without the option a null context"""
    return opt.averaged() if getattr(args, "ema_decay", None) is not None else contextlib.nullcontext()


class _SchedShim(torch.optim.Optimizer):
    """lets torch's ReduceLROnPlateau drive the 'lr' of every FusedAdam.param_groups entry"""

    def __init__(self, fused):
        self.fused = fused
        self.param_groups = fused.param_groups
        self.defaults = {}
        self.state = {}


def save_recorder(args, epoch, model, opt, sched, mode, best=None):
    """the 5-epoch "recorder" dict of roco_train.py:164-171 / roco_supcon_train.py:177-184 (keys epoch, optimizer,
    scheduler, scaler, model), plus two keys the reference's dict lacks: which loop wrote it and the best-so-far
    trackers -- without them a resumed run re-saves its "best" checkpoint in the first epoch whatever the loss, and a
    recorder of another loop in the same save_dir is loaded blindly."""
    os.makedirs(args.save_dir, exist_ok=True)
    torch.save({"epoch": epoch, "optimizer": opt.state_dict(), "scheduler": sched.state_dict(), "scaler": {},
                "model": model.state_dict(), "mode": mode, "best": dict(best or {})},
               os.path.join(args.save_dir, "recorder_2.pt"))


def save_model(args, model, suffix=""):
    """torch.save(model.state_dict(), save_dir/task/run_name[+suffix].pt) -- roco_train.py:194-197,
    roco_supcon_train.py:199-202, vqamed2019/train.py:265-283"""
    d = os.path.join(args.save_dir, args.task)
    os.makedirs(d, exist_ok=True)
    torch.save(model.state_dict(), os.path.join(d, args.run_name + suffix + ".pt"))


def maybe_resume(args, model, opt, sched, mode):
    """-> (first epoch to run, best-so-far trackers of the interrupted run)"""
    path = os.path.join(args.save_dir, "recorder_2.pt")
    if not (args.resume and os.path.exists(path)):
        return 0, {}
    rec = torch.load(path, map_location="cpu", weights_only=False)
    if rec.get("mode", mode) != mode:
        raise RuntimeError(f"{path} was written by the '{rec['mode']}' loop, this is '{mode}': refusing to resume from it")
    model.load_state_dict(rec["model"])
    opt.load_state_dict(rec["optimizer"])
    sched.load_state_dict(rec["scheduler"])
    return rec["epoch"] + 1, dict(rec.get("best") or {})


# ----------------------------------------------------------------------------------------- one training step each
def _update(loss, model, opt, red, world, scaler=None, scaled_backward=True, clip=False, watch=None):
    """What every step does once it has its loss: backward -> gradient all-reduce -> Adam on the gradients over `world`
    (times the clip factor of clip_grad_norm_(1.0): global 2-norm over the averaged flat gradient buffer).  With a
    scaler: backward of scaler.scale(loss), scaler.step after the all-reduce, scaler.update.  scaled_backward=False is
    vqa_step's: scale(loss) is still called (it creates the scale tensor update() asserts), the backward is unscaled.
    watch (--watch, rank 0): on a logged step the statistics of the gradients Adam is about to consume (with a scaler:
    unscaled here, which scaler.step then does not repeat) and of the parameters before the update are enqueued between
    the all-reduce and the optimizer step; a step the scaler skips reports which tensors overflowed."""
    scaled = loss if scaler is None else scaler.scale(loss)
    (scaled if scaled_backward else loss).backward()
    red.allreduce()
    scale = 1.0 / world
    if clip:
        gn = float(model.flat_grads.norm()) * scale
        scale *= min(1.0, 1.0 / (gn + 1e-6))
    if watch is not None and watch.begin_step():
        if scaler is not None and watch.wants_grads:
            scaler.unscale_(opt)
        watch.log(scale)
    if scaler is None:
        opt.step(grad_scale=scale, zero_grad=True)
    else:
        scaler.step(opt, grad_scale=scale, zero_grad=True)
        if watch is not None:
            watch.set_loss_scale(scaler.get_scale())    # (scaler.step has read the device: this waits for nothing more)
            if scaler.found_inf():                      # skipped: Adam did not run, the gradients are still there
                watch.log_skipped(scaler.get_scale())
        scaler.update()


def make_watcher(args, ctx, loop, model):
    """the loop's Watcher (--watch, rank 0 only: after the all-reduce every rank holds the same gradients), or None"""
    if not getattr(args, "watch", None) or ctx.rank != 0:
        return None
    from .watch import Watcher
    return Watcher(model, args.watch, args.watch_freq, os.path.join(args.save_dir, f"watch_{loop}.jsonl"), loop)


def mlm_step(model, opt, red, world, batch, scaler=None, watch=None):
    """pretrain/roco_utils.py:214-247,257-265: zero_grad -> forward -> log_softmax + NLLLoss -> backward ->
    (gradient all-reduce) -> Adam.  Returns (loss, pred[B,T], stats = {loss, #target>0, #correct}).
    With a scaler (--mixed_precision, roco_utils.py:224-245): autocast forward + loss, scaled backward, scaler.step
    after the all-reduce (every rank checks the same gradients), scaler.update."""
    img, ids, seg, mask, tgt = batch
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16) if scaler is not None else contextlib.nullcontext():
        loss, pred, stats = mlm_loss(model(img, ids, seg, mask), tgt)
    _update(loss, model, opt, red, world, scaler, watch=watch)
    return loss, pred, stats


def process_tensors(img, caption_token, aug_tokens, segment_ids, attention_mask, target, aug_targets):
    """models/SupConLoss/supcon_utils.py:253-256: the two views concatenated along the batch; segment ids and
    attention mask of view 1 are used for BOTH views"""
    cat = lambda a, b: torch.cat([a, b], dim=0)   # noqa: E731
    return (cat(img[0], img[1]), cat(caption_token, aug_tokens), cat(segment_ids, segment_ids),
            cat(attention_mask, attention_mask), cat(target, aug_targets))


def teacher_inputs(rows, teacher_T=None):
    """teacher rows int64 [B, 1 + L] (data.teacher_row) -> (ids int64 [B, Tp] contiguous, lens int32 [B], Tp): the
    batch cut at its longest length Tp -- teacher_T, the feeder's host-side figure (log entry `teacher_T`), or, without
    one, a read of the device"""
    Tp = int(rows[:, 0].max()) if teacher_T is None else int(teacher_T)
    return rows[:, 1:1 + Tp].contiguous(), rows[:, 0].to(torch.int32), Tp


def teacher_cosine_mask(teacher, rows, teacher_T=None):
    """SimilarityCalculator.bert_embedd (supcon_utils.py:140-159) on the device from the 2n teacher rows (captions, then
    the translations drawn): the mean hidden state over ALL positions of the batch padded to its longest text, unit
    rows (eps 1e-8), caption i against translation j, unit diagonal -> [n, n].  Under data parallelism each rank pads
    to its own longest text (the reference's per-process semantics), the mean vectors are gathered in the sample order
    of global_supcon_views and every rank builds the global [world n, world n] mask."""
    ids, lens, _ = teacher_inputs(rows, teacher_T)
    means = global_supcon_means(teacher.sentence_means(ids, lens), rows.shape[0] // 2)
    return cosine_mask_from_means(means)


def teacher_bertscore_mask(teacher, rows, layer, baseline, teacher_T=None):
    """SimilarityCalculator.bert_score (supcon_utils.py:170-182) on the device from the 2n teacher rows (captions, then
    the translations drawn): the teacher's hidden_states[layer] of every text, rows to unit length, and
    teacher.bertscore_mask's F1 of caption i against translation j with a unit diagonal -> [n, n].  The reference scores
    each pair alone; here the batch is padded to its longest text and no padded position enters a score, so the mask
    does not depend on the padding.  Under data parallelism each rank's states are zero-padded to the rows' fixed width
    (--max_token_length), gathered in the sample order of global_supcon_views (ddp.global_supcon_states) and every rank
    builds the global [world n, world n] mask."""
    ids, lens, Tp = teacher_inputs(rows, teacher_T)
    states = normalize_states_(teacher(ids, lens, layer=layer))
    n, width = rows.shape[0] // 2, rows.shape[1] - 1
    if ddp_world() > 1 and Tp < width:
        padded = states.new_zeros(2 * n, width, states.shape[2])
        padded[:, :Tp] = states
        states = padded
    xa, la, xb, lb = global_supcon_states(states, lens, n)
    return bertscore_mask_unit(xa, la, xb, lb, baseline)


def supcon_step(model, opt, red, world, batch, words=None, teacher_T=None, bert_score=None, watch=None):
    """models/SupConLoss/supcon_utils.py:270-294: MLM loss over both views + SupCon(split_feat(feat)) (called without
    a mask => SimCLR, :287); under DDP the views of all ranks are gathered first.  Returns (loss, pred, stats).
    With `words` (--supcon_mask jaccard: the table's WordSets on the device) the batch is the feeder's 6-tuple and the
    loss is the call the reference leaves in a comment, supcon_loss(feat, mask=mask) with buildMask's Jaccard matrix
    (:276-287): caption of sample i against the translation sample j drew.  When `words` is a data.CaptionEmbeddings
    (--supcon_mask embeddings) the mask is the cosine of the two texts' sentence embeddings instead, as
    sentence_trans(caption, aug) gives it (:162-168).  Under DDP the (row, column) pairs of all
    ranks are gathered and every rank builds the global mask, in the sample order of the gathered features; gather and
    mask launch go on the step's stream.  When `words` is a teacher.BertTeacher (--supcon_mask cosine) the batch's sixth
    element holds the teacher's ids of caption and translation and the mask is teacher_cosine_mask's; teacher_T is the
    feeder's host-side longest length.  With bert_score = (layer, baseline) beside the teacher (--supcon_mask bert_score)
    the same ids give teacher_bertscore_mask's BERTScore F1 mask instead (:170-182)."""
    img, ids, seg, mask, tgt = batch[:5]
    opt.zero_grad()
    logits, feat = model(img, ids, seg, mask)
    loss_mlm, pred, stats = mlm_loss(logits, tgt)
    bsz = img.shape[0] // 2                        # supcon_utils.py:284 (2 = n_views)
    feat = global_supcon_views(feat, bsz)          # = split_feat(feat, bsz) on one rank; global negatives under DDP
    if words is None:
        loss = loss_mlm + supcon_loss(feat)        # 2N*world rows: the tiled kernel has no size cap
    elif isinstance(words, BertTeacher) and bert_score is not None:
        loss = loss_mlm + supcon_loss(feat, mask=teacher_bertscore_mask(words, batch[5], bert_score[0], bert_score[1], teacher_T))
    elif isinstance(words, BertTeacher):
        loss = loss_mlm + supcon_loss(feat, mask=teacher_cosine_mask(words, batch[5], teacher_T))
    else:
        rows, cols = global_supcon_pairs(*batch[5])
        build_mask = embedding_mask if isinstance(words, D.CaptionEmbeddings) else jaccard_mask
        pos = build_mask(words, rows, torch.zeros_like(cols), rows, cols)
        loss = loss_mlm + supcon_loss(feat, mask=pos)
    _update(loss, model, opt, red, world, watch=watch)
    return loss, pred, stats


def vqa_forward(model, batch, group=None, cache=None):
    """logits of a VQA batch; group (--group_by_image): batch[0] holds each image once and group[b] names the image of
    question b (Model.forward_grouped); cache (--cache_tokens): batch[0] is the host pair (index, view) into that
    TokenCache instead of images (Model.forward_cached)"""
    if cache is not None:
        return model.forward_cached(cache, batch[0][0], batch[0][1], *batch[1:4])[0]
    if group is None:
        return model(*batch[:4])[0]                     # utils.py:646
    return model.forward_grouped(batch[0], group, *batch[1:4])[0]


def synthetic_vqa_grouped(args, ctx, seed, C, smooth=False):
    """the synthetic batch of --group_by_image: --batch_size questions, four of each image as in VQA-Med 2019 (the last
    image takes the rest), in the layout the grouped feeder hands out: (img, ids, seg, mask, target[, category], group)"""
    B = args.batch_size
    counts = [4] * (B // 4) + ([B % 4] if B % 4 else [])
    img, group, ids, seg, mask, tgt = synth.vqa_grouped_batch(len(counts), counts, args.max_position_embeddings, args.image_size,
                                                              args.emb_vocab, C, seed=seed, device=ctx.dev)
    cat = (synth.vqa_categories(B, C, seed=seed, device=ctx.dev),) if smooth else ()
    return (img, ids, seg, mask, tgt) + cat + (group,)


def vqa_step(model, opt, red, world, batch, crit, clip=False, scaler=None, group=None, watch=None, cache=None):
    """vqamed2019/utils.py:633-673: logits, _, _ = model(...); loss = criterion(logits, target); backward;
    optional clip_grad_norm_(1.0) (:663-664); Adam; pred = softmax(1).argmax(1).
    With a scaler (--mixed_precision) the reference's sequence of utils.py:641-657: autocast
    forward + loss; scaler.scale(loss) is computed and DISCARDED; the backward is unscaled; the clip acts on those
    gradients; scaler.step then unscales them by 1/scale all the same (and skips on a non-finite gradient).
    A 6-tuple batch (--smoothing) ends with the category ids and the loss is criterion(logits, target, category)
    (utils.py:648-649; also under a scaler, where the reference's call at :644 lacks the argument and raises).
    group: the step of --group_by_image (vqa_forward); `batch` is then without its last element, the group itself.
    cache: the step of --cache_tokens (vqa_forward); batch[0] is then (index, view) instead of images."""
    tgt = batch[4]
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16, enabled=scaler is not None):
        logits = vqa_forward(model, batch, group, cache)
        loss = crit(logits, tgt, batch[5]) if len(batch) == 6 else crit(logits, tgt)
    _update(loss, model, opt, red, world, scaler, scaled_backward=False, clip=clip, watch=watch)   # utils.py:651: the scaled loss is not used
    return loss, logits.detach().softmax(1).argmax(1)


# ----------------------------------------------------------------------------------------- the pre-training loops
@torch.no_grad()
def validate(ctx, model, batches, value, amp=False):
    """The validation loop of every mode: eval mode, no gradients, value(batch) -> host numbers (loss, #targets, #correct)
    of one batch, computed under fp16 autocast when amp.  -> (mean of the per-batch losses, averaged over the ranks;
    accuracy in percent over this rank's batches)"""
    model.eval()
    vl, nm, nc, steps = 0.0, 0, 0, 0
    for batch in batches:
        with torch.autocast("cuda", dtype=torch.float16, enabled=amp):
            s = value(batch)
        vl, nm, nc, steps = vl + s[0], nm + s[1], nc + s[2], steps + 1
    return ctx.mean(vl / max(steps, 1)), 100.0 * nc / max(nm, 1)


def pretrain(args, ctx, mode, model, opt, sched, batches, step, val, line, rank_mean=True, watch=None):
    """The epoch loop of mlm, distill and supcon (roco_train.py:155-197, roco_supcon_train.py:168-202).  A mode supplies
    batches(epoch) -> the epoch's train batches, step(batch) -> host numbers (loss, #targets, #correct) of one training
    step, val(epoch) -> (validation loss, accuracy) and the tail of its epoch line, a format string over tl, ta, vl, va.
    rank_mean=False is synthetic SupCon's line: this rank's loss sum over --steps_per_epoch.  watch: the loop's Watcher
    (--watch), told the epoch and flushed at the end of each.  -> best validation loss"""
    start, kept = maybe_resume(args, model, opt, sched, mode)
    best = kept.get("best", float("inf"))
    for epoch in range(start, args.epochs):
        model.train()
        tl, nm, nc, steps = 0.0, 0, 0, 0
        if watch is not None:
            watch.epoch = epoch
        for batch in batches(epoch):
            s = step(batch)
            tl, nm, nc, steps = tl + s[0], nm + s[1], nc + s[2], steps + 1
        if watch is not None:
            watch.flush()
        with averaged(args, opt):        # --ema_decay: the averaged weights are what is validated
            vl, va = val(epoch)
        sched.step(vl)
        if (epoch + 1) % 5 == 0 and ctx.rank == 0:
            save_recorder(args, epoch, model, opt, sched, mode, {"best": min(best, vl)})
        tl = ctx.mean(tl / max(steps, 1)) if rank_mean else tl / args.steps_per_epoch
        if ctx.rank == 0:
            print(f"Epoch {epoch + 1}/{args.epochs} Learning rate: {opt.param_groups[0]['lr']:.7f}, "
                  + line.format(tl=tl, ta=100.0 * nc / max(nm, 1), vl=vl, va=va), flush=True)
            if vl < best:
                with averaged(args, opt):    # ... and saved
                    save_model(args, model)
        best = min(best, vl)
    if watch is not None:
        watch.close()
    return best


MLM_LINE = "Train loss: {tl:.4f}, Train acc: {ta:.4f} ,Val loss: {vl:.4f}, Val acc: {va:.4f}"   # roco_train.py:190


def validate_mlm(args, ctx, model, fd, epoch, amp=False):
    """-> (loss, accuracy) over the validation feeder, or over synthetic batches without one.  amp: under fp16 autocast
    (mlm --mixed_precision, roco_utils.py:310-311); SupCon validates in fp32"""
    def value(batch):
        out = model(*batch[:4])
        return mlm_loss(out[0] if isinstance(out, tuple) else out, batch[4])[2].tolist()
    synthetic = (synthetic_roco(args, ctx, sd) for sd in val_seeds(args, ctx.rank))
    return validate(ctx, model, epoch_batches(fd, epoch, synthetic), value, amp)


def run_mlm(args):
    ctx = Ctx(args)
    args.dataset, args.task = "roco", "MLM"
    model, opt, sched, red = build(args, ctx)
    scaler = GradScaler() if args.mixed_precision else None
    tr_fd, va_fd = roco_feeders(args, ctx) if args.data_dir else (None, None)
    watch = make_watcher(args, ctx, "mlm", model)
    return pretrain(
        args, ctx, "mlm", model, opt, sched, line=MLM_LINE, watch=watch,
        batches=lambda epoch: epoch_batches(tr_fd, epoch, (synthetic_roco(args, ctx, sd) for sd in train_seeds(args, ctx, epoch))),
        step=lambda batch: mlm_step(model, opt, red, ctx.world, batch, scaler=scaler, watch=watch)[2].tolist(),   # per-step host sync, as roco_utils.py:267
        val=lambda epoch: validate_mlm(args, ctx, model, va_fd, epoch, amp=args.mixed_precision))


# ----------------------------------------------------------------------------------------- distillation
def distill_feeders(args, ctx):
    """(train feeder, validation feeder, train teacher states, validation teacher states): the ROCO tree with the MLM
    transforms (roco_train.py:98-118); the text of an item is the teacher's own tokens (data.TeacherStates.batch) and
    the fifth tensor of a batch is int64 [B, 2] = (start, count).  Both tables of states are uploaded once."""
    out = []
    for split, path in (("train", args.teacher_states), ("validation", args.val_teacher_states)):
        table = D.roco_table(args.data_dir, split)
        teacher = D.TeacherStates.from_file(path, table)
        teacher.check_vocab(args.emb_vocab)
        if teacher.dim != args.hidden_size:
            raise ValueError(f"{path}: the teacher's states are {teacher.dim} wide, --hidden_size is {args.hidden_size}")
        ds = D.DistillDataset(table, teacher, args.num_vis, args.max_position_embeddings)
        out.append((feeder(args, ctx, ds, split == "train", D.ROCO_AUG), teacher.to(ctx.dev)))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def online_distill_feeders(args, ctx):
    """(train feeder, validation feeder, teacher, teacher): the same tree with the teacher run per batch.  The workers
    tokenise with the teacher's WordPiece (data.OnlineDistillDataset); the fifth tensor of a batch is int64
    [B, 1 + --max_token_length] = (length, the teacher's input ids)."""
    teacher, tok = load_teacher(args, ctx), teacher_tokenizer(args)
    if teacher.hidden != args.hidden_size:
        raise ValueError(f"{args.teacher_weights}: the teacher's states are {teacher.hidden} wide, --hidden_size is {args.hidden_size}")
    if len(tok.vocab) > args.emb_vocab:
        raise ValueError(f"{args.teacher_vocab_file}: {len(tok.vocab)} tokens, the student's embedding table has "
                         f"{args.emb_vocab} rows (--emb_vocab must be the teacher's vocabulary size)")
    if len(tok.vocab) > teacher.vocab:
        raise ValueError(f"{args.teacher_vocab_file}: {len(tok.vocab)} tokens, the teacher's embedding table has {teacher.vocab} rows")
    fds = []
    for split in ("train", "validation"):
        ds = D.OnlineDistillDataset(D.roco_table(args.data_dir, split), tok, args.num_vis, args.max_position_embeddings,
                                    args.max_token_length)
        fds.append(feeder(args, ctx, ds, split == "train", D.ROCO_AUG))
    return fds[0], fds[1], teacher, teacher


def online_distill_targets(teacher, rows, teacher_T=None):
    """run the teacher on a batch's rows [B, 1 + L] -> (table [B * Tp, hidden], start int64 [B], count int32 [B]) in the
    form distill_loss reads: sample b's caption states are rows b * Tp + 1 .. of the teacher's output (CLS dropped),
    len - 2 of them (SEP dropped too) -- roco_utils.py:127-129"""
    ids, lens, Tp = teacher_inputs(rows, teacher_T)
    states = teacher(ids, lens)
    B = ids.shape[0]
    start = torch.arange(B, dtype=torch.int64, device=ids.device) * Tp + 1
    return states.view(B * Tp, teacher.hidden), start, lens - 2


def synthetic_teacher_rows(batch, num_vis=5):
    """teacher rows [B, 1 + L] for a synthetic distillation batch (synth.distill_batch): the teacher sees [CLS], the
    caption ids the student was given and [SEP], all of which the student's row already holds; L = T - num_vis - 1"""
    ids, count = batch[1], batch[5]
    first = num_vis + 2
    n_max = ids.shape[1] - first - 1
    lens = count.to(torch.int64).clamp(max=n_max) + 2
    return torch.cat([lens[:, None], ids[:, :1], ids[:, first:]], 1).contiguous()


def distill_targets(batch):
    """(start int64 [B], count int32 [B]) of a batch: its last two tensors, or the columns of a fed batch's [B, 2]"""
    if len(batch) == 6:
        return batch[4], batch[5]
    return batch[4][:, 0].contiguous(), batch[4][:, 1].to(torch.int32)


def distill_step(model, opt, red, world, batch, teacher, scaler=None, num_vis=5, teacher_T=None, watch=None):
    """pretrain/roco_utils.py:214-247 with task 'distillation' (:230-231, 237-238): zero_grad -> forward (the model
    returns h) -> nn.MSELoss against the teacher's states -> backward -> (gradient all-reduce) -> Adam.  batch =
    (img, ids, seg, mask, start, count) or (img, ids, seg, mask, [B, 2] of both); teacher = the resident table of
    states.  Returns the loss.  With a scaler (--mixed_precision, :224-245): autocast forward, the loss in fp32, scaled
    backward, scaler.step after the all-reduce, scaler.update.
    When `teacher` is a teacher.BertTeacher the batch's fifth tensor holds the teacher's input rows [B, 1 + L]
    (data.OnlineDistillDataset) and the table is the teacher's output for this batch, computed first
    (online_distill_targets); teacher_T is the feeder's host-side longest length.  The loss call is the same."""
    img, ids, seg, mask = batch[:4]
    if isinstance(teacher, BertTeacher):
        teacher, start, count = online_distill_targets(teacher, batch[4], teacher_T)
    else:
        start, count = distill_targets(batch)
    opt.zero_grad()
    with torch.autocast("cuda", dtype=torch.float16) if scaler is not None else contextlib.nullcontext():
        loss = distill_loss(model(img, ids, seg, mask), teacher, start, count, num_vis)
    _update(loss, model, opt, red, world, scaler, watch=watch)
    return loss


def distill_batches(args, ctx, fd, teacher, epoch, seeds):
    """(batch, teacher table) of one epoch: the feeder's batches beside the resident table, or one synthetic batch per
    seed, each with a table of its own"""
    if fd is not None:
        return ((b, teacher) for b in epoch_batches(fd, epoch, None))
    syn = (synth.distill_batch(args.batch_size, args.max_position_embeddings, args.image_size, args.emb_vocab,
                               args.hidden_size, seed=sd, device=ctx.dev, num_vis=args.num_vis) for sd in seeds)
    if teacher is None:
        return syn
    # --teacher_layers: the seeded random teacher over the synthetic caption ids instead of the batch's random table
    return ((b[:4] + (synthetic_teacher_rows(b, args.num_vis),), teacher) for b, _table in syn)


def run_distill(args):
    ctx = Ctx(args)
    args.dataset, args.task = "roco", "distillation"
    model, opt, sched, red = build(args, ctx)
    scaler = GradScaler() if args.mixed_precision else None
    tr_fd, va_fd, tr_teacher, va_teacher = (None,) * 4
    if args.data_dir:
        tr_fd, va_fd, tr_teacher, va_teacher = (online_distill_feeders if args.teacher_weights else distill_feeders)(args, ctx)
    elif args.teacher_layers:
        tr_teacher = va_teacher = BertTeacher.random(args.teacher_layers, args.hidden_size, 4 * args.hidden_size, args.emb_vocab,
                                                     max(args.max_position_embeddings, 2), seed=args.seed).to(ctx.dev)

    watch = make_watcher(args, ctx, "distill", model)

    def longest(fd, pair):       # the fed batch's longest teacher input, from the feeder's host-side log; synthetic: all of L
        return fd.log[-1]["teacher_T"] if fd is not None else pair[0][4].shape[1] - 1

    def step(pair):                                               # per-step host sync, as roco_utils.py:267
        tT = longest(tr_fd, pair) if isinstance(pair[1], BertTeacher) else None
        return float(distill_step(model, opt, red, ctx.world, *pair, scaler=scaler, num_vis=args.num_vis, teacher_T=tT,
                                  watch=watch).detach()), 0, 0

    def val_value(pair):    # roco_utils.py:292-372 with task 'distillation': no accuracy (total_acc is None)
        if isinstance(pair[1], BertTeacher):
            table, start, count = online_distill_targets(pair[1], pair[0][4], longest(va_fd, pair))
            return float(distill_loss(model(*pair[0][:4]), table, start, count, args.num_vis)), 0, 0
        return float(distill_loss(model(*pair[0][:4]), pair[1], *distill_targets(pair[0]), args.num_vis)), 0, 0

    return pretrain(
        args, ctx, "distill", model, opt, sched, step=step, watch=watch, line="Train loss: {tl:.4f}, Val loss: {vl:.4f}",   # roco_train.py:190
        batches=lambda epoch: distill_batches(args, ctx, tr_fd, tr_teacher, epoch, train_seeds(args, ctx, epoch)),
        val=lambda epoch: validate(ctx, model, distill_batches(args, ctx, va_fd, va_teacher, epoch, val_seeds(args, ctx.rank)),
                                   val_value, amp=args.mixed_precision))


# ----------------------------------------------------------------------------------------- MLM + SupCon
def run_supcon(args):
    ctx = Ctx(args)
    args.dataset, args.task, args.supcon = "roco", "MLM", True
    model, opt, sched, red = build(args, ctx)
    n = args.batch_size // 2                      # roco_supcon_train.py:137: the loader yields bs//2 pairs
    if n < 1:
        raise ValueError("--batch_size must be >= 2 (two views per sample)")
    # (fed batches come in process_tensors' layout: data.collate_supcon)
    tr_fd, va_fd, words = roco_supcon_feeders(args, ctx, n) if args.data_dir else (None, None, None)
    bert_score = ((args.bert_score_layer, args.bert_score_baseline)
                  if getattr(args, "supcon_mask", "none") == "bert_score" else None)
    watch = make_watcher(args, ctx, "supcon", model)

    def synthetic(epoch):
        for sd in train_seeds(args, ctx, epoch):
            a, b = synthetic_roco(args, ctx, sd, n), synthetic_roco(args, ctx, sd + 1, n)
            yield process_tensors((a[0], b[0]), a[1], b[1], a[2], a[3], a[4], b[4])

    def step(batch):
        tT = tr_fd.log[-1]["teacher_T"] if isinstance(words, BertTeacher) else None   # the feeder's host-side longest length
        loss, _, stats = supcon_step(model, opt, red, ctx.world, batch, words=words, teacher_T=tT, bert_score=bert_score,
                                     watch=watch)
        # fed: the MLM accuracy train_one_epoch returns (supcon_utils.py:296-318); synthetic: `stats` stays on the device
        return (float(loss.detach()), *(stats.tolist()[1:] if tr_fd is not None else (0, 0)))

    return pretrain(
        args, ctx, "supcon", model, opt, sched, rank_mean=tr_fd is not None, watch=watch,
        batches=lambda epoch: epoch_batches(tr_fd, epoch, synthetic(epoch)), step=step,
        val=lambda epoch: validate_mlm(args, ctx, model, va_fd, epoch),
        line=MLM_LINE if tr_fd is not None else "Train loss: {tl:.4f}, Val loss: {vl:.4f}, Val acc: {va:.4f}")   # roco_supcon_train.py:193


# ----------------------------------------------------------------------------------------- VQA-Med-2019
def plain_criterion(args):
    """--loss: ASLSingleLabel or cross entropy (vqamed2019/train.py:170-174, eval.py:126-130)"""
    return (lambda lg, t: asl_loss(lg, t)) if args.loss == "ASLSingleLabel" else (lambda lg, t: mlm_loss(lg, t)[0])


def vqa_criterion(args, ctx, train_rows=None):
    """vqamed2019/train.py:164-174: --smoothing is tested first (then --loss is not consulted): LabelSmoothByCategory
    over the WHOLE train table (every rank builds the same table, whatever its shard), with the flag's value (the
    reference drops it and always smooths with 0.1); else ASLSingleLabel or cross entropy.  Without --data_dir the
    train table is synth.vqa_category_rows."""
    if getattr(args, "smoothing", None):
        rows = synth.vqa_category_rows(args.num_classes) if train_rows is None else train_rows
        return CategorySmoothing(rows, args.num_classes, args.smoothing).to(ctx.dev)
    return plain_criterion(args)


class SyntheticTokenSource:
    """--cache_tokens without --data_dir: a synthetic train set of --cache_images images and a validation set of
    --val_steps x --batch_size, both from fixed seeds (chunks of --batch_size images, synth.vqa_batch), encoded once into
    two TokenCaches.  View 0 of an image is the image as it stands (a synthetic image is already what the evaluation
    transform hands out); view v >= 1 is DeviceAugment's training chain with VQA_AUG on the image's 8-bit pixels, its
    parameters drawn per image from (seed, image, view) alone.  A train step draws --batch_size (image, question, answer)
    triples from its seed and a view per sample from (seed, epoch, batch, rank); a validation batch is view 0 of the images
    of the uncached synthetic validation batch of the same seed, with questions and answers drawn from that seed without
    the images (other draws than the uncached batch's: its generator makes the images first)."""

    def __init__(self, args, ctx, model, n_classes, smooth=False):
        from .augment import DeviceAugment, sample_params
        from .tokens import TokenCache
        self.args, self.ctx, self.C, self.smooth = args, ctx, n_classes, smooth
        B = args.batch_size
        self.N = args.cache_images or 8 * B
        self.K = args.cache_views or 1
        self.train = TokenCache(model, self.N, self.K)
        self.val = TokenCache(model, max(1, args.val_steps) * B, 1)
        aug = DeviceAugment(size=args.image_size, train=True, device=ctx.dev, **D.VQA_AUG) if self.K > 1 else None
        for lo in range(0, self.N, B):
            n = min(B, self.N - lo)
            img = self.images("train", lo, n)
            self.train.fill(range(lo, lo + n), img.to(ctx.dev), 0)
            if aug is None:
                continue
            pixels = list(self.pixels(img))
            for v in range(1, self.K):
                params = [sample_params(1, args.image_size, generator=torch.Generator().manual_seed(
                    D.mix_seed(args.seed, lo + i, v, 0x746F6B)), **D.VQA_AUG)[0] for i in range(n)]
                self.train.fill(range(lo, lo + n), aug(pixels, params=params), v)
        for i in range(args.val_steps):
            self.val.fill(range(i * B, (i + 1) * B), self.images("val", i * B, B).to(ctx.dev), 0)

    def images(self, split, lo, n):
        """images lo .. lo + n - 1 of a split (lo a multiple of --batch_size) -> fp32 [n, 3, S, S] on the host"""
        a = self.args
        seed = (a.seed + 15485863 + lo) if split == "train" else list(val_seeds(a))[lo // a.batch_size]
        return synth.vqa_batch(n, a.max_position_embeddings, a.image_size, a.emb_vocab, self.C, seed=seed)[0]

    @staticmethod
    def pixels(img):
        """fp32 [n, 3, S, S] in [-1, 1] -> uint8 [n, S, S, 3], what a decoder would hand to the augment"""
        return ((img + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()

    def text(self, seed, smooth):
        """(ids, seg, mask, target[, category]) of synth.vqa_batch at `seed`, on the device, without its images"""
        a, dev = self.args, self.ctx.dev
        out = synth.vqa_batch(a.batch_size, a.max_position_embeddings, 1, a.emb_vocab, self.C, seed=seed, device=dev)[1:]
        return out + (synth.vqa_categories(a.batch_size, self.C, seed=seed, device=dev),) if smooth else out

    def train_batches(self, epoch):
        a, B = self.args, self.args.batch_size
        for b, sd in enumerate(train_seeds(a, self.ctx, epoch)):
            index = torch.randint(0, self.N, (B,), generator=torch.Generator().manual_seed(D.mix_seed(sd, 0x696478)))
            view = torch.randint(0, self.K, (B,), generator=D.batch_generator(a.seed, epoch, b, self.ctx.rank))
            yield ((index, view),) + self.text(sd, self.smooth)

    def val_batches(self):
        B = self.args.batch_size
        for i, sd in enumerate(val_seeds(self.args)):     # validation is plain cross entropy: no category
            yield ((torch.arange(i * B, (i + 1) * B), torch.zeros(B, dtype=torch.int64)),) + self.text(sd, False)

    def check(self, model):
        self.train.check(model)
        if self.args.val_steps:                           # (--val_steps 0 fills no validation cache)
            self.val.check(model)


class TableTokenSource:
    """--cache_tokens with --data_dir: the distinct images of the VQA-Med train and validation tables, encoded once into
    two TokenCaches (row i = image i of data.image_of_rows), through the DeviceFeeder / DeviceAugment path in file order:
    view 0 is the evaluation transform, view v >= 1 the training augmentation with data.view_params(seed, image, v).
    After the fill no image is decoded: the worker processes tokenise only (data.VqaTextDataset), a batch carries the
    cache rows of its questions on the host, and every sample of a train step takes a view drawn from
    (seed, epoch, batch, rank).  Validation reads view 0 of its own cache in table order."""

    def __init__(self, args, ctx, model, tok, tabs, categories=None):
        from .tokens import TokenCache
        self.args, self.ctx = args, ctx
        self.K = args.cache_views or 1
        T = args.max_position_embeddings
        self.tr_ds = D.VqaTextDataset(tabs["train"], tok, T, categories=categories)
        self.va_ds = D.VqaTextDataset(tabs["val"], tok, T)
        self.train = TokenCache(model, len(self.tr_ds.paths), self.K)
        self.val = TokenCache(model, len(self.va_ds.paths), 1)
        for split, cache, views in (("train", self.train, self.K), ("val", self.val, 1)):
            images = D.VqaImageDataset(tabs[split])
            for v in range(views):
                host = D.ViewLoader(images, args.batch_size, v, seed=args.seed, num_workers=args.num_workers, aug=D.VQA_AUG,
                                    size=args.image_size)
                fd = D.DeviceFeeder(host, ctx.dev, train=v > 0, depth=args.feeder_depth)
                for batch in fd:
                    cache.fill(fd.log[-1]["index"], batch[0], v)
                del fd, host
        loader = lambda ds, train: D.HostLoader(ds, args.batch_size, shuffle=train, seed=args.seed, rank=ctx.rank,   # noqa: E731
                                                world=ctx.world, num_workers=args.num_workers, size=args.image_size)
        self.tr_host, self.va_host = loader(self.tr_ds, True), loader(self.va_ds, False)

    def _batches(self, host, epoch, views, category):
        dev = self.ctx.dev
        host.set_epoch(epoch)
        for batch, _params, meta in host:
            n = batch["image"].shape[0]
            if views > 1:
                view = torch.randint(0, views, (n,), generator=D.batch_generator(self.args.seed, epoch, meta["batch"], self.ctx.rank))
            else:
                view = torch.zeros(n, dtype=torch.int64)
            out = ((batch["image"], view),) + tuple(batch[k].to(dev, non_blocking=True) for k in ("ids", "seg", "mask", "target"))
            yield out + (batch["category"].to(dev, non_blocking=True),) if category else out

    def train_batches(self, epoch):
        return self._batches(self.tr_host, epoch, self.K, self.tr_ds.categories is not None)

    def val_batches(self):
        return self._batches(self.va_host, 0, 1, False)

    def check(self, model):
        self.train.check(model)
        self.val.check(model)


def run_vqa(args):
    ctx = Ctx(args)
    args.dataset, args.task = "VQA-Med", "MLM"
    tr_fd = va_fd = None
    smooth = bool(getattr(args, "smoothing", None))
    # --group_by_image: a batch holds each image once; its last element is the host map `group`
    grouped = bool(getattr(args, "group_by_image", False))
    split = (lambda b: (b[:-1], b[-1])) if grouped else (lambda b: (b, None))
    if args.data_dir:                                   # train.py:100-105: the classes are the answers of the tables
        tok = tokenizer(args)
        _cols, tabs, idx2ans = D.vqa_tables(args.data_dir)
        args.num_classes = len(idx2ans)
        crit = vqa_criterion(args, ctx, tabs["train"])
        DS = D.VqaGroupedDataset if grouped else D.VqaDataset     # grouped: an item is an image with all of its questions
        if not getattr(args, "cache_tokens", False):             # (--cache_tokens reads the tables itself, below)
            tr_ds = DS(tabs["train"], tok, args.max_position_embeddings, categories=crit.cat2idx if smooth else None)
            tr_fd = feeder(args, ctx, tr_ds, True, D.VQA_AUG, category=smooth, grouped=grouped)
            va_fd = feeder(args, ctx, DS(tabs["val"], tok, args.max_position_embeddings), False, grouped=grouped)
    else:
        crit = vqa_criterion(args, ctx)
    C = args.num_classes
    model, opt, sched, red = build(args, ctx, n_classes=C)
    scaler = GradScaler() if args.mixed_precision else None
    watch = make_watcher(args, ctx, "vqa", model)
    T, B = args.max_position_embeddings, args.batch_size
    src = tr_cache = va_cache = None

    def synthetic_train(epoch):
        for sd in train_seeds(args, ctx, epoch):
            if grouped:
                yield synthetic_vqa_grouped(args, ctx, sd, C, smooth)
                continue
            batch = synth.vqa_batch(B, T, args.image_size, args.emb_vocab, C, seed=sd, device=ctx.dev)
            yield batch + (synth.vqa_categories(B, C, seed=sd, device=ctx.dev),) if smooth else batch

    def val_value(batch):                               # utils.py:708-715, 673
        batch, group = split(batch)
        logits = vqa_forward(model, batch, group, va_cache)
        return float(crit(logits, batch[4])), batch[4].shape[0], int((logits.softmax(1).argmax(1) == batch[4]).sum())
    # (vqamed2019/train.py itself has no recorder / --resume; kept here like the two pre-training loops)
    start, kept = maybe_resume(args, model, opt, sched, "vqa")
    # --cache_tokens: batch[0] is (index, view) into a TokenCache, filled here, once, from the
    # weights the run trains with (after --resume has loaded them)
    if getattr(args, "cache_tokens", False):
        if args.data_dir:
            src = TableTokenSource(args, ctx, model, tok, tabs, crit.cat2idx if smooth else None)
        else:
            src = SyntheticTokenSource(args, ctx, model, C, smooth)
        tr_cache, va_cache = src.train, src.val
    best_loss, best_acc1 = kept.get("best_loss", float("inf")), kept.get("best_acc1", 0.0)
    best_acc2, counter = kept.get("best_acc2", 0.0), kept.get("counter", 0)
    for epoch in range(start, args.epochs):
        model.train()
        if src is not None:
            src.check(model)    # a cache is only as good as the backbone it was filled from
        if smooth:
            crit.train()        # every epoch: the reference leaves the criterion in eval mode after its first validate
        tl, steps = 0.0, 0
        if watch is not None:
            watch.epoch = epoch
        for batch in epoch_batches(tr_fd, epoch, synthetic_train(epoch) if src is None else src.train_batches(epoch)):
            batch, group = split(batch)
            loss, _ = vqa_step(model, opt, red, ctx.world, batch, crit, clip=args.clip, scaler=scaler, group=group,
                               watch=watch, cache=tr_cache)
            tl, steps = tl + float(loss.detach()), steps + 1
        if watch is not None:
            watch.flush()
        if smooth:
            crit.eval()         # utils.py:693: validation is plain cross entropy
        if src is not None:
            synthetic = src.val_batches()
        elif grouped:
            synthetic = (synthetic_vqa_grouped(args, ctx, sd, C) for sd in val_seeds(args))
        else:
            synthetic = (synth.vqa_batch(B, T, args.image_size, args.emb_vocab, C, seed=sd, device=ctx.dev) for sd in val_seeds(args))
        with averaged(args, opt):        # --ema_decay: the averaged weights are what is validated
            vl, acc = validate(ctx, model, epoch_batches(va_fd, epoch, synthetic), val_value, amp=args.mixed_precision)
        sched.step(vl)
        if ctx.rank == 0:
            print(f"Epoch {epoch + 1}/{args.epochs} lr {opt.param_groups[0]['lr']:.7f} train_loss {tl / max(steps, 1):.4f} "
                  f"val_loss {vl:.4f} val_total_acc {acc:.2f}", flush=True)
        if ctx.rank == 0 and (vl < best_loss or acc > best_acc1):
            with averaged(args, opt):            # ... and saved: eval and gradcam load these files as they are
                if vl < best_loss:               # train.py:264-268 "save by val loss"
                    save_model(args, model, "_loss")
                if acc > best_acc1:              # train.py:270-276 "save by accuracy in val"
                    save_model(args, model)
        best_loss = min(best_loss, vl)
        best_acc1 = max(best_acc1, acc)
        expired = False
        if best_acc1 > best_acc2:                # train.py:288-296 early stop
            counter, best_acc2 = 0, best_acc1
        else:
            counter += 1
            expired = counter > args.counter
        if (epoch + 1) % 5 == 0 and ctx.rank == 0:
            save_recorder(args, epoch, model, opt, sched, "vqa",
                          dict(best_loss=best_loss, best_acc1=best_acc1, best_acc2=best_acc2, counter=counter))
        if expired:
            if ctx.rank == 0:
                print("Counter expired, finishing.")
            break
    if watch is not None:
        watch.close()
    return best_loss


# ----------------------------------------------------------------------------------------- VQA-Med-2019 test-set run
def run_eval(args):
    """vqamed2019/eval.py:99-180: Model(args) -> classifier[2] = Linear(hidden, num_classes) -> load_state_dict(model_dir)
    -> test() over the test split (batch_size, shuffle False) -> print acc / bleu -> <model_name>_preds.csv and
    <model_name>_res.txt in save_dir.  The test split is synthetic (mmvqa_amd.synth.vqa_test_table + vqa_batch: the
    dataset and its tokenizer are not in the image); everything after the loader is the reference's sequence."""
    ctx, model, cols, rows, idx2ans, batches = eval_setup(args)
    if getattr(args, "smoothing", None):     # eval.py:124-125; test() puts it in eval mode (utils.py:772): cross entropy
        crit = LabelSmoothing(args.smoothing)
    else:
        crit = plain_criterion(args)
    # --group_by_image: the loader's order is the images' first appearance with an image's questions together (the batches'
    # `index`); the metrics take the categories in that order, the files the predictions back in the table's
    grouped = bool(getattr(args, "group_by_image", False))
    order = [r for _, idx in D.group_rows_by_image(rows) for r in idx] if grouped else list(range(len(rows)))
    cats = [rows[r][3] for r in order]
    with torch.autocast("cuda", dtype=torch.float16, enabled=args.mixed_precision):   # utils.py:786-792
        test_loss, predictions, acc, bleu = evaluate.test(batches, model, crit, cats, idx2ans, category=args.category,
                                                          grouped=grouped)
    if grouped:
        in_table_order = np.empty_like(predictions)
        in_table_order[np.asarray(order)] = predictions
        predictions = in_table_order
    model_name = (args.model_dir or args.run_name).split("/")[-1]               # eval.py:68
    if ctx.rank == 0:
        paths = evaluate.write_test_files(rows, cols, predictions, idx2ans, args.save_dir, model_name)   # eval.py:171-178
        print("test_loss", float(test_loss))
        print("acc", acc)
        print("bleu", bleu)
        print("wrote", *paths)
    return test_loss, acc, bleu


def eval_setup(args):
    """What the test-set run and `gradcam` share: the model with its checkpoint (eval.py:99-112) and the test split in
    file order -> (ctx, model, columns, rows, idx2ans, batches)"""
    ctx = Ctx(args)
    args.dataset, args.task = "VQA-Med", "MLM"
    if args.data_dir:                                   # the real test split (vqamed2019/utils.py:51-79)
        tok = tokenizer(args)
        cols, tabs, idx2ans = D.vqa_tables(args.data_dir)
        rows = tabs["test"]
        args.num_classes = len(idx2ans)
    C = args.num_classes
    torch.manual_seed(args.seed)
    model = Model(args)
    model.classifier[2] = torch.nn.Linear(args.hidden_size, C)                     # eval.py:109
    if args.model_dir:
        print("Loading model at ", args.model_dir)
        model.load_state_dict(checkpoint.read_state_dict(args.model_dir))        # eval.py:112
    model.to(ctx.dev)
    B, T = args.batch_size, args.max_position_embeddings
    if not args.data_dir:
        cols, rows, idx2ans = synth.vqa_test_table(args.test_samples, C, seed=args.seed)

    def loader():                                                                # DataLoader(testdataset, batch_size, shuffle=False)
        for lo in range(0, len(rows), B):
            n = min(B, len(rows) - lo)
            img, ids, seg, mask, _ = synth.vqa_batch(n, T, args.image_size, args.emb_vocab, C, seed=args.seed + lo, device=ctx.dev)
            tgt = torch.tensor([r[2] for r in rows[lo:lo + n]], dtype=torch.long, device=ctx.dev)
            yield img, ids, seg, mask, tgt

    grouped = bool(getattr(args, "group_by_image", False))
    if args.data_dir:            # file order, every row on every rank; test() keeps the targets, so they leave the slots
        one = argparse.Namespace(rank=0, world=1, dev=ctx.dev)
        if grouped:              # every image once, with all of its questions: the batches end with the host map `group`
            test_fd = feeder(args, one, D.VqaGroupedDataset(rows, tok, T), False, grouped=True)
            batches = (b[:4] + (b[4].clone(), b[5]) for b in epoch_batches(test_fd, 0, None))
        else:
            test_fd = feeder(args, one, D.VqaDataset(rows, tok, T), False)
            batches = ((img, ids, seg, mask, tgt.clone()) for img, ids, seg, mask, tgt in epoch_batches(test_fd, 0, None))
    elif grouped:                # every synthetic row has an image of its own: the identity map, through the grouped step
        batches = (b + (torch.arange(b[1].shape[0]),) for b in loader())
    else:
        batches = loader()
    return ctx, model, cols, rows, idx2ans, batches


# ----------------------------------------------------------------------------------------- Grad-CAM over the test split
def run_gradcam(args):
    """vqamed2019/grad_cam2.py:99-188 over the whole test split instead of one named image: the model and checkpoint of
    `eval`, one attribution pass per batch (mmvqa_amd.gradcam.grad_cam), <save_dir>/<category>_<image name>.png per
    row (grad_cam2.py:188's naming) and gradcam_index.csv (image, category, question index, target, predicted, valid).
    --method other than gradcam (grad_cam.py:30,65-72) goes through mmvqa_amd.gradcam.attribute and adds a `method` column."""
    import csv
    from PIL import Image
    from . import gradcam as G
    if args.mixed_precision:
        raise SystemExit("gradcam: attribution runs in fp32 (no --mixed_precision)")
    ctx, model, _cols, rows, _idx2ans, batches = eval_setup(args)
    model.eval()
    limit = len(rows) if args.limit is None else min(args.limit, len(rows))
    os.makedirs(args.save_dir, exist_ok=True)
    index, done = [], 0
    extra = [] if args.method == "gradcam" else [args.method]
    for img, ids, seg, mask, tgt in batches:
        if done >= limit:
            break
        if args.method == "gradcam":
            res = G.grad_cam(model, img, ids, seg, mask, target=tgt if args.target == "answer" else None,
                             image_u8=G.image_u8_from_normalised(img))
        else:
            res = G.attribute(model, img, ids, seg, mask, method=args.method, target=tgt if args.target == "answer" else None,
                              image_u8=G.image_u8_from_normalised(img))
        over, pred = res.overlay.cpu().numpy(), res.logits.argmax(1).cpu().tolist()
        target, valid = res.target.cpu().tolist(), res.valid.cpu().tolist()
        for b in range(img.shape[0]):
            if done >= limit:
                break
            path, _q, _a, cat, _m = rows[done]
            name = os.path.splitext(os.path.basename(str(path)))[0]
            out = os.path.join(args.save_dir, f"{cat}_{name}.png")
            if ctx.rank == 0:
                Image.fromarray(over[b], "RGB").save(out)
            index.append([os.path.basename(out), cat, done, target[b], pred[b], valid[b]] + extra)
            done += 1
    p_idx = os.path.join(args.save_dir, "gradcam_index.csv")
    if ctx.rank == 0:
        with open(p_idx, "w", newline="") as f:
            w = csv.writer(f, lineterminator="\n")
            w.writerow(["image", "category", "question_index", "target", "predicted", "valid"] + (["method"] if extra else []))
            w.writerows(index)
        print("wrote", done, "overlays and", p_idx)
    return index


def parse_args(argv=None):
    """-> (mode, args); contradictory options end in argparse's error exit before anything touches the GPU"""
    argv = list(sys.argv[1:] if argv is None else argv)
    mode = argv.pop(0) if argv and argv[0] in ("mlm", "supcon", "distill", "vqa", "eval", "gradcam") else "mlm"
    p = argparse.ArgumentParser(description=f"mmvqa_amd training ({mode})")
    common_args(p)
    if mode in ("mlm", "supcon", "distill"):
        if mode != "distill":
            p.add_argument("--mlm_prob", type=float, default=0.15)
        p.add_argument("--lr", type=float, default=2e-5)
        p.add_argument("--max_position_embeddings", type=int, default=75)
        if mode == "distill":
            p.add_argument("--teacher_states", type=str, default=None, metavar="FILE",
                           help="with --data_dir: an .npz of the teacher's precomputed per-token states of the train "
                                "captions -- names [R], offsets [R + 1], ids [total] (the teacher tokenizer's ids without "
                                "CLS / SEP), states [total, hidden_size]; no teacher is run here")
            p.add_argument("--val_teacher_states", type=str, default=None, metavar="FILE",
                           help="the same for the validation split")
            p.add_argument("--teacher_layers", type=int, default=0, metavar="N",
                           help="without --data_dir: run a seeded random BERT teacher of N layers (--hidden_size wide) over "
                                "the synthetic caption ids instead of a random table of states")
        if mode in ("distill", "supcon"):
            p.add_argument("--teacher_weights", type=str, default=None, metavar="FILE",
                           help="with --data_dir: a local HF BertModel state dict (.bin / .pt / .safetensors), e.g. "
                                "ClinicalBERT: the teacher is run on the GPU per batch (distill: instead of "
                                "--teacher_states; supcon: --supcon_mask cosine)")
            p.add_argument("--teacher_vocab_file", type=str, default=None, metavar="FILE",
                           help="the teacher's WordPiece vocab.txt (with --teacher_weights)")
            p.add_argument("--max_token_length", type=int, default=512,
                           help="the teacher's inputs are truncated to this many tokens, [CLS] and [SEP] included")
            p.add_argument("--teacher_lower_case", action="store_true", default=False,
                           help="lower-case and strip accents before the teacher's WordPiece (default: cased)")
        if mode == "supcon":
            p.add_argument("--con_task", type=str, default="supcon", choices=["simclr", "supcon"])
            p.add_argument("--similarity", type=str, default="sentence_transformers")      # accepted, not read
            p.add_argument("--bert_score", type=str, default=None, choices=["bert", "scibert"])   # accepted; `bert` is refused below
            p.add_argument("--bert_score_layer", type=int, default=None, metavar="N",
                           help="with --supcon_mask bert_score: the teacher's hidden layer whose output is scored, "
                                "hidden_states[N] with N in 1..the checkpoint's depth (default 8, the library's choice "
                                "for allenai/scibert_scivocab_uncased)")
            p.add_argument("--bert_score_baseline", type=float, default=None, metavar="B",
                           help="with --supcon_mask bert_score: rescale F to (F - B) / (1 - B), the library's "
                                "rescale_with_baseline (default 0: no rescaling)")
            p.add_argument("--supcon_mask", type=str, default="none",
                           choices=["none", "jaccard", "embeddings", "cosine", "bert_score"],
                           help="positives of the SupCon loss: none = the other view only (SimCLR, what the reference's "
                                "loop runs); jaccard = caption / back-translation word overlap weights every pair "
                                "(SimilarityCalculator.jaccard); embeddings = the cosine of the two texts' sentence "
                                "embeddings (SimilarityCalculator.sentence_trans) from --caption_embeddings; cosine = "
                                "the cosine of the BERT teacher's mean hidden states of the two texts "
                                "(SimilarityCalculator.bert_embedd), the teacher of --teacher_weights run per batch; "
                                "bert_score = the BERTScore F1 of the two texts (SimilarityCalculator.bert_score, the "
                                "library's greedy matching restated) from the same teacher's --bert_score_layer.  "
                                "Every mask is built on the GPU per batch and needs --data_dir")
            p.add_argument("--caption_embeddings", type=str, default=None, metavar="FILE",
                           help="with --supcon_mask embeddings: an .npz of precomputed sentence embeddings, names [R] "
                                "(image file names) and emb [R, 4, D] (caption and the three translations); no "
                                "encoder is run here")
    else:
        p.add_argument("--lr", type=float, default=1e-4)
        p.add_argument("--max_position_embeddings", type=int, default=28)
        p.add_argument("--loss", type=str, default="CrossEntropyLoss", choices=["CrossEntropyLoss", "ASLSingleLabel"])
        p.add_argument("--smoothing", type=float, default=None,
                       help="label smoothing by question category (LabelSmoothByCategory, vqamed2019/utils.py:1234-1300): the "
                            "train step's target keeps 1 - SMOOTHING and SMOOTHING is spread over the answers of the "
                            "question's category in the train table; validation and test use cross entropy.  Takes "
                            "precedence over --loss (train.py:164).  0.1 is what the reference always uses")
        p.add_argument("--num_classes", type=int, default=1552)
        p.add_argument("--counter", type=int, default=20)
        p.add_argument("--clip", action="store_true", default=False, help="clip_grad_norm_(1.0), utils.py:663-664")
        p.add_argument("--use_pretrained", action="store_true", default=False)      # vqamed2019/train.py:69-72
        p.add_argument("--model_dir", type=str, default=None, help="ROCO-pretrained Model state_dict")
        p.add_argument("--resume_training", action="store_true", default=False)
        p.add_argument("--resume_dir", type=str, default=None, help="fine-tuned Model state_dict to continue from")
        p.add_argument("--category", type=str, default=None, help="eval: one question category only (eval.py:29)")
        p.add_argument("--test_samples", type=int, default=64, help="eval: size of the synthetic test split")
        p.add_argument("--group_by_image", action="store_true", default=False,
                       help="vqa / eval: a batch holds each image once with all of its questions (VQA-Med asks four per "
                            "image), so the CNN backbone runs once per image, forward and backward; --batch_size keeps "
                            "counting questions.  Train-mode BatchNorm then sees each image once per step.  Under data "
                            "parallelism whole batches are dealt to the ranks, so every rank runs as many steps.  Without "
                            "--data_dir: vqa draws four synthetic questions per image; eval's synthetic table has one "
                            "image per question, so the grouped step runs there but shares nothing")
        if mode == "gradcam":
            p.add_argument("--target", type=str, default="answer", choices=["answer", "predicted"],
                           help="the class each map explains: the row's answer (grad_cam2.py:141) or the model's prediction")
            p.add_argument("--limit", type=int, default=None, help="stop after N rows of the split")
            p.add_argument("--method", type=str, default="gradcam",
                           choices=["gradcam", "gradcam++", "xgradcam", "eigencam", "ablationcam"],
                           help="attribution method (vqamed2019/grad_cam.py:30,65-72); other than gradcam, the index "
                                "gains a `method` column")
    args = p.parse_args(argv)
    if args.cache_tokens:
        if mode != "vqa":
            p.error(f"--cache_tokens is for vqa: caching visual tokens for {mode} is not built")
        if args.mixed_precision:
            p.error("--cache_tokens cannot be combined with --mixed_precision: cached visual tokens and the step from them are fp32")
        if args.group_by_image:
            p.error("--cache_tokens cannot be combined with --group_by_image: a cached step runs no backbone to share")
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            p.error("--cache_tokens runs in one process: a cache sharded over data-parallel ranks is not built")
        if args.data_dir and args.cache_images is not None:
            p.error("--cache_images sizes the synthetic train set: with --data_dir the cache holds the images of the tables")
        if args.cache_views is not None and args.cache_views < 1:
            p.error(f"--cache_views {args.cache_views} must be at least 1")
        if args.cache_images is not None and args.cache_images < 1:
            p.error(f"--cache_images {args.cache_images} must be at least 1")
    elif args.cache_views is not None or args.cache_images is not None:
        p.error(f"--{'cache_views' if args.cache_views is not None else 'cache_images'} is read with --cache_tokens only")
    if mode == "gradcam" and args.group_by_image:
        p.error("--group_by_image is for vqa and eval: attribution over grouped batches is not built")
    if args.mixed_precision and args.overlap_adam:
        p.error("--overlap_adam cannot be combined with --mixed_precision: the whole gradient must be checked for "
                "inf / nan before the first parameter update")
    if args.watch in ("gradients", "all") and args.overlap_adam:
        p.error(f"--watch {args.watch} cannot be combined with --overlap_adam: gradient ranges are consumed and zeroed "
                "during backward, before the whole gradient can be looked at")
    if args.watch_freq < 1:
        p.error(f"--watch_freq {args.watch_freq} must be at least 1")
    try:
        check_optimizer_args(args)
    except ValueError as ex:
        p.error(str(ex))
    if getattr(args, "smoothing", None) is not None and not 0.0 <= args.smoothing <= 1.0:
        p.error(f"--smoothing {args.smoothing} is outside [0, 1]")
    if mode == "supcon":
        if args.supcon_mask != "none" and args.con_task == "simclr":
            p.error(f"--con_task simclr contradicts --supcon_mask {args.supcon_mask}: SimCLR has no positive mask")
        if args.supcon_mask != "none" and not args.data_dir:
            p.error(f"--supcon_mask {args.supcon_mask} needs --data_dir: synthetic batches have no captions to compare")
        if args.supcon_mask == "embeddings" and not args.caption_embeddings:
            p.error("--supcon_mask embeddings needs --caption_embeddings FILE (the precomputed sentence embeddings)")
        if args.supcon_mask != "embeddings" and args.caption_embeddings:
            p.error(f"--caption_embeddings is read by --supcon_mask embeddings only, not by --supcon_mask {args.supcon_mask}")
        tgiven = [o for o in ("teacher_weights", "teacher_vocab_file") if getattr(args, o)]
        if args.supcon_mask == "cosine" and len(tgiven) != 2:
            # (worded as argparse words a refused value: without the teacher's files `cosine` is not a choice)
            p.error("argument --supcon_mask: invalid choice: 'cosine' needs --teacher_weights FILE and --teacher_vocab_file FILE "
                    "(the BERT teacher and its WordPiece)")
        if args.supcon_mask == "bert_score" and len(tgiven) != 2:
            p.error("argument --supcon_mask: invalid choice: 'bert_score' needs --teacher_weights FILE and --teacher_vocab_file "
                    "FILE (the BERT teacher whose hidden layer is scored, and its WordPiece)")
        if args.supcon_mask not in ("cosine", "bert_score") and tgiven:
            p.error(f"--{tgiven[0]} is read by --supcon_mask bert_score and --supcon_mask cosine only, not by --supcon_mask "
                    f"{args.supcon_mask}")
        if args.bert_score == "bert":
            p.error("--bert_score bert is roberta-large with a baseline file (BERTScorer(lang='en', rescale_with_baseline=True)): "
                    "neither its byte-level BPE nor the baseline file is built here; use --bert_score scibert with a local "
                    "BERT checkpoint")
        bgiven = [o for o in ("bert_score_layer", "bert_score_baseline") if getattr(args, o) is not None]
        if args.supcon_mask != "bert_score" and bgiven:
            p.error(f"--{bgiven[0]} is read by --supcon_mask bert_score only, not by --supcon_mask {args.supcon_mask}")
        if args.supcon_mask == "bert_score":
            args.bert_score_layer = 8 if args.bert_score_layer is None else args.bert_score_layer
            args.bert_score_baseline = 0.0 if args.bert_score_baseline is None else args.bert_score_baseline
            if args.bert_score_layer < 1:
                p.error(f"--bert_score_layer {args.bert_score_layer} must be at least 1 (hidden_states[0] is the embeddings)")
            if not args.bert_score_baseline < 1.0:
                p.error(f"--bert_score_baseline {args.bert_score_baseline} must be below 1 (F is divided by 1 - B)")
    if mode in ("distill", "supcon") and args.max_token_length < 2:
        p.error(f"--max_token_length {args.max_token_length} has no room for [CLS] and [SEP]")
    if mode == "distill":
        given = [o for o in ("teacher_states", "val_teacher_states") if getattr(args, o)]
        tgiven = [o for o in ("teacher_weights", "teacher_vocab_file") if getattr(args, o)]
        if tgiven and given:
            p.error(f"--{tgiven[0]} (the teacher run on the GPU) and --{given[0]} (its precomputed states) exclude each other")
        if tgiven and not args.data_dir:
            p.error(f"--{tgiven[0]} is read with --data_dir only (synthetic batches: --teacher_layers N runs a random teacher)")
        if tgiven and len(tgiven) != 2:
            p.error("distill with the teacher on the GPU needs both --teacher_weights FILE and --teacher_vocab_file FILE")
        if args.teacher_layers and args.data_dir:
            p.error("--teacher_layers is for synthetic batches: with --data_dir the teacher comes from --teacher_weights")
        if args.teacher_layers < 0 or (args.teacher_layers and args.hidden_size % 64):
            p.error("--teacher_layers needs N >= 1 and a --hidden_size that is a multiple of 64")
        if args.data_dir and not tgiven and len(given) != 2:
            p.error("distill with --data_dir needs --teacher_states FILE and --val_teacher_states FILE (the teacher's "
                    "precomputed states of both splits)")
        if not args.data_dir and given:
            p.error(f"--{given[0]} is read with --data_dir only: synthetic batches bring their own teacher table")
    return mode, args


def main(argv=None):
    mode, args = parse_args(argv)
    if args.mixed_precision and mode == "supcon":
        print("--mixed_precision: the SupCon loop runs in fp32, as the reference's (supcon_utils.py:263-323 has no autocast)")
    out = {"mlm": run_mlm, "supcon": run_supcon, "distill": run_distill, "vqa": run_vqa, "eval": run_eval, "gradcam": run_gradcam}[mode](args)
    if dist.is_initialized():
        dist.destroy_process_group()
    return out


if __name__ == "__main__":
    main()
