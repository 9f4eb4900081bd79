"""Losses of the MMBERT training loops as autograd Functions over the HIP kernels.

  mlm_loss      -- pretrain/roco_utils.py:235-236 (log_softmax + NLLLoss over ALL positions) and
                   :257-265 (argmax accuracy over target > 0), one fused pass over the logits
  asl_loss      -- models/asl_singlelabel.py:23-53
  soft_ce_loss  -- soft-target cross entropy, forward and gradient in one launch: hard target, LabelSmoothing
                   (vqamed2019/utils.py:178-200), LabelSmoothByCategory (vqamed2019/utils.py:1234-1300)
  CategorySmoothing, LabelSmoothing -- the two --smoothing criteria of vqamed2019/train.py:164-174 over it
  supcon_loss   -- models/SupConLoss/loss.py:21-98: features only (SimCLR), or with labels / a positive mask
  jaccard_mask  -- models/SupConLoss/supcon_utils.py:110-138 from word-id sets resident on the device
  embedding_mask -- models/SupConLoss/supcon_utils.py:140-168 from precomputed sentence embeddings resident on the device
  split_feat    -- models/SupConLoss/supcon_utils.py:259-261
  distill_loss  -- pretrain/roco_utils.py:230-238 (nn.MSELoss against the teacher's states) with the target gathered from
                   a table resident on the device, forward and gradient in one launch
"""
from __future__ import annotations

import torch

from . import _lib as L


def _padded(x2d):
    """[rows, V] view whose row stride is a multiple of 4 and base 16-byte aligned (copy if not)"""
    rows, V = x2d.shape
    if x2d.stride(1) == 1 and x2d.stride(0) % 4 == 0 and x2d.stride(0) >= V and x2d.data_ptr() % 16 == 0:
        return x2d, x2d.stride(0)
    ld = (V + 3) & ~3
    buf = torch.zeros(rows, ld, dtype=torch.float32, device=x2d.device)
    buf[:, :V] = x2d
    return buf[:, :V], ld


class _MLMLoss(torch.autograd.Function):
    """forward: one pass over the logits (row log-sum-exp, NLL, first-index argmax); backward: one streaming
    pass writing (softmax - onehot) * upstream / rows.  The upstream gradient is read on the device by the kernel:
    nothing is synchronised with the host between forward and backward."""

    @staticmethod
    def forward(ctx, logits, target):
        if not logits.is_cuda:
            raise L.MMVQAError("mlm_loss: GPU tensors only (no CPU fallback)")
        V = logits.shape[-1]
        x, ld = _padded(logits.reshape(-1, V))
        rows = x.shape[0]
        tgt = target.reshape(-1).contiguous().long()
        row_loss = torch.empty(rows, dtype=torch.float32, device=x.device)
        row_lse = torch.empty(rows, dtype=torch.float32, device=x.device)
        pred = torch.empty(rows, dtype=torch.int64, device=x.device)
        out3 = torch.empty(3, dtype=torch.float32, device=x.device)
        L.check(L.lib().mmvqa_mlm_loss(L.stream_ptr(), L.ptr(x), ld, L.ptr(tgt), L.ptr(row_loss), L.ptr(row_lse),
                                       L.ptr(pred), None, 0, None, 1.0, rows, V, L.ptr(out3)))
        ctx.save_for_backward(x, tgt, row_lse)
        ctx.ld, ctx.shape = ld, logits.shape
        ctx.mark_non_differentiable(pred, out3)
        return out3[0].clone(), pred.view(target.shape), out3

    @staticmethod
    def backward(ctx, gloss, _gp, _go):
        x, tgt, row_lse = ctx.saved_tensors
        rows, V = x.shape
        dld = (V + 3) & ~3
        dl = torch.empty(rows, dld, dtype=torch.float32, device=x.device)
        g = gloss.reshape(1).float().contiguous()
        L.check(L.lib().mmvqa_mlm_grad(L.stream_ptr(), L.ptr(x), ctx.ld, L.ptr(tgt), L.ptr(row_lse), L.ptr(dl), dld,
                                       L.ptr(g), 1.0 / rows, rows, V))
        return dl[:, :V].view(ctx.shape), None


def mlm_loss(logits, target):
    """returns (loss, pred[B,T] (argmax at every position), stats[3] = {loss, n_masked, n_correct})"""
    return _MLMLoss.apply(logits, target)


class _ASLLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, gamma_pos, gamma_neg, eps):
        if not logits.is_cuda:
            raise L.MMVQAError("asl_loss: GPU tensors only (no CPU fallback)")
        x, ld = _padded(logits)
        rows, Cc = x.shape
        tgt = target.contiguous().long()
        row_loss = torch.empty(rows, dtype=torch.float32, device=x.device)
        dl = torch.zeros(rows, (Cc + 3) & ~3, dtype=torch.float32, device=x.device)
        L.check(L.lib().mmvqa_asl_loss(L.stream_ptr(), L.ptr(x), ld, L.ptr(tgt), L.ptr(row_loss), L.ptr(dl),
                                       dl.stride(0), rows, Cc, gamma_pos, gamma_neg, eps, 1.0 / rows))
        ctx.save_for_backward(dl)
        ctx.C = Cc
        return row_loss.mean()

    @staticmethod
    def backward(ctx, gloss):
        (dl,) = ctx.saved_tensors
        return (dl * gloss)[:, :ctx.C], None, None, None, None


def asl_loss(logits, target, gamma_pos=0.0, gamma_neg=4.0, eps=0.1):
    return _ASLLoss.apply(logits, target, gamma_pos, gamma_neg, eps)


def _soft_ce(x, ld, tgt, mode, smoothing, table, category, want_grad):
    """one mmvqa_soft_ce_loss call over the [rows, C] view x -> (loss (0-dim), row_loss [rows], dlogits [rows, ld'] or
    None); dlogits already carries the 1 / rows of the mean"""
    rows, Cc = x.shape
    row_loss = torch.empty(rows, dtype=torch.float32, device=x.device)
    loss = torch.empty((), dtype=torch.float32, device=x.device)
    dl = torch.empty(rows, (Cc + 3) & ~3, dtype=torch.float32, device=x.device) if want_grad else None
    n_cat, tld = (table.shape[0], table.stride(0)) if table is not None else (0, 0)
    L.check(L.lib().mmvqa_soft_ce_loss(L.stream_ptr(), L.ptr(x), ld, L.ptr(tgt), L.ptr(category), L.ptr(table), tld, n_cat,
                                       mode, float(smoothing), L.ptr(row_loss), L.ptr(loss), L.ptr(dl),
                                       dl.stride(0) if want_grad else 0, rows, Cc, 1.0 / rows))
    return loss, row_loss, dl


class _SoftCE(torch.autograd.Function):
    """forward: one launch writes the row losses AND dlogits (saved), a one-workgroup launch the mean; backward
    multiplies the saved dlogits by the upstream gradient, as _ASLLoss does.  want_grad is decided by the caller
    (soft_ce_loss): grad mode is always off inside forward and needs_input_grad does not see torch.no_grad.  Without
    it dlogits is neither allocated, written nor saved."""

    @staticmethod
    def forward(ctx, logits, target, mode, smoothing, table, category, want_grad):
        x, ld = _padded(logits)
        tgt = target.reshape(-1).contiguous().long()
        loss, _row_loss, dl = _soft_ce(x, ld, tgt, mode, smoothing, table, category, want_grad)
        if dl is not None:
            ctx.save_for_backward(dl)
        ctx.C = x.shape[1]
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dl,) = ctx.saved_tensors
        return (dl * gloss)[:, :ctx.C], None, None, None, None, None, None


def soft_ce_loss(logits, target, mode=L.SOFT_CE_HARD, smoothing=0.0, table=None, category=None):
    """Mean soft-target cross entropy of logits [rows, C] (fp32, on the GPU) against target [rows]:
      mode SOFT_CE_HARD (0)      nn.CrossEntropyLoss; `smoothing` is not read
      mode SOFT_CE_UNIFORM (1)   LabelSmoothing (vqamed2019/utils.py:178-200): soft = smoothing / C + (1 - smoothing) onehot
      mode SOFT_CE_CATEGORY (2)  LabelSmoothByCategory's training branch (utils.py:1247-1260): soft = table[category],
                                 then soft[target] = 1 - smoothing (overwritten, not added); `table` [n_cat, C] fp32 on the
                                 device (unit column stride; CategorySmoothing builds it), `category` [rows] integer ids
    A target outside [0, C) or a category outside [0, n_cat) makes the loss NaN (and that row's gradient); nothing is
    read outside the table.  Runs on the current stream, nothing is synchronised; the loss is bit-equal from run to run.
    Every tensor must already be on the logits' device: nothing is moved (a hidden host-to-device copy would stall the
    step).  Under torch.no_grad(), or for logits that need no gradient, dlogits is not computed."""
    if not logits.is_cuda:
        raise L.MMVQAError("soft_ce_loss: GPU tensors only (no CPU fallback)")
    if target.device != logits.device or (mode == L.SOFT_CE_CATEGORY and category is not None and category.device != logits.device):
        raise L.MMVQAError("soft_ce_loss: target and category must be on the logits' device (GPU tensors only; nothing is moved)")
    if logits.dim() != 2 or logits.dtype != torch.float32:
        raise ValueError(f"soft_ce_loss: logits must be fp32 [rows, C], got {logits.dtype} {list(logits.shape)}")
    if target.numel() != logits.shape[0]:
        raise ValueError(f"soft_ce_loss: {target.numel()} targets for {logits.shape[0]} rows")
    if mode == L.SOFT_CE_CATEGORY:
        if table is None or category is None:
            raise ValueError("soft_ce_loss: the category mode needs `table` and `category`")
        if (table.device != logits.device or table.dtype != torch.float32 or table.dim() != 2 or table.stride(1) != 1
                or table.shape[1] != logits.shape[1]):
            raise ValueError("soft_ce_loss: `table` must be fp32 [n_cat, C] on the logits' device with unit column stride")
        if category.numel() != logits.shape[0]:
            raise ValueError(f"soft_ce_loss: {category.numel()} category ids for {logits.shape[0]} rows")
        category = category.reshape(-1).long().contiguous()
    else:
        table = category = None
    want_grad = torch.is_grad_enabled() and logits.requires_grad
    return _SoftCE.apply(logits, target, int(mode), float(smoothing), table, category, want_grad)


class _Distill(torch.autograd.Function):
    """forward: one launch writes the rows' squared distances AND dh = (h - target) * 2 / (B T H) (saved), a
    one-workgroup launch the mean; backward multiplies the saved dh by the upstream gradient, as _SoftCE does.
    want_grad is decided by the caller (distill_loss)."""

    @staticmethod
    def forward(ctx, h, teacher, start, count, first, want_grad):
        B, T, H = h.shape
        x, ld = _padded(h.reshape(B * T, H))
        row_sq = torch.empty(B * T, dtype=torch.float32, device=x.device)
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        dh = torch.empty(B * T, (H + 3) & ~3, dtype=torch.float32, device=x.device) if want_grad else None
        L.check(L.lib().mmvqa_distill_mse(L.stream_ptr(), L.ptr(x), ld, L.ptr(teacher), int(teacher.dtype == torch.float16),
                                          teacher.shape[0], L.ptr(start), L.ptr(count), first, B, T, H, L.ptr(row_sq),
                                          L.ptr(loss), L.ptr(dh), dh.stride(0) if want_grad else 0,
                                          2.0 / (float(B) * T * H)))
        if dh is not None:
            ctx.save_for_backward(dh)
        ctx.shape = (B, T, H)
        return loss

    @staticmethod
    def backward(ctx, gloss):
        (dh,) = ctx.saved_tensors
        B, T, H = ctx.shape
        return (dh * gloss)[:, :H].reshape(B, T, H), None, None, None, None, None


def distill_loss(h, teacher, start, count, num_vis=5):
    """nn.MSELoss()(h, target) of the distillation task (pretrain/roco_train.py:94-95, roco_utils.py:230-238) for the
    headless model's output h [B, T, hidden] (fp32, on the GPU), the target being encode_text's distillation layout
    (roco_utils.py:162-199) gathered on the fly and never stored: rows num_vis + 2 .. num_vis + 2 + n_b - 1 of sample b
    are teacher[start[b] .. start[b] + n_b - 1] with n_b = min(count[b], T - num_vis - 3), every other row is zero, and
    the mean runs over all B T hidden elements.  teacher: the per-token states of every caption, [rows, hidden] fp32 or
    fp16 on h's device (a data.TeacherStates moved with .to(device), or its .states); start int64 [B] (first row of each
    sample's caption), count int32 [B] (its token count), both on the device.  A sample whose rows leave the table makes
    the loss (and that sample's gradient) NaN; nothing is read outside the table.  Runs on the current stream, nothing is
    synchronised; the loss is bit-equal from run to run.  Under torch.no_grad(), or for an h that needs no gradient, the
    gradient is not computed."""
    teacher = getattr(teacher, "states", teacher)
    if not h.is_cuda:
        raise L.MMVQAError("distill_loss: GPU tensors only (no CPU fallback)")
    if h.dim() != 3 or h.dtype != torch.float32:
        raise ValueError(f"distill_loss: h must be fp32 [B, T, hidden], got {h.dtype} {list(h.shape)}")
    B, T, H = h.shape
    if (teacher.dim() != 2 or teacher.dtype not in (torch.float32, torch.float16) or teacher.device != h.device
            or not teacher.is_contiguous() or teacher.shape[0] < 1):
        raise ValueError("distill_loss: `teacher` must be a contiguous fp32 / fp16 table [rows, hidden] on h's device")
    if teacher.shape[1] != H:
        raise ValueError(f"distill_loss: the teacher's states are {teacher.shape[1]} wide, h is {H} wide")
    if start.dtype != torch.int64 or tuple(start.shape) != (B,) or start.device != h.device:
        raise ValueError(f"distill_loss: `start` must be int64 [{B}] on h's device")
    if count.dtype != torch.int32 or tuple(count.shape) != (B,) or count.device != h.device:
        raise ValueError(f"distill_loss: `count` must be int32 [{B}] on h's device")
    first = int(num_vis) + 2
    if not 0 <= first < T:
        raise ValueError(f"distill_loss: num_vis + 2 = {first} does not fit T = {T}")
    want_grad = torch.is_grad_enabled() and h.requires_grad
    return _Distill.apply(h, teacher, start.contiguous(), count.contiguous(), first, want_grad)


class _Criterion:
    """what the loops ask of a criterion object: .to(device), .train() / .eval() (nn.Module's protocol: a fresh object
    is in training mode) and __call__(logits, target, category=None).  In eval mode both criteria are the plain cross
    entropy of the CE path (mlm_loss), as the reference's else branches are."""

    training = True

    def train(self, mode=True):
        self.training = bool(mode)
        return self

    def eval(self):
        return self.train(False)

    def to(self, device):
        return self


class LabelSmoothing(_Criterion):
    """vqamed2019/utils.py:178-200: training, mean_rows(sum_j -(smoothing / C + (1 - smoothing) [j == t]) log_softmax(x)_j);
    eval, cross entropy.  `category` is accepted and ignored, so the loops call both criteria the same way."""

    def __init__(self, smoothing=0.1):
        self.smoothing, self.confidence = float(smoothing), 1.0 - float(smoothing)

    def __call__(self, logits, target, category=None):
        if not self.training:
            return mlm_loss(logits, target)[0]
        return soft_ce_loss(logits, target, L.SOFT_CE_UNIFORM, self.smoothing)


class CategorySmoothing(_Criterion):
    """LabelSmoothByCategory (vqamed2019/utils.py:1234-1300).  train_rows: the WHOLE train table as data.vqa_tables
    gives it (row[2] = answer index, row[3] = category name).  categories: the distinct category names in row order --
    category id i is categories[i], the numbering VqaDataset(categories=...) hands out (the dataset's own numbering,
    utils.py:228-229; on VQA-Med 2019's table it is the order the reference hard-codes at :1292-1293).  table
    [n_cat, num_classes] fp32 on the host: row i is smoothing / len(idx) at idx = the distinct answers of category i's
    train rows (the double quotient rounded to fp32, as torch's indexed assignment stores it, :1266-1293), 0 elsewhere;
    a category without rows keeps a zero row.  .to(device) puts a copy with 16-byte-aligned rows on the GPU.
    Training mode: soft = table[category] with soft[target] = 1 - smoothing; eval mode: cross entropy, category ignored."""

    def __init__(self, train_rows, num_classes, smoothing=0.1, categories=None):
        self.smoothing, self.confidence, self.num_classes = float(smoothing), 1.0 - float(smoothing), int(num_classes)
        answers = {c: [] for c in (categories or ())}
        for r in train_rows:
            answers.setdefault(r[3], []).append(int(r[2]))
        self.categories = list(answers)
        self.cat2idx = {c: i for i, c in enumerate(self.categories)}
        self.table = torch.zeros(max(len(self.categories), 1), self.num_classes, dtype=torch.float32)
        for i, c in enumerate(self.categories):
            idx = sorted(set(answers[c]))
            if idx:
                self.table[i, torch.tensor(idx, dtype=torch.long)] = self.smoothing / len(idx)
        self._dev = None

    def to(self, device):
        ld = (self.num_classes + 3) & ~3
        buf = torch.zeros(self.table.shape[0], ld, dtype=torch.float32, device=device)
        buf[:, :self.num_classes] = self.table
        self._dev = buf[:, :self.num_classes]
        return self

    def __call__(self, logits, target, category=None):
        if not self.training:
            return mlm_loss(logits, target)[0]
        if category is None:
            raise ValueError("CategorySmoothing: the training branch needs the category ids of the batch")
        if self._dev is None or self._dev.device != logits.device:
            raise L.MMVQAError("CategorySmoothing: move the criterion to the logits' device first (.to(device)); "
                               "GPU tensors only (no CPU fallback)")
        return soft_ce_loss(logits, target, L.SOFT_CE_CATEGORY, self.smoothing, self._dev, category)


class _SupCon(torch.autograd.Function):
    """SupConLoss.forward(features) or (features, mask=mask): mmvqa_supcon_loss / mmvqa_supcon_loss_masked; no gradient
    for the mask"""

    @staticmethod
    def forward(ctx, features, mask, temperature, base_temperature):
        if not features.is_cuda:
            raise L.MMVQAError("supcon_loss: GPU tensors only (no CPU fallback)")
        N, nv, D = features.shape
        if nv != 2:
            raise NotImplementedError("two views (supcon_utils.py:259-261)")
        f = torch.cat(torch.unbind(features, dim=1), dim=0).contiguous().float()
        loss = torch.empty(1, dtype=torch.float32, device=f.device)
        df = torch.empty_like(f)
        if mask is None:
            ws = torch.empty(4 * N, dtype=torch.float32, device=f.device)
            L.check(L.lib().mmvqa_supcon_loss(L.stream_ptr(), L.ptr(f), L.ptr(loss), L.ptr(df), L.ptr(ws), N, D,
                                              temperature, base_temperature, 1.0))
        else:
            m = mask.detach().to(device=f.device, dtype=torch.float32).contiguous()      # loss.py:55
            ws = torch.empty(6 * N, dtype=torch.float32, device=f.device)
            L.check(L.lib().mmvqa_supcon_loss_masked(L.stream_ptr(), L.ptr(f), L.ptr(m), L.ptr(loss), L.ptr(df),
                                                     L.ptr(ws), N, D, temperature, base_temperature, 1.0))
        ctx.save_for_backward(df)
        ctx.N = N
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gloss):
        (df,) = ctx.saved_tensors
        N = ctx.N
        g = df * gloss
        return torch.stack([g[:N], g[N:]], dim=1), None, None, None


def supcon_loss(features, temperature=0.07, base_temperature=0.07, labels=None, mask=None):
    """SupConLoss.forward (models/SupConLoss/loss.py:21-98, contrast_mode 'all') over features [N, 2, D].
    Neither `labels` nor `mask`: SimCLR, the other view is the only positive (the unmasked kernels).
    labels [N]: samples of equal label are positives, mask = (labels[:, None] == labels[None, :]).
    mask [N, N]: mask[i][j] weights sample j as a positive of sample i; any real weights, may be asymmetric (the
    Jaccard mask is `jaccard_mask`; similarities computed elsewhere are passed the same way).  The mask gets no gradient.
    A row whose weights, the self-pair excluded, sum to zero makes the loss NaN: the reference divides by that sum and
    so does the kernel -- nothing is guarded.  A mask with a unit diagonal (Jaccard, labels) cannot produce it."""
    if labels is not None and mask is not None:
        raise ValueError("Cannot define both `labels` and `mask`")
    if labels is None and mask is None:
        return _SupCon.apply(features, None, temperature, base_temperature)
    N = features.shape[0]
    if labels is not None:
        labels = labels.contiguous().view(-1, 1)
        if labels.shape[0] != N:
            raise ValueError("Num of labels does not match num of features")
        mask = torch.eq(labels, labels.T).float().to(features.device)
    elif tuple(mask.shape) != (N, N):
        raise ValueError(f"`mask` must be [{N}, {N}] (one row and one column per sample), got {list(mask.shape)}")
    return _SupCon.apply(features, mask, temperature, base_temperature)


def jaccard_mask(words, rows_a, cols_a, rows_b=None, cols_b=None):
    """SimilarityCalculator.jaccard (supcon_utils.py:110-138) on the device -> [n, n] fp32:
    mask[i][j] = 1 for i == j, else |A_i & B_j| / |A_i | B_j| (0 when both sets are empty), A_i = the word set of text
    (rows_a[i], cols_a[i]) and B_j of (rows_b[j], cols_b[j]) in `words`, a data.WordSets moved to the device
    (column 0 = caption, 1..3 = translations).  rows_* / cols_* are int32 device tensors [n]; rows_b defaults to
    rows_a.  Bit-equal to the reference's Python loop.  Runs on the current stream; nothing is synchronised."""
    rows_b = rows_a if rows_b is None else rows_b
    if cols_b is None:
        raise ValueError("jaccard_mask: cols_b (the translation column each sample drew) is required")
    if not words.offsets.is_cuda:
        raise L.MMVQAError("jaccard_mask: GPU tensors only (no CPU fallback); move the WordSets with .to(device)")
    n = rows_a.shape[0]
    args = []
    for t in (rows_a, cols_a, rows_b, cols_b):
        if t.dtype != torch.int32 or t.device != words.offsets.device or t.shape != (n,):
            raise ValueError("jaccard_mask: rows / cols must be int32 tensors [n] on the device of the word sets")
        args.append(t.contiguous())
    mask = torch.empty(n, n, dtype=torch.float32, device=words.offsets.device)
    L.check(L.lib().mmvqa_jaccard_mask(L.stream_ptr(), L.ptr(words.offsets), L.ptr(words.ids), *(L.ptr(t) for t in args),
                                       L.ptr(mask), n, words.rows))
    return mask


def embedding_mask(emb, rows_a, cols_a, rows_b=None, cols_b=None):
    """SimilarityCalculator.sentence_trans / bert_embedd (supcon_utils.py:140-168) on the device -> [n, n] fp32:
    mask[i][j] = 1 for i == j, else the cosine of the embeddings of text (rows_a[i], cols_a[i]) and text
    (rows_b[j], cols_b[j]) in `emb`, a data.CaptionEmbeddings moved to the device with .to(device), which normalised it
    (column 0 = caption, 1..3 = translations).  rows_* / cols_* are int32 device tensors [n]; rows_b defaults to rows_a.
    Cosines may be negative and are used as they are, as in the reference.  Within (2 D + 8) 2^-24 of the exact cosine;
    the same inputs give the same bits on every launch.  Runs on the current stream; nothing is synchronised."""
    rows_b = rows_a if rows_b is None else rows_b
    if cols_b is None:
        raise ValueError("embedding_mask: cols_b (the translation column each sample drew) is required")
    if not emb.table.is_cuda or not emb.normalised:
        raise L.MMVQAError("embedding_mask: GPU tensors only (no CPU fallback); move the CaptionEmbeddings with "
                           ".to(device), which also normalises them")
    n = rows_a.shape[0]
    args = []
    for t in (rows_a, cols_a, rows_b, cols_b):
        if t.dtype != torch.int32 or t.device != emb.table.device or t.shape != (n,):
            raise ValueError("embedding_mask: rows / cols must be int32 tensors [n] on the device of the embeddings")
        args.append(t.contiguous())
    mask = torch.empty(n, n, dtype=torch.float32, device=emb.table.device)
    L.check(L.lib().mmvqa_cosine_mask(L.stream_ptr(), L.ptr(emb.table), *(L.ptr(t) for t in args), L.ptr(mask), n,
                                      emb.dim, emb.rows))
    return mask


def split_feat(feat, bsz):
    f1, f2 = torch.split(feat, [bsz, bsz], dim=0)
    return torch.cat([f1.unsqueeze(1), f2.unsqueeze(1)], dim=1)
