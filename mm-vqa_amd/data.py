"""Data layer: ROCO / VQA-Med 2019 files on disk -> device batches the hot path consumes.

Tables follow the reference's on-disk layouts:
  ROCO      pretrain/roco_utils.py:71-97, 567-587    <root>/<split>/radiology/<split>data.csv, images/<name>;
                                                     rows whose image is missing are dropped; name = column 1,
                                                     caption = column 2, stripped
  VQA-Med   vqamed2019/utils.py:51-79, train.py:100-105, utils.py:234-257
                                                     traindf / valdf / testdf.csv, {Train,Val,Test}/images/<img_id>.jpg;
                                                     category and answer lower-cased; ans2idx over
                                                     concat(train, val, test) in first-seen order
  ROCO SupCon pretrain/roco_supcon_train.py:83-85, models/SupConLoss/supcon_utils.py:218-256
                                                     the ROCO train table with back-translations in columns 3-5
                                                     (fr / de / es); three named rows removed; an item is both views'
                                                     image, the caption and one translation, each MLM-masked
(The reference also shuffles each table with DataFrame.sample(frac=pct); here the file order is kept and the epoch
order is a seeded permutation, so ans2idx is the first-seen order of the files.)

Two stages:
  host    HostLoader: a torch DataLoader whose worker processes decode (Image.open(p).convert("RGB")) and tokenise;
          collate packs a batch's images into one contiguous uint8 tensor + a [B, 2] shape table, pinned.  The
          train-time augment parameters are drawn in the main process, per batch, from a generator seeded with
          (seed, epoch, batch, rank), in torchvision's order (augment.sample_params).
  device  DeviceFeeder: copies each pinned batch to the GPU and runs DeviceAugment.run_packed on its own low-priority
          stream, `depth` batches ahead of the consumer; nothing on the host waits for the GPU.

Workers start through "forkserver": they are children of a fresh server process, never forks of this process,
which has the GPU open -- they inherit none of its GPU state and never touch the GPU themselves.

Determinism: a batch is a function of (seed, epoch, batch index, rank) only.  The epoch order is a seeded
permutation sharded across ranks like DistributedSampler (drop_last=False: the shard is padded from the head); the
MLM masking rng is seeded per sample; worker count and timing do not enter.

Grouped batches (VQA with --group_by_image): VqaGroupedDataset's item is an IMAGE with all of its
questions, GroupedBatchSampler packs images in the same seeded order until the next one's questions would pass
batch_size (which keeps counting questions), collate_grouped adds the host map `group`.  The augment parameters are drawn
per image, so every question of an image sees the same view in a step.
"""
from __future__ import annotations

import csv
import math
import os
import pickle
import random
from collections import deque

import numpy as np
import torch

from . import text
from .augment import DeviceAugment, sample_params

# torchvision settings of the two reference scripts (RandomResizedCrop scale / ratio, RandomRotation, ColorJitter)
ROCO_AUG = dict(scale=(0.95, 1.05), ratio=(0.95, 1.05), degrees=5.0, jitter=(0.05,) * 4)     # roco_train.py:98-108
VQA_AUG = dict(scale=(0.75, 1.25), ratio=(0.75, 1.25), degrees=10.0, jitter=(0.4,) * 4)      # vqamed2019/train.py:179-190


def usable_host_threads():
    """threads this process may really use: affinity mask capped by the cgroup CPU quota (os.cpu_count() reports the
    whole host)"""
    n = os.cpu_count() or 1
    try:
        n = len(os.sched_getaffinity(0))
    except Exception:
        pass
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()
        if q != "max":
            n = min(n, max(1, int(int(q) / int(per))))
    except Exception:
        pass
    return n


def default_workers():
    return min(4, usable_host_threads())


def mix_seed(*parts):
    """a 63-bit seed from a tuple of integers (independent of Python's hash randomisation)"""
    return int(np.random.SeedSequence([int(p) & 0xFFFFFFFF for p in parts]).generate_state(1, np.uint64)[0]) >> 1


def sample_rng(seed, epoch, index):
    """the MLM masking rng of one sample"""
    return random.Random(mix_seed(seed, epoch, index, 0x6D6C6D))


def batch_generator(seed, epoch, batch, rank):
    """the torch.Generator the augment parameters of one batch are drawn from"""
    return torch.Generator().manual_seed(mix_seed(seed, epoch, batch, rank, 0x617567))


# --------------------------------------------------------------------------- tables
def _read_csv(path):
    with open(path, newline="", encoding="utf-8") as f:
        rows = list(csv.reader(f))
    if not rows:
        raise ValueError(f"{path}: empty table")
    return rows[0], rows[1:]


def roco_table(root, split):
    """[(image path, caption)] of <root>/<split>/radiology/<split>data.csv, rows without an image dropped (in order)"""
    d = os.path.join(root, split, "radiology")
    names = set(os.listdir(os.path.join(d, "images")))
    fname = {"validation": "valdata.csv"}.get(split, split + "data.csv")
    _hdr, rows = _read_csv(os.path.join(d, fname))
    return [(os.path.join(d, "images", r[1]), r[2].strip()) for r in rows if len(r) > 2 and r[1] in names]


# rows roco_supcon_train.py:83-85 removes from the SupCon train table (two without an image, one without a caption)
SUPCON_DROPPED = ("PMC4345544_yjbm_88_1_93_g04.jpg", "PMC4240561_MA-68-291-g002.jpg", "PMC4093298_jadp-03-059-g02.jpg")


def roco_supcon_table(root):
    """[(image path, caption, (t3, t4, t5))] of <root>/train/radiology/traindata.csv for SupCon: rows without an image
    dropped (in order), then the three rows of SUPCON_DROPPED.  The translations are columns 3-5 by position, as
    supcon_utils.py:228-236 reads them.  A kept row with fewer than 6 fields or an empty translation raises
    ValueError naming the file and row (the reference would fail later, on the draw that picks the cell)."""
    d = os.path.join(root, "train", "radiology")
    names = set(os.listdir(os.path.join(d, "images")))
    path = os.path.join(d, "traindata.csv")
    _hdr, rows = _read_csv(path)
    out = []
    for k, r in enumerate(rows, start=1):
        if len(r) < 2 or r[1] not in names or r[1] in SUPCON_DROPPED:
            continue
        if len(r) < 6:
            raise ValueError(f"{path}: row {k} (after the header) has {len(r)} fields; SupCon needs 6 "
                             "(id, name, caption and three translations)")
        tr = tuple(c.strip() for c in r[3:6])
        for c, t in enumerate(tr, start=3):
            if not t:
                raise ValueError(f"{path}: row {k} (after the header) has an empty translation in column {c}")
        out.append((os.path.join(d, "images", r[1]), r[2].strip(), tr))
    return out


class WordSets:
    """Word sets of every text of a SupCon table as one CSR of integer ids, for the Jaccard mask
    (SimilarityCalculator.jaccard_similarity, supcon_utils.py:120-138).  Text t = row * 4 + column (0 = caption,
    1..3 = the translations of CSV columns 3..5) owns ids[offsets[t]:offsets[t + 1]]: the sorted, unique ids of
    set(text.lower().split()).  Words map to ids through one table-wide dictionary in first-seen order -- exact, no
    hashing, so two different words never share an id.  offsets [4 * rows + 1] and ids are int32 tensors; built once
    per dataset on the host, moved once with .to(device)."""

    TEXTS = 4

    def __init__(self, offsets, ids, rows, vocab=None):
        self.offsets, self.ids, self.rows, self.vocab = offsets, ids, int(rows), vocab

    @classmethod
    def from_texts(cls, texts):
        """texts: per row, (caption, t3, t4, t5)"""
        vocab, offs, chunks = {}, [0], []
        for row in texts:
            if len(row) != cls.TEXTS:
                raise ValueError(f"WordSets: a row holds {cls.TEXTS} texts (caption and three translations), got {len(row)}")
            for t in row:
                w = np.array(sorted({vocab.setdefault(x, len(vocab)) for x in t.lower().split()}), dtype=np.int64)
                chunks.append(w)
                offs.append(offs[-1] + len(w))
        if offs[-1] >= 2 ** 31 or len(vocab) >= 2 ** 31:
            raise ValueError(f"WordSets: {offs[-1]} ids / {len(vocab)} words do not fit int32 offsets")
        ids = np.concatenate(chunks) if chunks else np.zeros(0, dtype=np.int64)
        if ids.size == 0:
            ids = np.zeros(1, dtype=np.int64)       # never read (every set is empty); keeps the pointer non-null
        return cls(torch.from_numpy(np.asarray(offs, dtype=np.int32)), torch.from_numpy(ids.astype(np.int32)),
                   len(texts), vocab)

    @classmethod
    def from_table(cls, rows):
        """rows of roco_supcon_table: (image path, caption, (t3, t4, t5))"""
        return cls.from_texts([(r[1],) + tuple(r[2]) for r in rows])

    def to(self, device):
        return WordSets(self.offsets.to(device), self.ids.to(device), self.rows, self.vocab)

    def word_ids(self, row, col):
        """the id set of one text as a numpy array (host copy of the CSR only)"""
        t = int(row) * self.TEXTS + int(col)
        o = self.offsets.numpy()
        return self.ids.numpy()[o[t]:o[t + 1]]

    def jaccard_host(self, rows_a, cols_a, rows_b, cols_b):
        """the mask mmvqa_jaccard_mask computes, in numpy from the host CSR (tests, and the DDP rehearsal on CPU)"""
        n = len(rows_a)
        out = np.zeros((n, n), dtype=np.float32)
        for i in range(n):
            a = self.word_ids(rows_a[i], cols_a[i])
            for j in range(n):
                if i == j:
                    out[i, j] = 1.0
                    continue
                b = self.word_ids(rows_b[j], cols_b[j])
                inter = np.intersect1d(a, b, assume_unique=True).size
                uni = a.size + b.size - inter
                out[i, j] = np.float32(float(inter) / uni) if uni else 0.0
        return out


class CaptionEmbeddings:
    """Sentence embeddings of every text of a SupCon table, for the cosine mask (SimilarityCalculator.sentence_trans /
    bert_embedd, supcon_utils.py:140-168).  The encoder is not run here: the embeddings are computed once, offline, with
    any sentence encoder and read from a file.  table [rows, 4, D] fp32; text (row, column) as in WordSets (0 = caption,
    1..3 = the translations of CSV columns 3..5).  On the host the table holds the embeddings as given; .to(device)
    uploads it once and scales every text to unit length there (mmvqa_normalize_rows), which is the form
    mmvqa_cosine_mask reads.  Held whole on every rank: rows x 4 x D x 4 bytes."""

    TEXTS = 4
    MAX_DIM = 4096

    def __init__(self, table, normalised=False):
        self.table, self.normalised = table, bool(normalised)
        self.rows, self.dim = int(table.shape[0]), int(table.shape[2])

    @classmethod
    def from_array(cls, emb):
        """emb [rows, 4, D], float16 / float32 / float64 (numpy or torch), finite -> held as fp32 on the host"""
        emb = emb.detach().cpu().numpy() if isinstance(emb, torch.Tensor) else np.asarray(emb)
        if emb.ndim != 3 or emb.shape[1] != cls.TEXTS:
            raise ValueError(f"CaptionEmbeddings: embeddings must be [rows, {cls.TEXTS}, D] (caption and three "
                             f"translations per row), got {list(emb.shape)}")
        if emb.dtype not in (np.float16, np.float32, np.float64):
            raise ValueError(f"CaptionEmbeddings: embeddings must be float16, float32 or float64, got {emb.dtype}")
        if emb.shape[0] < 1 or not 1 <= emb.shape[2] <= cls.MAX_DIM:
            raise ValueError(f"CaptionEmbeddings: need at least one row and 1 <= D <= {cls.MAX_DIM}, got {list(emb.shape)}")
        emb = np.ascontiguousarray(emb, dtype=np.float32)
        if not np.isfinite(emb).all():
            raise ValueError("CaptionEmbeddings: the embeddings hold non-finite values")
        return cls(torch.from_numpy(emb))

    @classmethod
    def from_file(cls, path, table):
        """path: an .npz with `names` (image file names, a unicode array) and `emb` [len(names), 4, D]; table: rows of
        roco_supcon_table.  Row r of the result is the entry named like the base name of table[r]'s image, so the file
        may hold more rows than the table keeps, in any order."""
        with np.load(path, allow_pickle=False) as z:
            for key in ("names", "emb"):
                if key not in z.files:
                    raise ValueError(f"{path}: no array {key!r} (needs names [R] and emb [R, 4, D])")
            names, emb = z["names"], z["emb"]
        if names.ndim != 1 or names.dtype.kind != "U":
            raise ValueError(f"{path}: names must be a one-dimensional unicode array, got {names.dtype} {list(names.shape)}")
        if emb.ndim != 3 or emb.shape[1] != cls.TEXTS or emb.shape[0] != len(names):
            raise ValueError(f"{path}: emb must be [{len(names)}, {cls.TEXTS}, D] (one row per name), got {list(emb.shape)}")
        if emb.dtype.kind != "f":
            raise ValueError(f"{path}: emb must be float16, float32 or float64, got {emb.dtype}")
        where = {}
        for k, name in enumerate(names.tolist()):
            if where.setdefault(name, k) != k:
                raise ValueError(f"{path}: name {name!r} appears more than once (entries {where[name]} and {k})")
        want = [os.path.basename(str(r[0])) for r in table]
        missing = [w for w in want if w not in where]
        if missing:
            raise ValueError(f"{path}: no embeddings for {len(missing)} of the table's {len(want)} rows: "
                             + ", ".join(missing[:5]) + (" ..." if len(missing) > 5 else ""))
        try:
            return cls.from_array(emb[np.asarray([where[w] for w in want], dtype=np.int64)])
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None

    def to(self, device, eps=1e-8):
        """the table on `device`, every text scaled to x / max(|x|, eps) there (once; on the current stream)"""
        from . import _lib as L
        if self.normalised:
            return CaptionEmbeddings(self.table.to(device), True)
        t = self.table.to(device).contiguous()
        if not t.is_cuda:
            raise L.MMVQAError("CaptionEmbeddings.to: the table is normalised by a HIP kernel (no CPU fallback); "
                               "cosine_host gives the mask from the host copy")
        if t.data_ptr() == self.table.data_ptr():
            t = t.clone()
        with torch.cuda.device(t.device):
            L.check(L.lib().mmvqa_normalize_rows(L.stream_ptr(), L.ptr(t), self.rows * self.TEXTS, self.dim, float(eps)))
        return CaptionEmbeddings(t, True)

    def cosine_host(self, rows_a, cols_a, rows_b, cols_b, eps=1e-8):
        """the mask mmvqa_cosine_mask computes, in numpy float64 from the host copy (tests, and the DDP rehearsal on
        CPU): a / max(|a|, eps) . b / max(|b|, eps), diagonal 1 (supcon_utils.py:152-159)"""
        if self.normalised or self.table.is_cuda:
            raise ValueError("CaptionEmbeddings.cosine_host: needs the host copy of the embeddings as given")
        t = self.table.numpy()
        unit = lambda x: x / np.maximum(np.sqrt((x * x).sum(1, keepdims=True)), eps)   # noqa: E731
        a = unit(t[np.asarray(rows_a, dtype=np.int64), np.asarray(cols_a, dtype=np.int64)].astype(np.float64))
        b = unit(t[np.asarray(rows_b, dtype=np.int64), np.asarray(cols_b, dtype=np.int64)].astype(np.float64))
        out = np.einsum("ik,jk->ij", a, b)
        np.fill_diagonal(out, 1.0)
        return out


def distill_layout(piece_ids, T, num_vis, cls_id, sep_id):
    """the teacher's piece ids of one caption (without CLS / SEP) in encode_text's distillation layout
    (roco_utils.py:162-199) -> (ids, seg, mask) lists of T"""
    part2 = [int(i) for i in piece_ids[:max(T - (num_vis + 3), 0)]]                   # :174-175
    tokens = [cls_id] + [0] * num_vis + [sep_id] + part2 + [sep_id]                   # :178
    seg = [0] * (num_vis + 2) + [1] * (len(part2) + 1)                                # :181
    n_pad = T - len(tokens)
    if n_pad < 0:
        raise ValueError(f"TeacherStates: T={T} has no room for [CLS], {num_vis} visual tokens and two [SEP]")
    return tokens + [0] * n_pad, seg + [0] * n_pad, [1] * len(tokens) + [0] * n_pad


def teacher_row(tokenizer, text_, max_token_length):
    """what the teacher is fed for one text, as HF's tokenizer(text, truncation=True) with model_max_length =
    --max_token_length gives it: [CLS] + the first max_token_length - 2 pieces + [SEP] -> int64 [1 + max_token_length]:
    the length (CLS and SEP included), then the ids, zero-padded.  The shape is the same for every text."""
    L = int(max_token_length)
    if L < 2:
        raise ValueError(f"max_token_length = {L} has no room for [CLS] and [SEP]")
    pieces = tokenizer.convert_tokens_to_ids(tokenizer.tokenize(text_))[:L - 2]
    ids = [tokenizer.cls_token_id] + pieces + [tokenizer.sep_token_id]
    return torch.tensor([len(ids)] + ids + [0] * (L - len(ids)), dtype=torch.int64)


class TeacherStates:
    """The teacher's per-token states of every caption of a ROCO table, for the distillation task
    (pretrain/roco_utils.py:112-132: last_hidden_state[1:len-1] of the teacher on the caption, CLS and SEP dropped).
    The teacher and its tokenizer are not run here: the states are computed once, offline, and read from a file.
    Caption r owns ids[offsets[r]:offsets[r + 1]] (the teacher tokenizer's ids, without CLS / SEP -- the student is fed
    exactly the tokens the teacher saw, roco_utils.py:130) and the rows of `states` [total, D] of the same range.
    offsets / ids are int64 numpy arrays on the host; states is a torch tensor, float16 as given or fp32 (float32 and
    float64 input), uploaded once by .to(device) and held whole on every rank: total x D x 2 or 4 bytes."""

    def __init__(self, offsets, ids, states, cls_id=101, sep_id=102):
        self.offsets, self.ids, self.states = offsets, ids, states
        self.cls_id, self.sep_id = int(cls_id), int(sep_id)
        self.rows, self.dim = len(offsets) - 1, int(states.shape[1])

    @classmethod
    def from_arrays(cls, offsets, ids, states, cls_id=101, sep_id=102):
        """offsets [rows + 1] non-decreasing from 0, ids [total] integers, states [total, D] float16 / 32 / 64 (numpy or
        torch), finite"""
        as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)   # noqa: E731
        offsets, ids, states = as_np(offsets), as_np(ids), as_np(states)
        if offsets.ndim != 1 or ids.ndim != 1 or states.ndim != 2:
            raise ValueError(f"TeacherStates: offsets and ids must be one-dimensional and states [total, D], got "
                             f"{list(offsets.shape)}, {list(ids.shape)}, {list(states.shape)}")
        if offsets.dtype.kind not in "iu" or ids.dtype.kind not in "iu":
            raise ValueError(f"TeacherStates: offsets and ids must be integer arrays, got {offsets.dtype} and {ids.dtype}")
        if states.dtype not in (np.float16, np.float32, np.float64):
            raise ValueError(f"TeacherStates: states must be float16, float32 or float64, got {states.dtype}")
        offsets = offsets.astype(np.int64)
        if len(offsets) < 1 or offsets[0] != 0 or (np.diff(offsets) < 0).any():
            raise ValueError("TeacherStates: offsets must start at 0 and never decrease")
        if not offsets[-1] == len(ids) == states.shape[0]:
            raise ValueError(f"TeacherStates: offsets end at {int(offsets[-1])}, there are {len(ids)} ids and "
                             f"{states.shape[0]} states (all three must agree)")
        if states.shape[1] < 1:
            raise ValueError("TeacherStates: the states have no columns")
        if not np.isfinite(states).all():
            raise ValueError("TeacherStates: the states hold non-finite values")
        if states.dtype != np.float16:
            states = states.astype(np.float32)
        if states.shape[0] == 0:
            states = np.zeros((1, states.shape[1]), dtype=states.dtype)   # never read (every caption is empty); keeps the pointer non-null
        return cls(offsets, ids.astype(np.int64), torch.from_numpy(np.ascontiguousarray(states)), cls_id, sep_id)

    @classmethod
    def from_file(cls, path, table):
        """path: an .npz (no pickled objects) with names [R] (image file names, a unicode array), offsets [R + 1], ids
        [total], states [total, D] and optionally the scalars cls_id / sep_id (default 101 / 102); table: rows of
        roco_table.  Caption r of the result is the entry named like the base name of table[r]'s image, so the file may
        hold more entries than the table keeps, in any order."""
        with np.load(path, allow_pickle=False) as z:
            for key in ("names", "offsets", "ids", "states"):
                if key not in z.files:
                    raise ValueError(f"{path}: no array {key!r} (needs names [R], offsets [R + 1], ids [total] and "
                                     "states [total, D])")
            names, offs, ids, states = z["names"], z["offsets"], z["ids"], z["states"]
            cls_id = int(z["cls_id"]) if "cls_id" in z.files else 101
            sep_id = int(z["sep_id"]) if "sep_id" in z.files else 102
        if names.ndim != 1 or names.dtype.kind != "U":
            raise ValueError(f"{path}: names must be a one-dimensional unicode array, got {names.dtype} {list(names.shape)}")
        if offs.ndim != 1 or ids.ndim != 1 or states.ndim != 2:
            raise ValueError(f"{path}: offsets and ids must be one-dimensional and states [total, D], got "
                             f"{list(offs.shape)}, {list(ids.shape)}, {list(states.shape)}")
        if offs.dtype.kind not in "iu" or ids.dtype.kind not in "iu":
            raise ValueError(f"{path}: offsets and ids must be integer arrays, got {offs.dtype} and {ids.dtype}")
        if states.dtype.kind != "f":
            raise ValueError(f"{path}: states must be float16, float32 or float64, got {states.dtype}")
        if len(offs) != len(names) + 1:
            raise ValueError(f"{path}: {len(offs)} offsets for {len(names)} names (needs one more than names)")
        offs = offs.astype(np.int64)
        if offs[0] != 0 or (np.diff(offs) < 0).any():
            raise ValueError(f"{path}: offsets must start at 0 and never decrease")
        if not offs[-1] == len(ids) == states.shape[0]:
            raise ValueError(f"{path}: offsets end at {int(offs[-1])}, there are {len(ids)} ids and {states.shape[0]} "
                             "states (all three must agree)")
        where = {}
        for k, name in enumerate(names.tolist()):
            if where.setdefault(name, k) != k:
                raise ValueError(f"{path}: name {name!r} appears more than once (entries {where[name]} and {k})")
        want = [os.path.basename(str(r[0])) for r in table]
        missing = [w for w in want if w not in where]
        if missing:
            raise ValueError(f"{path}: no teacher states for {len(missing)} of the table's {len(want)} rows: "
                             + ", ".join(missing[:5]) + (" ..." if len(missing) > 5 else ""))
        pick = np.asarray([where[w] for w in want], dtype=np.int64)
        lens = offs[pick + 1] - offs[pick]
        new = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = (np.concatenate([np.arange(offs[k], offs[k + 1]) for k in pick]) if len(pick) else np.zeros(0)).astype(np.int64)
        try:
            return cls.from_arrays(new, ids[take], states[take], cls_id, sep_id)
        except ValueError as e:
            raise ValueError(f"{path}: {e}") from None

    def to(self, device):
        """the states on `device` (one upload); offsets and ids stay on the host, where batch() reads them"""
        return TeacherStates(self.offsets, self.ids, self.states.to(device), self.cls_id, self.sep_id)

    def check_vocab(self, emb_vocab):
        """every id the student will be fed must index its embedding table"""
        bad = [i for i in (self.cls_id, self.sep_id) if not 0 <= i < emb_vocab]
        if len(self.ids) and (self.ids.min() < 0 or self.ids.max() >= emb_vocab):
            bad.append(int(self.ids.max() if self.ids.max() >= emb_vocab else self.ids.min()))
        if bad:
            raise ValueError(f"TeacherStates: token id {bad[0]} is outside the embedding table [0, {emb_vocab}) "
                             "(--emb_vocab must be the teacher's vocabulary size)")

    def encode(self, row, T, num_vis=5):
        """one caption in encode_text's distillation layout (roco_utils.py:162-199) -> (ids, seg, mask) lists of T"""
        lo, hi = int(self.offsets[row]), int(self.offsets[row + 1])
        return distill_layout(self.ids[lo:hi], T, num_vis, self.cls_id, self.sep_id)

    def batch(self, rows, T, num_vis=5):
        """-> host (ids, seg, mask) int64 [B, T], start int64 [B] (first row of each caption in `states`) and count
        int32 [B] (its token count, not truncated: mmvqa_distill_mse clamps it to T - num_vis - 3)"""
        enc = [self.encode(int(r), T, num_vis) for r in rows]
        ids, seg, mask = (torch.tensor([e[k] for e in enc], dtype=torch.int64).reshape(len(enc), T) for k in range(3))
        rows = np.asarray(rows, dtype=np.int64)
        start = torch.from_numpy(self.offsets[rows].astype(np.int64))
        count = torch.from_numpy((self.offsets[rows + 1] - self.offsets[rows]).astype(np.int32))
        return ids, seg, mask, start, count

    def target_host(self, rows, T, num_vis=5):
        """the dense target of roco_utils.py:196-197 as float64 [B, T, D], from the host copy of the states (tests)"""
        st = self.states.cpu().double()
        out = torch.zeros(len(rows), T, self.dim, dtype=torch.float64)
        for b, r in enumerate(rows):
            lo = int(self.offsets[int(r)])
            n = min(int(self.offsets[int(r) + 1]) - lo, max(T - (num_vis + 3), 0))
            out[b, num_vis + 2:num_vis + 2 + n] = st[lo:lo + n]
        return out


def vqa_tables(root):
    """-> (columns, {"train", "val", "test": [row]}, idx2ans).  A row is (image path, question, answer index, category,
    mode) -- the fields evaluate.write_test_files writes."""
    splits = {}
    for key, fname, folder in (("train", "traindf.csv", "Train"), ("val", "valdf.csv", "Val"), ("test", "testdf.csv", "Test")):
        hdr, rows = _read_csv(os.path.join(root, fname))
        col = {c: i for i, c in enumerate(hdr)}
        for need in ("img_id", "question", "answer", "category"):
            if need not in col:
                raise ValueError(f"{fname}: no column {need!r}")
        splits[key] = [(os.path.join(root, folder, "images", r[col["img_id"]] + ".jpg"), r[col["question"]],
                        r[col["answer"]].lower(), r[col["category"]].lower(), r[col["mode"]] if "mode" in col else key)
                       for r in rows]
    ans2idx = {}
    for key in ("train", "val", "test"):
        for r in splits[key]:
            ans2idx.setdefault(r[2], len(ans2idx))
    out = {k: [(p, q, ans2idx[a], c, m) for (p, q, a, c, m) in v] for k, v in splits.items()}
    return ["img_id", "question", "answer", "category", "mode"], out, {i: a for a, i in ans2idx.items()}


def load_keywords(root):
    with open(os.path.join(root, "vocab", "med_vocab.pkl"), "rb") as f:
        return text.get_keywords(pickle.load(f))


# --------------------------------------------------------------------------- datasets (run in the worker processes)
def decode(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.asarray(im.convert("RGB"), dtype=np.uint8)


class RocoDataset(torch.utils.data.Dataset):
    """item (epoch, index) -> (uint8 [H, W, 3], ids, seg, mask, target) as roco_utils.py:573-587 returns it"""

    def __init__(self, rows, tokenizer, keywords, num_vis=5, max_position_embeddings=75, mlm_prob=0.15, seed=0):
        self.rows, self.tok, self.kw = list(rows), tokenizer, frozenset(keywords)
        self.num_vis, self.T, self.mlm_prob, self.seed = num_vis, max_position_embeddings, mlm_prob, seed

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, key):
        epoch, idx = key
        path, caption = self.rows[idx]
        ids, seg, mask, tgt = text.encode_text(caption, self.tok, self.kw, self.num_vis, self.T, self.mlm_prob,
                                               sample_rng(self.seed, epoch, idx))
        return decode(path), ids, seg, mask, tgt, idx


class DistillDataset(torch.utils.data.Dataset):
    """item (epoch, index) -> (uint8 [H, W, 3], ids, seg, mask, (start, count)) of the distillation task: the text is
    TeacherStates.encode of the row's caption, and in the target's place travel the two integers that name the caption's
    states in the resident table (int64 [2]; a batch's fifth tensor is int64 [B, 2]).  Only the teacher's offsets and
    ids are kept here (the worker processes get a copy of the dataset): the states stay with the caller."""

    def __init__(self, rows, teacher, num_vis=5, max_position_embeddings=75):
        if teacher.rows != len(rows):
            raise ValueError(f"DistillDataset: {len(rows)} table rows, teacher states of {teacher.rows} captions")
        self.rows, self.num_vis, self.T = list(rows), num_vis, max_position_embeddings
        self.text = TeacherStates(teacher.offsets, teacher.ids, torch.zeros(1, teacher.dim), teacher.cls_id, teacher.sep_id)

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, key):
        _epoch, idx = key
        ids, seg, mask, start, count = self.text.batch([idx], self.T, self.num_vis)
        return decode(self.rows[idx][0]), ids[0], seg[0], mask[0], torch.tensor([int(start[0]), int(count[0])]), idx


def collate_teacher(items):
    """collate for OnlineDistillDataset: the same dict plus teacher_T, the batch's longest teacher input (a host
    scalar: the step sizes the teacher's launches from it without reading the device)"""
    out = collate(items)
    out["teacher_T"] = out["target"][:, 0].max()
    return out


class OnlineDistillDataset(torch.utils.data.Dataset):
    """item (epoch, index) -> (uint8 [H, W, 3], ids, seg, mask, teacher row) of the distillation task with the teacher
    run on the device (teacher.BertTeacher): the caption is tokenised here, in the worker, with the TEACHER's WordPiece;
    the student's ids / seg / mask are encode_text's distillation layout of those same piece ids
    (roco_utils.py:174-186; the student is fed the tokens the teacher saw), and in the target's place travels
    teacher_row's int64 [1 + max_token_length]: length, then [CLS] pieces [SEP].  A batch's fifth tensor is int64
    [B, 1 + max_token_length] -- one shape for every batch -- and the host batch carries teacher_T, its longest length."""

    collate = staticmethod(collate_teacher)

    def __init__(self, rows, tokenizer, num_vis=5, max_position_embeddings=75, max_token_length=512):
        self.rows, self.tok = list(rows), tokenizer
        self.num_vis, self.T, self.L = num_vis, max_position_embeddings, int(max_token_length)
        if self.L < 2:
            raise ValueError(f"OnlineDistillDataset: max_token_length = {self.L} has no room for [CLS] and [SEP]")

    def __len__(self):
        return len(self.rows)

    def encode(self, idx):
        """(ids, seg, mask int64 [T], teacher row int64 [1 + L])"""
        row = teacher_row(self.tok, self.rows[idx][1], self.L)
        n = int(row[0])
        ids, seg, mask = distill_layout(row[2:n].tolist(), self.T, self.num_vis, self.tok.cls_token_id, self.tok.sep_token_id)
        return tuple(torch.tensor(v, dtype=torch.int64) for v in (ids, seg, mask)) + (row,)

    def __getitem__(self, key):
        _epoch, idx = key
        return (decode(self.rows[idx][0]),) + self.encode(idx) + (idx,)


def category_ids(rows):
    """{category name: id}: id i is the i-th distinct category of `rows` (data.vqa_tables rows, row[3]) in row order,
    the numbering of vqamed2019/utils.py:228-229 over the train table"""
    ids = {}
    for r in rows:
        ids.setdefault(r[3], len(ids))
    return ids


class VqaDataset(torch.utils.data.Dataset):
    """item (epoch, index) -> (uint8 [H, W, 3], ids, seg, mask, answer index) as vqamed2019/utils.py:234-257
    categories = {category name: id} (category_ids of the train table, or CategorySmoothing.cat2idx): the item gains a
    last element, the row's category id (utils.py:252, self.cats2ans[category]), and batches are packed by
    collate_category.  A row whose category the map lacks is refused when the dataset is built.  Default (None): the
    item and the batches are as before."""

    def __init__(self, rows, tokenizer, max_position_embeddings=28, categories=None):
        self.rows, self.tok, self.T = list(rows), tokenizer, max_position_embeddings
        self.categories = None if categories is None else dict(categories)
        if self.categories is not None:
            missing = sorted({r[3] for r in self.rows} - set(self.categories))
            if missing:
                raise ValueError(f"VqaDataset: categories {missing} of the rows are not in the category map")
            self.collate = collate_category

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, key):
        _epoch, idx = key
        path, question, ans = self.rows[idx][:3]
        ids, seg, mask = (torch.tensor(v, dtype=torch.long) for v in text.encode_text_vqa(question, self.tok, self.T))
        item = decode(path), ids, seg, mask, torch.tensor(ans, dtype=torch.long), idx
        return item if self.categories is None else item + (self.categories[self.rows[idx][3]],)


def collate(items):
    """-> dict: pixels (uint8, the images back to back), shapes [B, 2] (h, w), ids / seg / mask [B, T], target,
    index [B] (dataset rows)"""
    imgs = [it[0] for it in items]
    pixels = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs]))
    return dict(pixels=pixels, shapes=torch.tensor([a.shape[:2] for a in imgs], dtype=torch.int64),
                ids=torch.stack([it[1] for it in items]), seg=torch.stack([it[2] for it in items]),
                mask=torch.stack([it[3] for it in items]), target=torch.stack([it[4] for it in items]),
                index=torch.tensor([it[5] for it in items], dtype=torch.int64))


def collate_category(items):
    """collate for items that end with the category id (VqaDataset(categories=...)): the same dict plus category [B]
    int64 (like target)"""
    out = collate([it[:6] for it in items])
    out["category"] = torch.tensor([it[6] for it in items], dtype=torch.int64)
    return out


# --------------------------------------------------------------------------- grouped batches
def group_rows_by_image(rows):
    """VQA-Med asks several questions of one image (four per train / val image in 2019).  -> [(image path, [row index])]
    over data.vqa_tables rows: images in first-appearance order, an image's rows in table order."""
    by = {}
    for i, r in enumerate(rows):
        by.setdefault(r[0], []).append(i)
    return list(by.items())


class VqaGroupedDataset(torch.utils.data.Dataset):
    """VqaDataset with one item per IMAGE: item (epoch, image) -> (uint8 [H, W, 3], ids [n, T], seg, mask, answer
    indices [n], table rows [n]) of the image's n questions, the image decoded once.  categories as VqaDataset's: the
    item gains category ids [n].  Batches are packed by collate_grouped and drawn by GroupedBatchSampler, which counts
    QUESTIONS: an image with more than batch_size of them is refused when the sampler is built."""

    def __init__(self, rows, tokenizer, max_position_embeddings=28, categories=None):
        self.rows, self.tok, self.T = list(rows), tokenizer, max_position_embeddings
        self.images = group_rows_by_image(self.rows)
        self.categories = None if categories is None else dict(categories)
        if self.categories is not None:
            missing = sorted({r[3] for r in self.rows} - set(self.categories))
            if missing:
                raise ValueError(f"VqaGroupedDataset: categories {missing} of the rows are not in the category map")
        self.collate = collate_grouped

    def __len__(self):
        return len(self.images)

    def counts(self):
        return [len(idx) for _, idx in self.images]

    def batch_sampler(self, batch_size, shuffle, seed=0, rank=0, world=1):
        return GroupedBatchSampler(self.counts(), batch_size, shuffle, seed, rank, world)

    def __getitem__(self, key):
        _epoch, i = key
        path, idx = self.images[i]
        enc = [text.encode_text_vqa(self.rows[r][1], self.tok, self.T) for r in idx]
        ids, seg, mask = (torch.tensor([e[k] for e in enc], dtype=torch.long) for k in range(3))
        item = (decode(path), ids, seg, mask, torch.tensor([self.rows[r][2] for r in idx], dtype=torch.long),
                torch.tensor(idx, dtype=torch.int64))
        if self.categories is None:
            return item
        return item + (torch.tensor([self.categories[self.rows[r][3]] for r in idx], dtype=torch.int64),)


def collate_grouped(items):
    """-> dict: pixels / shapes [NI, 2] per IMAGE as collate packs them; ids / seg / mask [B, T], target, index [B]
    (table rows) and, where the items carry it, category [B] per QUESTION, an image's questions adjacent and in table
    order; group [B] int64 on the host, group[b] = the batch's image of question b (Model.forward_grouped)."""
    imgs = [it[0] for it in items]
    cat = lambda k: torch.cat([it[k] for it in items])   # noqa: E731
    out = dict(pixels=torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs])),
               shapes=torch.tensor([a.shape[:2] for a in imgs], dtype=torch.int64),
               ids=cat(1), seg=cat(2), mask=cat(3), target=cat(4), index=cat(5),
               group=torch.repeat_interleave(torch.arange(len(items)), torch.tensor([it[1].shape[0] for it in items])))
    if len(items[0]) > 6:
        out["category"] = cat(6)
    return out


# --------------------------------------------------------------------------- cached visual tokens
def image_of_rows(rows):
    """-> (image paths in first-appearance order, image index of every table row): the index <-> table-row map of a
    token cache over data.vqa_tables rows (row r asks about image image_of[r]; group_rows_by_image's numbering)"""
    images = group_rows_by_image(rows)
    image_of = [0] * len(rows)
    for i, (_, idx) in enumerate(images):
        for r in idx:
            image_of[r] = i
    return [p for p, _ in images], image_of


class VqaImageDataset(torch.utils.data.Dataset):
    """The distinct images of a VQA table, for the fill of a token cache: item (epoch, i) -> image i decoded, in the item
    layout `collate` packs, with one-token dummy text (the fill runs the backbone alone) and index = i, the row of the
    cache the image's tokens go to."""

    def __init__(self, rows):
        self.paths, self.image_of = image_of_rows(rows)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, key):
        _epoch, i = key
        z = torch.zeros(1, dtype=torch.long)
        return decode(self.paths[i]), z, z, z, torch.tensor(0, dtype=torch.long), i


class VqaTextDataset(torch.utils.data.Dataset):
    """VqaDataset without its images, for steps from a token cache: item (epoch, row) -> (ids, seg, mask, answer index,
    image index, row[, category id]).  Nothing is decoded: the workers tokenise only.  image index is image_of_rows'
    numbering, the one VqaImageDataset fills the cache in.  categories as VqaDataset's."""

    def __init__(self, rows, tokenizer, max_position_embeddings=28, categories=None):
        self.rows, self.tok, self.T = list(rows), tokenizer, max_position_embeddings
        self.paths, self.image_of = image_of_rows(self.rows)
        self.categories = None if categories is None else dict(categories)
        if self.categories is not None:
            missing = sorted({r[3] for r in self.rows} - set(self.categories))
            if missing:
                raise ValueError(f"VqaTextDataset: categories {missing} of the rows are not in the category map")
        self.collate = collate_text

    def __len__(self):
        return len(self.rows)

    def __getitem__(self, key):
        _epoch, idx = key
        _path, question, ans = self.rows[idx][:3]
        ids, seg, mask = (torch.tensor(v, dtype=torch.long) for v in text.encode_text_vqa(question, self.tok, self.T))
        item = ids, seg, mask, torch.tensor(ans, dtype=torch.long), self.image_of[idx], idx
        return item if self.categories is None else item + (self.categories[self.rows[idx][3]],)


def collate_text(items):
    """VqaTextDataset items -> dict: ids / seg / mask [B, T], target [B], image [B] int64 (cache rows, stays on the
    host), index [B] (table rows) and, where the items carry it, category [B]"""
    out = dict(ids=torch.stack([it[0] for it in items]), seg=torch.stack([it[1] for it in items]),
               mask=torch.stack([it[2] for it in items]), target=torch.stack([it[3] for it in items]),
               image=torch.tensor([it[4] for it in items], dtype=torch.int64),
               index=torch.tensor([it[5] for it in items], dtype=torch.int64))
    if len(items[0]) > 6:
        out["category"] = torch.tensor([it[6] for it in items], dtype=torch.int64)
    return out


def collate_supcon(items):
    """RocoSupConDataset items -> collate's dict with n images and the text already in process_tensors' layout
    (supcon_utils.py:253-256): ids = (captions; translations), target = (caption targets; translation targets),
    seg / mask = the captions' twice -- the translation half keeps the caption's mask even where its length differs,
    as in the reference.  ids / seg / mask / target are [2n, T], index [n]."""
    imgs = [it[0] for it in items]
    pixels = torch.from_numpy(np.concatenate([np.ascontiguousarray(a).reshape(-1) for a in imgs]))
    col = lambda i: torch.stack([it[i] for it in items])   # noqa: E731
    seg, mask = col(3), col(4)
    return dict(pixels=pixels, shapes=torch.tensor([a.shape[:2] for a in imgs], dtype=torch.int64),
                ids=torch.cat([col(1), col(2)]), seg=torch.cat([seg, seg]), mask=torch.cat([mask, mask]),
                target=torch.cat([col(5), col(6)]), index=torch.tensor([it[7] for it in items], dtype=torch.int64))


def collate_supcon_cols(items):
    """collate_supcon for items that end with the translation column drawn (RocoSupConDataset(report_aug_col=True)):
    the same dict plus aug_col [n] int32 (1..3: which translation each sample drew) and row [n] int32 (= index; the
    pair (row, aug_col) names the translation text in the table's WordSets)"""
    out = collate_supcon([it[:8] for it in items])
    out["aug_col"] = torch.tensor([it[8] for it in items], dtype=torch.int32)
    out["row"] = out["index"].to(torch.int32)
    return out


def collate_supcon_teacher(items):
    """collate_supcon for items that end with the teacher rows of caption and drawn translation
    (RocoSupConDataset(teacher_tokenizer=...)): the same dict plus teacher int64 [2n, 1 + L] (captions, then translations:
    the order of `list(doc1) + list(doc2)`, supcon_utils.py:141) and teacher_T, the longest of the 2n lengths"""
    out = collate_supcon([it[:8] for it in items])
    t = torch.stack([it[8] for it in items])                        # [n, 2, 1 + L]
    out["teacher"] = torch.cat([t[:, 0], t[:, 1]]).contiguous()
    out["teacher_T"] = out["teacher"][:, 0].max()
    return out


class RocoSupConDataset(torch.utils.data.Dataset):
    """item (epoch, index) -> (uint8 [H, W, 3], ids, aug_ids, seg, mask, tgt, aug_tgt, index) as supcon_utils.py:218-232
    returns it (the image untransformed: both views are made on the device).  One rng, sample_rng(seed, epoch,
    index), is drawn in the reference's order: the caption's MLM masking, then randint(3, 5) for the translation
    column (get_translation), then the translation's masking.  The translation's seg / mask are not kept: the
    reference uses the caption's for both halves (process_tensors).
    report_aug_col=True (the Jaccard mask needs to know which translation was drawn): the item gains a ninth element,
    the drawn column as 1..3 (= CSV column - 2, the WordSets column), and batches are packed by collate_supcon_cols.
    teacher_tokenizer (the cosine mask of the BERT teacher; not with report_aug_col): the ninth element is int64
    [2, 1 + max_token_length], teacher_row of the caption and of the translation drawn, tokenised with the teacher's
    WordPiece; batches are packed by collate_supcon_teacher."""

    collate = staticmethod(collate_supcon)     # HostLoader packs its batches with it

    def __init__(self, rows, tokenizer, keywords, num_vis=5, max_position_embeddings=75, mlm_prob=0.15, seed=0,
                 report_aug_col=False, teacher_tokenizer=None, max_token_length=512):
        self.rows, self.tok, self.kw = list(rows), tokenizer, frozenset(keywords)
        self.num_vis, self.T, self.mlm_prob, self.seed = num_vis, max_position_embeddings, mlm_prob, seed
        self.report_aug_col = bool(report_aug_col)
        self.teacher_tok, self.L = teacher_tokenizer, int(max_token_length)
        if self.report_aug_col and teacher_tokenizer is not None:
            raise ValueError("RocoSupConDataset: report_aug_col and teacher_tokenizer are the ninth element of different masks' items")
        if self.report_aug_col:
            self.collate = collate_supcon_cols
        if teacher_tokenizer is not None:
            self.collate = collate_supcon_teacher

    def __len__(self):
        return len(self.rows)

    def encode_col(self, epoch, idx):
        """(the item's text, the translation column drawn as 1..3)"""
        _path, caption, trans = self.rows[idx]
        rng = sample_rng(self.seed, epoch, idx)
        ids, seg, mask, tgt = text.encode_text(caption, self.tok, self.kw, self.num_vis, self.T, self.mlm_prob, rng)
        col = rng.randint(3, 5) - 3
        aug_ids, _seg, _mask, aug_tgt = text.encode_text(trans[col], self.tok, self.kw, self.num_vis, self.T,
                                                         self.mlm_prob, rng)
        return (ids, aug_ids, seg, mask, tgt, aug_tgt), col + 1

    def encode(self, epoch, idx):
        """the item's text: (ids, aug_ids, seg, mask, tgt, aug_tgt)"""
        return self.encode_col(epoch, idx)[0]

    def __getitem__(self, key):
        epoch, idx = key
        enc, col = self.encode_col(epoch, idx)
        item = (decode(self.rows[idx][0]),) + enc + (idx,)
        if self.teacher_tok is not None:
            _path, caption, trans = self.rows[idx]
            return item + (torch.stack([teacher_row(self.teacher_tok, caption, self.L),
                                        teacher_row(self.teacher_tok, trans[col - 1], self.L)]),)
        return item + (col,) if self.report_aug_col else item


def unpack(batch):
    """collate's pixels + shapes -> list of uint8 [h, w, 3] arrays (host)"""
    px, out, o = batch["pixels"].numpy(), [], 0
    for h, w in batch["shapes"].tolist():
        out.append(px[o:o + h * w * 3].reshape(h, w, 3))
        o += h * w * 3
    return out


def offsets(shapes):
    """byte offset of each image in collate's pixels"""
    sz = [h * w * 3 for h, w in shapes.tolist()]
    return [0] + np.cumsum(sz)[:-1].tolist()


class EpochBatchSampler(torch.utils.data.Sampler):
    """batches of (epoch, index): seeded permutation per epoch (or file order), this rank's DistributedSampler shard,
    partial last batch kept"""

    def __init__(self, n, batch_size, shuffle, seed=0, rank=0, world=1):
        self.n, self.bs, self.shuffle, self.seed, self.rank, self.world = n, batch_size, shuffle, seed, rank, world
        self.epoch = 0

    def indices(self):
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            idx = torch.randperm(self.n, generator=g).tolist()
        else:
            idx = list(range(self.n))
        total = int(math.ceil(self.n / self.world)) * self.world
        idx += (idx * int(math.ceil(total / max(self.n, 1))))[:total - self.n]
        return idx[self.rank:total:self.world]

    def __iter__(self):
        idx = self.indices()
        for lo in range(0, len(idx), self.bs):
            yield [(self.epoch, i) for i in idx[lo:lo + self.bs]]

    def __len__(self):
        return -(-int(math.ceil(self.n / self.world)) // self.bs)


class GroupedBatchSampler(EpochBatchSampler):
    """EpochBatchSampler over IMAGES whose batches are sized in QUESTIONS: counts[i] = the questions of image i.  The
    images come in the same seeded epoch order; a batch is closed when the next image's questions would push it past
    batch_size, so no batch holds more than batch_size questions and none is empty.  An image with more questions than
    batch_size cannot be placed and is refused here, when the loader is built.

    Ranks: the WHOLE epoch order is packed first and whole batches are dealt to the ranks (batch j goes to rank
    j % world), the list padded from its head to a multiple of world as the ungrouped shard pads its images.  Every rank
    therefore runs the same number of steps, whatever the counts: a data-parallel step is one gradient all-reduce, and
    ranks that packed their own image shards would close their batches at different places and fall out of step.  The
    batches of an epoch are a function of (seed, epoch, rank) and the table alone."""

    def __init__(self, counts, batch_size, shuffle, seed=0, rank=0, world=1):
        self.counts = [int(c) for c in counts]
        super().__init__(len(self.counts), batch_size, shuffle, seed, rank, world)
        worst = max(self.counts, default=0)
        if worst > batch_size:
            raise ValueError(f"an image of the table has {worst} questions, more than --batch_size {batch_size} (which "
                             "counts questions): it fits no grouped batch")

    def order(self):
        """the epoch's order of all images, the same on every rank"""
        if self.shuffle:
            g = torch.Generator().manual_seed(self.seed + self.epoch)
            return torch.randperm(self.n, generator=g).tolist()
        return list(range(self.n))

    def all_batches(self):
        """the epoch's batches before they are dealt to the ranks"""
        out, cur, n = [], [], 0
        for i in self.order():
            if cur and n + self.counts[i] > self.bs:
                out.append(cur)
                cur, n = [], 0
            cur.append(i)
            n += self.counts[i]
        if cur:
            out.append(cur)
        return out

    def batches(self):
        """this rank's batches: every world-th of all_batches, padded from the head so that all ranks have as many"""
        allb = self.all_batches()
        total = int(math.ceil(len(allb) / self.world)) * self.world
        allb += (allb * int(math.ceil(total / max(len(allb), 1))))[:total - len(allb)]
        return allb[self.rank:total:self.world]

    def indices(self):
        return [i for b in self.batches() for i in b]

    def __iter__(self):
        for b in self.batches():
            yield [(self.epoch, i) for i in b]

    def __len__(self):
        return len(self.batches())


class HostLoader:
    """iterates one epoch of host batches: (batch dict, augment params or None, {"epoch", "batch"}).  With views=V the
    params are V per image, sample_params(V * n, ...) from the batch's generator: params[i * V + v] is view v of
    image i (TwoCropTransform's V calls in a row).  A dataset with a `collate` attribute packs its own batches, one with
    a `batch_sampler` method draws them (VqaGroupedDataset: batch_size counts questions, the params stay one set per
    IMAGE, so every question of an image sees the same view in a step)."""

    def __init__(self, dataset, batch_size, shuffle=True, seed=0, rank=0, world=1, num_workers=None, aug=None,
                 size=224, pin_memory=True, views=1):
        if int(views) < 1:
            raise ValueError("views must be >= 1")
        if hasattr(dataset, "batch_sampler"):
            self.sampler = dataset.batch_sampler(batch_size, shuffle, seed, rank, world)
        else:
            self.sampler = EpochBatchSampler(len(dataset), batch_size, shuffle, seed, rank, world)
        self.seed, self.rank, self.aug, self.size, self.views = seed, rank, aug, size, int(views)
        self.num_workers = default_workers() if num_workers is None else int(num_workers)
        kw = {}
        if self.num_workers > 0:
            kw = dict(multiprocessing_context="forkserver", persistent_workers=True, prefetch_factor=2)
        self.loader = torch.utils.data.DataLoader(dataset, batch_sampler=self.sampler, num_workers=self.num_workers,
                                                  collate_fn=getattr(dataset, "collate", None) or collate,
                                                  pin_memory=bool(pin_memory) and torch.cuda.is_available(), **kw)

    def set_epoch(self, epoch):
        self.sampler.epoch = int(epoch)

    def __len__(self):
        return len(self.sampler)

    def __iter__(self):
        epoch = self.sampler.epoch
        for b, batch in enumerate(self.loader):
            params = None
            if self.aug is not None:
                n = batch["shapes"].shape[0]
                params = sample_params(self.views * n, self.size, generator=batch_generator(self.seed, epoch, b, self.rank),
                                       **self.aug)
            yield batch, params, dict(epoch=epoch, batch=b)


def view_params(seed, image, view, size, aug):
    """the training-augmentation parameters of view `view` >= 1 of cache image `image`: a function of (seed, image,
    view) alone, whatever batch the image is filled in"""
    g = torch.Generator().manual_seed(mix_seed(seed, image, view, 0x746F6B))
    return sample_params(1, size, generator=g, **aug)[0]


class ViewLoader(HostLoader):
    """HostLoader over a VqaImageDataset in file order for the fill of one view of a token cache: view 0 carries no
    augment parameters (the feeder applies the evaluation transform), view v >= 1 carries view_params(seed, i, v) for
    every image i of the batch -- not a draw from the batch's generator, so a view does not depend on the batch size."""

    def __init__(self, dataset, batch_size, view, seed=0, num_workers=None, aug=None, size=224):
        super().__init__(dataset, batch_size, shuffle=False, seed=seed, num_workers=num_workers,
                         aug=aug if view else None, size=size)
        self.view = int(view)

    def __iter__(self):
        for b, batch in enumerate(self.loader):
            params = None
            if self.aug is not None:
                params = [view_params(self.seed, i, self.view, self.size, self.aug) for i in batch["index"].tolist()]
            yield batch, params, dict(epoch=self.view, batch=b)


def low_priority_stream(device):
    """(torch stream, priority): the library's least-priority stream of `device`, kept for the life of the process"""
    import ctypes as C
    from . import _lib as L
    with torch.cuda.device(device):
        h, prio = C.c_void_p(), C.c_int()
        L.check(L.lib().mmvqa_low_priority_stream(C.byref(h), C.byref(prio)))
        return torch.cuda.ExternalStream(h.value, device=device), prio.value


class _Slot:
    def __init__(self):
        self.tensors = None       # device buffers of the batch in this slot (reused)
        self.ready = None         # recorded on the feeder stream after the batch's copies and augment
        self.free = None          # recorded on the consumer's stream when it moved past the batch


class DeviceFeeder:
    """Iterator over device batches (img fp32 [B, 3, S, S], ids, seg, mask, target) of one epoch of a HostLoader.
    With views=V (the HostLoader's, SupCon: 2) a batch of n images gives img [V * n, 3, S, S], view-major (row
    v * n + i = view v of image i), and the text tensors as the host batch holds them.

    `depth` device slots rotate.  When batch n is handed out, batches up to n + depth - 1 are already enqueued on the
    feeder's stream (pinned H2D copies with non_blocking=True, then DeviceAugment.run_packed), so batch n + 1's copy
    and augment are in the queue before the step of batch n syncs the host.  __next__ makes the caller's current
    stream wait on the batch's ready event.  A slot is refilled only after the feeder stream has waited on an event
    the consumer's stream recorded when the consumer moved on (the next __next__): the batch it returned stays valid
    on that stream until then.

    The feeder stream has the LEAST priority the device offers (HIP priority 1, below the normal 0 of the step's
    streams; the library creates it, as torch's own stream pools on ROCm stop at normal priority): the augment is there
    to fill the gaps the step leaves, and should yield to the step's kernels when both are ready.

    The refill (DataLoader get + run_packed's packing, ~2 ms of host time per batch) runs inside __next__: in a
    loop that syncs every step it sits between one step's sync and the next step's first launch.

    log: one entry per batch handed out -- epoch, batch, dataset rows and the augment params used (tests rebuild the
    batch from it).

    pairs=True (SupCon with the Jaccard mask; the host batches must carry `row` and `aug_col`, i.e. come from a
    RocoSupConDataset(report_aug_col=True)): the batch is a 6-tuple whose last element is (rows, cols), two int32 device
    tensors [n] naming the translation text (table row, WordSets column 1..3) of each sample.  They live in the slot and
    are copied on the feeder's stream with the rest of it: same ready event, same reuse rule.  The log entry gains
    `aug_col`.  With pairs=False (default) the batch stays the 5-tuple.

    category=True (VQA with label smoothing by category; the host batches must carry `category`, i.e. come from a
    VqaDataset(categories=...)): the batch is a 6-tuple whose last element is category, an int64 device tensor [B] of
    category ids.  It lives in the slot and is copied on the feeder's stream like the rest: same ready event, same reuse
    rule.  The log entry gains `category`.  Not together with pairs.

    teacher=True (SupCon with the BERT teacher's cosine mask; the host batches must carry `teacher`, i.e. come from a
    RocoSupConDataset(teacher_tokenizer=...)): the batch is a 6-tuple whose last element is the int64 device tensor
    [2n, 1 + L] of teacher rows (data.teacher_row: length, ids), in the slot like the rest.  Not together with pairs or
    category.  Whenever a host batch carries `teacher_T` (this one, or OnlineDistillDataset's, whose teacher rows are the
    batch's fifth tensor) the log entry gains `teacher_T`, the batch's longest teacher input as a host integer.

    grouped=True (VQA with --group_by_image; the host batches come from a VqaGroupedDataset): img holds the batch's NI
    images, the text tensors and target its B >= NI questions, and the batch tuple ends with `group`, the int64 HOST
    tensor [B] naming the image of each question (after category, where both are on).  The augment parameters are one
    set per IMAGE, so every question of an image sees the same view in a step -- the ungrouped loop draws a view per
    question.  The log entry gains `group`; `index` names the table rows of the questions."""

    def __init__(self, host: HostLoader, device, train=True, depth=2, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5),
                 fused=True, pairs=False, category=False, teacher=False, grouped=False):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("DeviceFeeder runs on the GPU only (no CPU fallback)")
        if depth < 1:
            raise ValueError("depth must be >= 1")
        self.host, self.dev, self.depth, self.fused = host, device, int(depth), fused
        self.views = getattr(host, "views", 1)
        self.pairs, self.category, self.teacher = bool(pairs), bool(category), bool(teacher)
        if self.pairs + self.category + self.teacher > 1:
            raise ValueError("DeviceFeeder: pairs, category and teacher are the sixth element of different loops' batches")
        self.grouped = bool(grouped)
        if self.grouped and (self.pairs or self.teacher or self.views != 1):
            raise ValueError("DeviceFeeder: grouped batches are the VQA loop's (one view, no pairs, no teacher)")
        aug = host.aug or {}
        self.aug = DeviceAugment(size=host.size, train=train, mean=mean, std=std, device=device, **aug)
        self.stream, self.priority = low_priority_stream(device)
        self.slots = [_Slot() for _ in range(self.depth)]
        self.log = []
        self._it = None

    def set_epoch(self, epoch):
        self.host.set_epoch(epoch)

    def __len__(self):
        return len(self.host)

    def __iter__(self):
        self._release()                # a consumer that left the last epoch early is still done with its batch
        self._it = iter(self.host)
        self._queue = deque()          # (slot, batch tuple, log entry) enqueued and not yet handed out
        self._next_slot = 0
        self._out = None               # slot handed out last
        self._done = False
        while len(self._queue) < self.depth and self._enqueue():
            pass
        return self

    def _buffers(self, slot, NI, B, T):
        t = slot.tensors
        S = self.aug.size
        if t is None or t["img"].shape[0] < NI or t["ids"].shape[0] < B or t["ids"].shape[1] != T:
            with torch.cuda.stream(self.stream):
                t = slot.tensors = dict(
                    img=torch.empty(NI, 3, S, S, dtype=torch.float32, device=self.dev),
                    **{k: torch.empty(B, T, dtype=torch.int64, device=self.dev) for k in ("ids", "seg", "mask")},
                    target=None)
        return t

    def _enqueue(self):
        if self._done:
            return False
        try:
            batch, params, meta = next(self._it)
        except StopIteration:
            self._done = True
            return False
        slot = self.slots[self._next_slot]
        self._next_slot = (self._next_slot + 1) % self.depth
        s = self.stream
        if slot.free is not None:
            s.wait_event(slot.free)         # the consumer is done with what this slot held
        B, T = batch["ids"].shape
        NI = self.views * batch["shapes"].shape[0]          # image rows: views x images
        buf = self._buffers(slot, NI, B, T)
        with torch.cuda.stream(s):
            tgt = batch["target"]
            if buf["target"] is None or buf["target"].shape[0] < B or buf["target"].shape[1:] != tgt.shape[1:]:
                buf["target"] = torch.empty((max(B, buf["ids"].shape[0]),) + tuple(tgt.shape[1:]), dtype=tgt.dtype,
                                            device=self.dev)
            pix = batch["pixels"].to(self.dev, non_blocking=True)
            img = buf["img"][:NI]
            self.aug.run_packed(pix, offsets(batch["shapes"]), batch["shapes"], params, s, fused=self.fused, out=img,
                                views=self.views)
            out = [img]
            for k in ("ids", "seg", "mask", "target"):
                d = buf[k][:B]
                d.copy_(batch[k], non_blocking=True)
                out.append(d)
            if self.pairs:
                if "aug_col" not in batch or "row" not in batch:
                    raise ValueError("DeviceFeeder(pairs=True): the host batches carry no `row` / `aug_col` "
                                     "(RocoSupConDataset(report_aug_col=True) reports them)")
                n = batch["row"].shape[0]
                if buf.get("pair") is None or buf["pair"].shape[1] < n:
                    buf["pair"] = torch.empty(2, max(n, NI // self.views), dtype=torch.int32, device=self.dev)
                rows, cols = buf["pair"][0, :n], buf["pair"][1, :n]
                rows.copy_(batch["row"], non_blocking=True)
                cols.copy_(batch["aug_col"], non_blocking=True)
                out.append((rows, cols))
            if self.category:
                if "category" not in batch:
                    raise ValueError("DeviceFeeder(category=True): the host batches carry no `category` "
                                     "(VqaDataset(categories=...) reports it)")
                if buf.get("category") is None or buf["category"].shape[0] < B:
                    buf["category"] = torch.empty(max(B, buf["ids"].shape[0]), dtype=torch.int64, device=self.dev)
                cat = buf["category"][:B]
                cat.copy_(batch["category"], non_blocking=True)
                out.append(cat)
            if self.teacher:
                if "teacher" not in batch:
                    raise ValueError("DeviceFeeder(teacher=True): the host batches carry no `teacher` "
                                     "(RocoSupConDataset(teacher_tokenizer=...) reports it)")
                tr = batch["teacher"]
                if buf.get("teacher") is None or buf["teacher"].shape[0] < tr.shape[0] or buf["teacher"].shape[1] != tr.shape[1]:
                    buf["teacher"] = torch.empty(max(tr.shape[0], NI), tr.shape[1], dtype=torch.int64, device=self.dev)
                td = buf["teacher"][:tr.shape[0]]
                td.copy_(tr, non_blocking=True)
                out.append(td)
            if self.grouped:
                if "group" not in batch:
                    raise ValueError("DeviceFeeder(grouped=True): the host batches carry no `group` "
                                     "(VqaGroupedDataset reports it)")
                out.append(batch["group"].clone())     # stays on the host: Model.forward_grouped validates it there
            slot.ready = torch.cuda.Event()
            slot.ready.record(s)
        entry = dict(meta, index=batch["index"].tolist(), params=params, shapes=batch["shapes"].tolist())
        if self.pairs:
            entry["aug_col"] = batch["aug_col"].tolist()
        if self.category:
            entry["category"] = batch["category"].tolist()
        if "teacher_T" in batch:
            entry["teacher_T"] = int(batch["teacher_T"])
        if self.grouped:
            entry["group"] = batch["group"].tolist()
        self._queue.append((slot, tuple(out), entry))
        return True

    def _release(self):
        """the slot handed out last is free once the consumer's stream reaches this point"""
        if getattr(self, "_out", None) is None:
            return False
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self._out.free = ev
        self._out = None
        return True

    def __next__(self):
        if self._it is None:
            iter(self)
        cur = torch.cuda.current_stream(self.dev)
        if self._release():                 # the consumer moved past the previous batch: its slot may be refilled
            while len(self._queue) < self.depth and self._enqueue():
                pass
        if not self._queue:
            self._it = None
            raise StopIteration
        slot, out, entry = self._queue.popleft()
        cur.wait_event(slot.ready)
        self._out = slot
        self.log.append(entry)
        return out
