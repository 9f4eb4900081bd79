"""Host-side mirror of the reference's ``Model(args)`` protocol over the HIP engine.

Reference interface mirrored here:
  * ``Model(args)``                      -- models/mmbert.py:129-148
  * ``model(img, ids, seg, mask)``       -- models/mmbert.py:150-167 (Tensor | (logits, feat) | (logits, 0, 0));
                                            with dataset 'roco' and task 'distillation' (:159-161) the Tensor is the
                                            encoder output h [B, T, hidden]: no fc1, no classifier, no SupCon head even
                                            when ``supcon`` is set; their parameters stay in the state_dict and never
                                            receive a gradient (engine head kind 2)
  * ``.to() .train() .eval() .parameters() .state_dict() .load_state_dict()``
  * ``model.classifier[2] = nn.Linear(hidden, num_classes)`` -- vqamed2019/train.py:137
Parameter names and logical shapes equal the reference's state_dict; storage is ONE flat fp32
buffer per kind (params / grads / BN buffers) owned by PyTorch, whose layout the C++ engine
defines (mmvqa_engine_tensor_info).  All arithmetic runs in libmmvqa_hip.so; there is no
PyTorch fallback -- forward() on a non-GPU tensor or without the library raises.
"""
from __future__ import annotations

import ctypes as C
import math
import operator

import torch
import torch.nn as nn

from . import _lib as L

# parameters the reference never uses => their .grad stays None
_NEVER_USED = ("transformer.blocks.norm2.", "transformer.trans.model.fc.",
               "transformer.block.token_emb.", "transformer.block.to_logits.")

# the Feedback Transformer's one to_kv weight (feedback_transformer_pytorch.py:229-230,246): the engine lists it under the
# reference's first name; the reference's state_dict carries it under every layer's name and as shared_kv_proj
_FB = "transformer.block."
_BACKBONE = "transformer.trans.model."   # the CNN body (models/image_encoding.py:43-62); the five tap convolutions are not in it
_NOT_FROZEN = (0, ())
_TOKEN_PLAN_HW = 64                      # image size of the workspace layout behind forward_tokens (its backbone never runs)
_REQUIRES_GRAD = operator.attrgetter("requires_grad")
_FB_KV = _FB + "layers.0.0.fn.fn.to_kv.weight"


def _fb_kv_aliases(n_layers):
    return [f"{_FB}layers.{i}.0.fn.fn.to_kv.weight" for i in range(1, n_layers)] + [_FB + "shared_kv_proj.weight"]


def desc_from_args(args, feat_dim=128, n_classes=None) -> L.ModelDesc:
    """Translate the argparse Namespace the reference passes to Model(args)."""
    d = L.ModelDesc()
    enc = args.cnn_encoder
    if "resnet" in enc:
        d.cnn = 0
    elif "efficientnetv2" in enc:
        d.cnn = 1
    else:
        raise NotImplementedError(enc)  # models/image_encoding.py:41
    layers = getattr(args, "resnet_layers", (3, 8, 36, 3))
    for i in range(4):
        d.resnet_layers[i] = int(layers[i])
    d.resnet_width = int(getattr(args, "resnet_width", 64))
    d.effnet_depth_div = int(getattr(args, "effnet_depth_div", 1))
    tm = args.transformer_model
    if "feedback-transformer" in tm:     # models/mmbert.py:38-43 tests this string first
        d.encoder = L.ENC_FEEDBACK
    elif "realformer" in tm:
        d.encoder = 1
    elif "transformer" in tm:
        d.encoder = 0
    else:
        raise NotImplementedError(tm)  # models/mmbert.py:42
    d.hidden = int(args.hidden_size)
    d.heads = int(getattr(args, "heads", 12))
    d.n_layers = int(args.n_layers)
    d.emb_vocab = int(getattr(args, "emb_vocab", 30522))
    d.max_pos = int(getattr(args, "bert_max_pos", 512))
    d.type_vocab = 2
    d.num_vis = int(args.num_vis)
    if args.dataset == "roco":
        task = getattr(args, "task", "MLM")
        if task == "MLM":
            d.head_kind = L.HEAD_MLM
        elif task == "distillation":          # models/mmbert.py:159-161: the model returns the encoder output h
            d.head_kind = L.HEAD_NONE
        else:
            raise NotImplementedError(f"task={task!r}: only 'MLM' and 'distillation' are on the hot path")
    elif args.dataset == "VQA-Med":
        d.head_kind = 1
    else:
        raise NotImplementedError(args.dataset)
    d.n_classes = int(n_classes if n_classes is not None else args.vocab_size)
    d.supcon = 1 if (getattr(args, "supcon", False) and d.head_kind == 0) else 0
    d.feat_dim = int(feat_dim)
    d.use_relu = 1 if getattr(args, "use_relu", False) else 0
    d.p_drop = float(getattr(args, "hidden_dropout_prob", 0.3))
    d.p_emb_drop = float(getattr(args, "emb_dropout_prob", 0.1))
    d.p_rf_drop = float(getattr(args, "rf_dropout_prob", 0.1))
    d.p_fb_drop = float(getattr(args, "fb_dropout_prob", 0.1))   # mmbert.py:118-119: attn_dropout = ff_dropout = 0.1
    d.fb_tokens = int(args.vocab_size)
    return d


class _Node(nn.Module):
    """plain container so that dotted state_dict names resolve to a module tree"""


class _HeadSeq(_Node):
    """``model.classifier``: indexable like nn.Sequential; assigning item 2 re-heads the model
    (vqamed2019/train.py:137,141,149: ``model.classifier[2] = nn.Linear(hidden, num_classes)``)."""

    def __init__(self, owner):
        super().__init__()
        object.__setattr__(self, "_owner", owner)

    def __getitem__(self, i):
        return getattr(self, str(i))

    def __setitem__(self, i, module):
        if int(i) != 2 or not isinstance(module, nn.Linear):
            raise NotImplementedError("only classifier[2] = nn.Linear(...) is supported")
        self._owner._rehead(module)

    def __len__(self):
        return 3


class _ModelFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, anchor, img, ids, seg, mask, prec, frozen):
        ctx.model = model
        ctx.prec = prec
        ctx.frozen = frozen   # (engine flags, [lo, hi) ranges of flat_grads without gradient) as this forward read them
        return model._engine_forward(img, ids, seg, mask, prec, frozen[0])

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._engine_backward(*grads, prec=ctx.prec, frozen=ctx.frozen)
        return (None,) * 8


class _GroupedModelFn(torch.autograd.Function):
    """_ModelFn for a grouped batch: `maps` is the device copy of group | offsets (group_maps)"""

    @staticmethod
    def forward(ctx, model, anchor, img, maps, ids, seg, mask, prec, frozen):
        ctx.model = model
        ctx.prec = prec
        ctx.frozen = frozen
        return model._engine_forward(img, ids, seg, mask, prec, frozen[0], maps=maps)

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._engine_backward(*grads, prec=ctx.prec, frozen=ctx.frozen)
        return (None,) * 9


class _CachedModelFn(torch.autograd.Function):
    """_ModelFn for a step from the token cache: `maps` is the device copy of index | view (cached_maps)"""

    @staticmethod
    def forward(ctx, model, anchor, tokens, maps, ids, seg, mask, frozen):
        ctx.model = model
        ctx.frozen = frozen
        return model._engine_forward_cached(tokens, maps, ids, seg, mask)

    @staticmethod
    def backward(ctx, *grads):
        ctx.model._engine_backward_cached(*grads, frozen=ctx.frozen)
        return (None,) * 8


def _host_ints(what, values):
    """a host integer tensor or sequence -> list of int; ValueError for a device tensor, a float, a bool"""
    if isinstance(values, torch.Tensor):
        if values.is_cuda:
            raise ValueError(f"{what} must be a host tensor or a sequence: it is validated before anything is launched")
        if values.dtype.is_floating_point or values.dtype == torch.bool or values.dim() != 1:
            raise ValueError(f"{what} must be a 1-d integer tensor, not {values.dtype} with shape {tuple(values.shape)}")
        return [int(v) for v in values.tolist()]
    out = list(values)
    for b, v in enumerate(out):
        if isinstance(v, bool) or not isinstance(v, (int, float)) and not hasattr(v, "__index__") or int(v) != v:
            raise ValueError(f"{what} must hold integers, not {v!r} at position {b}")
    return [int(v) for v in out]


def cached_maps(index, view, n_images: int, n_views: int, n_rows: int):
    """Validates the (image, view) choice of a step from a TokenCache on the host and returns one int32 CPU tensor
    [2 * n_rows]: index, then view.  Both are host integer tensors or sequences of length n_rows with
    0 <= index[b] < n_images and 0 <= view[b] < n_views; ValueError names the first offending position otherwise.  The
    kernels that read them do not check ranges."""
    idx, vw = _host_ints("index", index), _host_ints("view", view)
    for what, vals, bound, of in (("index", idx, n_images, "images"), ("view", vw, n_views, "views")):
        if len(vals) != n_rows:
            raise ValueError(f"{what} has {len(vals)} entries for {n_rows} rows")
        for b, v in enumerate(vals):
            if not 0 <= v < bound:
                raise ValueError(f"{what}[{b}] = {v} is outside the cache's {bound} {of} (0 .. {bound - 1})")
    return torch.tensor(idx + vw, dtype=torch.int32)


def group_maps(group, n_images: int, n_rows: int):
    """Validates the image-of-question map of a grouped batch on the host and returns one int32 CPU tensor
    [n_rows + n_images + 1]: group, then offsets (the questions of image i are rows offsets[i] .. offsets[i+1]-1).
    `group` is a host integer tensor or sequence of length n_rows: non-decreasing, starting at 0, rising by at most 1,
    ending at n_images - 1 -- the questions of an image are adjacent and every image has one.  ValueError otherwise."""
    if isinstance(group, torch.Tensor):
        if group.is_cuda:
            raise ValueError("group must be a host tensor or a sequence: it is validated before anything is launched")
        if group.dtype.is_floating_point or group.dtype == torch.bool or group.dim() != 1:
            raise ValueError(f"group must be a 1-d integer tensor, not {group.dtype} with shape {tuple(group.shape)}")
        g = [int(v) for v in group.tolist()]
    else:
        g = list(group)
        if any(isinstance(v, bool) or int(v) != v for v in g):
            raise ValueError("group must hold integers")
        g = [int(v) for v in g]
    if n_images < 1 or n_rows < n_images:
        raise ValueError(f"a grouped batch has 1 <= images <= questions, not {n_images} images for {n_rows} questions")
    if len(g) != n_rows:
        raise ValueError(f"group has {len(g)} entries for {n_rows} questions")
    if min(g) < 0:
        raise ValueError(f"group holds a negative image index ({min(g)})")
    if g[0] != 0:
        raise ValueError(f"group must start at image 0, not {g[0]}")
    offsets = [0]
    for b in range(1, n_rows):
        step = g[b] - g[b - 1]
        if step < 0:
            raise ValueError(f"group decreases at question {b} ({g[b - 1]} -> {g[b]}): the questions of an image are adjacent")
        if step > 1:
            raise ValueError(f"group skips from image {g[b - 1]} to {g[b]} at question {b}: every image has a question")
        if step:
            offsets.append(b)
    offsets.append(n_rows)
    if g[-1] != n_images - 1:
        raise ValueError(f"group ends at image {g[-1]}, the batch has {n_images} images (last index {n_images - 1})")
    return torch.tensor(g + offsets, dtype=torch.int32)


def autocast_precision(model_desc) -> int:
    """Operand precision of a forward run now: PREC_F16 inside torch.autocast("cuda", dtype=torch.float16) (what the
    reference's torch.cuda.amp.autocast() means), PREC_F32 outside autocast.  Any other autocast dtype, and an
    EfficientNet encoder under fp16 autocast, raise NotImplementedError instead of running silently in fp32."""
    if not torch.is_autocast_enabled("cuda"):
        return L.PREC_F32
    dt = torch.get_autocast_dtype("cuda")
    if dt != torch.float16:
        raise NotImplementedError(f"mixed precision supports torch.autocast('cuda', dtype=torch.float16) only, not {dt}")
    if model_desc.cnn != 0:
        raise NotImplementedError("mixed precision (fp16 autocast) supports the ResNet encoders only, not "
                                  "tf_efficientnetv2_m: its squeeze-excite, depthwise and thin tap products run "
                                  "outside the implicit GEMM")
    return L.PREC_F16


class Model(nn.Module):
    def __init__(self, args, feat_dim=128, device=None):
        super().__init__()
        self._args = args
        self._feat_dim = feat_dim
        self.task = getattr(args, "task", "MLM")
        self.dataset = args.dataset
        self.supcon = bool(getattr(args, "supcon", False))
        self._handle = None
        self._plan_key = None
        self._ws = None
        self._seed_ctr = 0
        self._fwd_state = None
        self._bn_stats_running = False
        dev = torch.device(device) if device is not None else torch.device("cpu")
        self._build(desc_from_args(args, feat_dim), dev, init=True)

    # ------------------------------------------------------------------ construction
    def _build(self, desc, dev, init, old_state=None):
        lib = L.lib()
        if self._handle is not None:
            lib.mmvqa_engine_destroy(self._handle)
            self._handle = None
        h = C.c_void_p()
        L.check(lib.mmvqa_engine_create(C.byref(desc), C.byref(h)))
        self._handle = h
        self._desc = desc
        self._plan_key = None
        n_p = lib.mmvqa_engine_param_floats(h)
        n_b = lib.mmvqa_engine_buf_floats(h)
        n_n = max(1, lib.mmvqa_engine_nbt_count(h))
        self._flat = {
            0: torch.zeros(n_p, dtype=torch.float32, device=dev),
            1: torch.zeros(max(4, n_b), dtype=torch.float32, device=dev),
            2: torch.zeros(n_n, dtype=torch.int64, device=dev),
        }
        self._flat_grad = torch.zeros(n_p, dtype=torch.float32, device=dev)
        self._anchor = torch.zeros(1, dtype=torch.float32, device=dev, requires_grad=True)
        # drop the old module tree
        for name in list(self._modules.keys()):
            del self._modules[name]
        self._table = []
        name_buf = C.create_string_buffer(256)
        kind, ndim, cl = C.c_int(), C.c_int(), C.c_int()
        shape = (C.c_longlong * 4)()
        off = C.c_longlong()
        for i in range(lib.mmvqa_engine_num_tensors(h)):
            L.check(lib.mmvqa_engine_tensor_info(h, i, name_buf, 256, C.byref(kind), C.byref(ndim),
                                                 C.byref(shape), C.byref(off), C.byref(cl)))
            name = name_buf.value.decode()
            shp = tuple(int(shape[k]) for k in range(ndim.value))
            self._table.append((name, kind.value, shp, int(off.value), bool(cl.value)))
        self._params_by_name = {}
        for name, kind, shp, off, cl in self._table:
            view = self._view(self._flat[kind], shp, off, cl)
            parts = name.split(".")
            mod = self
            for j, p in enumerate(parts[:-1]):
                if p not in mod._modules:
                    child = _HeadSeq(self) if (j == 0 and p == "classifier") else _Node()
                    mod.add_module(p, child)
                mod = mod._modules[p]
            if kind == 0:
                prm = nn.Parameter(view, requires_grad=True)
                mod.register_parameter(parts[-1], prm)
                self._params_by_name[name] = prm
            else:
                mod.register_buffer(parts[-1], view)
        if desc.encoder == L.ENC_FEEDBACK:
            shared = self._params_by_name[_FB_KV]
            for name in _fb_kv_aliases(desc.n_layers):
                parts = name.split(".")
                mod = self
                for p in parts[:-1]:
                    if p not in mod._modules:
                        mod.add_module(p, _Node())
                    mod = mod._modules[p]
                mod.register_parameter(parts[-1], shared)   # the same Parameter: named_parameters() lists it once
        if init:
            self._init_weights()
        if old_state is not None:
            own = self.state_dict()
            keep = {k: v for k, v in old_state.items() if k in own and own[k].shape == v.shape}
            self.load_state_dict(keep, strict=False)

    @staticmethod
    def _view(flat, shp, off, cl):
        n = 1
        for s in shp:
            n *= s
        v = flat[off:off + n]
        if len(shp) == 0:
            return v.view(())
        if cl and len(shp) == 4:
            return v.view(shp[0], shp[2], shp[3], shp[1]).permute(0, 3, 1, 2)
        return v.view(*shp)

    @torch.no_grad()
    def _init_weights(self):
        """Seedable random init (no network fetches -- SURVEY.md 8(b) 'Construction'): torch's default
        per-module inits; HF's N(0, 0.02) for the embedding tables; torchvision's kaiming_normal
        fan_out for the backbone convs."""
        shapes = {n: shp for n, _, shp, _, _ in self._table}
        for name, kind, shp, off, cl in self._table:
            t = self._view(self._flat[kind], shp, off, cl)
            if kind == 2:
                t.zero_()
            elif kind == 1:
                t.fill_(1.0 if name.endswith("running_var") else 0.0)
            elif name == _FB + "layer_weight":
                t.fill_(1.0)          # torch.ones(depth + 1)
            elif name in (_FB + "token_emb.weight", _FB + "pos_emb.relative_attention_bias.weight"):
                t.normal_(0.0, 1.0)   # nn.Embedding
            elif name.endswith("embeddings.weight"):
                t.normal_(0.0, 0.02)
                if "word_embeddings" in name:
                    t[0].zero_()  # padding_idx row
            elif len(shp) == 4:
                if ".trans.model." in name:
                    nn.init.kaiming_normal_(t, mode="fan_out", nonlinearity="relu")
                else:
                    nn.init.kaiming_uniform_(t, a=math.sqrt(5))
            elif len(shp) == 2:
                nn.init.kaiming_uniform_(t, a=math.sqrt(5))
            elif name.endswith(".bias") and len(shapes.get(name[:-5] + ".weight", ())) == 2:
                bound = 1.0 / math.sqrt(shapes[name[:-5] + ".weight"][1])
                t.uniform_(-bound, bound)
            elif name.endswith(".weight"):
                t.fill_(1.0)  # LayerNorm / BatchNorm gamma
            else:
                t.zero_()     # LayerNorm / BatchNorm beta

    def _rehead(self, new_linear: nn.Linear):
        """classifier[2] surgery: rebuild the engine with the new class count, keep every other
        weight, take classifier.2.* from the given nn.Linear."""
        old = {k: v.detach().clone() for k, v in self.state_dict().items() if not k.startswith("classifier.2.")}
        dev = self._flat[0].device
        desc = desc_from_args(self._args, self._feat_dim, n_classes=new_linear.out_features)
        self._build(desc, dev, init=True, old_state=old)
        with torch.no_grad():
            self._params_by_name["classifier.2.weight"].copy_(new_linear.weight)
            if new_linear.bias is not None:
                self._params_by_name["classifier.2.bias"].copy_(new_linear.bias)

    # ------------------------------------------------------------------ nn.Module protocol
    def _apply(self, fn, recurse=True):
        """.to()/.cuda()/.cpu(): move the flat buffers and re-point every parameter at its view."""
        probe = fn(torch.zeros(1, dtype=torch.float32, device=self._flat[0].device))
        if probe.dtype != torch.float32:
            raise NotImplementedError("the MMBERT hot path is fp32 (SURVEY.md section 8)")
        for k in (0, 1):
            self._flat[k] = fn(self._flat[k])
        self._flat[2] = self._flat[2].to(self._flat[0].device)
        self._flat_grad = fn(self._flat_grad)
        self._anchor = torch.zeros(1, dtype=torch.float32, device=self._flat[0].device, requires_grad=True)
        self._plan_key = None
        self._ws = None
        for name, kind, shp, off, cl in self._table:
            view = self._view(self._flat[kind], shp, off, cl)
            parts = name.split(".")
            mod = self
            for p in parts[:-1]:
                mod = mod._modules[p]
            if kind == 0:
                prm = mod._parameters[parts[-1]]
                had_grad = prm.grad is not None
                prm.data = view
                prm.grad = self._view(self._flat_grad, shp, off, cl) if had_grad else None
            else:
                mod._buffers[parts[-1]] = view
        return self

    def load_state_dict(self, state_dict, strict=True, **kw):
        """The Feedback Transformer's shared to_kv weight arrives under n_layers + 1 names; the aliases of a real
        checkpoint are equal, so all of them take the tensor of layers.0 when it is there."""
        if self._desc.encoder == L.ENC_FEEDBACK and _FB_KV in state_dict:
            state_dict = dict(state_dict)
            for name in _fb_kv_aliases(self._desc.n_layers):
                if name in state_dict:
                    state_dict[name] = state_dict[_FB_KV]
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def __del__(self):
        try:
            if self._handle is not None:
                L.lib().mmvqa_engine_destroy(self._handle)
        except Exception:
            pass

    # ------------------------------------------------------------------ flat views for the fused optimizer / DDP
    @property
    def flat_params(self):
        return self._flat[0]

    @property
    def flat_grads(self):
        return self._flat_grad

    def attach_grads(self):
        """make the .grad of every used parameter that requires a gradient a view of the flat gradient buffer"""
        for name, kind, shp, off, cl in self._table:
            if kind == 0 and not name.startswith(_NEVER_USED):
                p = self._params_by_name[name]
                if p.grad is None and p.requires_grad:
                    p.grad = self._view(self._flat_grad, shp, off, cl)

    # ------------------------------------------------------------------ frozen parameters
    def _frozen_state(self):
        """(engine flags, merged [lo, hi) ranges of the flat buffers whose parameters have requires_grad=False), read
        from the parameters now; _NOT_FROZEN when every parameter requires a gradient"""
        tab = self._param_ranges()
        if all(map(_REQUIRES_GRAD, self._ranges[2])):
            return _NOT_FROZEN
        ranges, backbone = [], True
        for name, p, lo, hi in tab:
            if p.requires_grad:
                backbone = backbone and not name.startswith(_BACKBONE)
            elif ranges and ranges[-1][1] == lo:
                ranges[-1][1] = hi
            else:
                ranges.append([lo, hi])
        flags = 0
        if backbone:
            flags = L.FREEZE_BACKBONE | (L.FREEZE_BN_STATS if self._bn_stats_running else 0)
        return flags, tuple((lo, hi) for lo, hi in ranges)

    def _param_ranges(self):
        """[(name, parameter, lo, hi)] in buffer order; [lo, hi) runs to the next tensor (each starts on a multiple of 4
        floats), so the ranges partition the flat parameter buffer"""
        tab = getattr(self, "_ranges", None)
        if tab is None or tab[0] is not self._table:
            prm = sorted((off, name) for name, kind, _, off, _ in self._table if kind == 0)
            ends = [o for o, _ in prm[1:]] + [self._flat[0].numel()]
            rows = [(name, self._params_by_name[name], off, hi) for (off, name), hi in zip(prm, ends)]
            tab = self._ranges = (self._table, rows, tuple(r[1] for r in rows))
        return tab[1]

    def freeze_backbone(self, bn_stats="batch"):
        """The reference's commented-out freeze (models/image_encoding.py:50-51): requires_grad_(False) on every
        parameter of the CNN body, transformer.trans.model.* (the five tap convolutions keep training).  Their .grad
        becomes None, and training forwards skip the backbone's backward pass.  bn_stats="batch": BatchNorm keeps
        normalising with batch statistics and updating the running ones, which is what torch does with frozen
        parameters under .train().  bn_stats="running": the backbone's BatchNorms use their running statistics and leave
        them alone (the backbone.eval() half of the usual freeze); dropout and the rest of the model stay in training
        mode."""
        if bn_stats not in ("batch", "running"):
            raise ValueError(f"freeze_backbone: bn_stats={bn_stats!r} is neither 'batch' nor 'running'")
        for name, p in self._params_by_name.items():
            if name.startswith(_BACKBONE):
                p.requires_grad_(False)
                p.grad = None
        self._bn_stats_running = bn_stats == "running"
        return self

    def unfreeze_backbone(self):
        for name, p in self._params_by_name.items():
            if name.startswith(_BACKBONE):
                p.requires_grad_(True)
        self._bn_stats_running = False
        return self

    def freeze_visual(self):
        """freeze_backbone(bn_stats="running") extended to the five tap convolutions: requires_grad_(False) on every
        parameter under transformer.trans., the state in which an image's visual tokens depend on the image alone
        (tokens.TokenCache).  The taps cannot train from cached tokens: their activation sits between the 1x1
        convolution and the pooling, so the token is not a function of anything a cache could hold short of the whole
        feature map."""
        for name, p in self._params_by_name.items():
            if name.startswith("transformer.trans."):
                p.requires_grad_(False)
                p.grad = None
        self._bn_stats_running = True
        return self

    def unfreeze_visual(self):
        """undoes freeze_visual (and freeze_backbone): every parameter under transformer.trans. requires a gradient again
        and the backbone's BatchNorms are back on batch statistics.  unfreeze_backbone alone leaves the taps frozen."""
        for name, p in self._params_by_name.items():
            if name.startswith("transformer.trans."):
                p.requires_grad_(True)
        self._bn_stats_running = False
        return self

    # ------------------------------------------------------------------ engine calls
    def _ensure_plan(self, B, T, IH, IW, NI=None):
        """NI: the images of a grouped batch (forward_grouped); None: the ungrouped plan, one image per row"""
        key = (B, T, IH, IW, NI)
        lib = L.lib()
        if self._plan_key != key:
            if NI is None:
                nbytes = lib.mmvqa_engine_plan(self._handle, B, T, IH, IW)
            else:
                nbytes = lib.mmvqa_engine_plan_grouped(self._handle, NI, B, T, IH, IW)
            if nbytes == 0:
                L.check(-1)
            if self._ws is None or self._ws.numel() < nbytes:
                self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self._flat[0].device)
            L.check(lib.mmvqa_engine_bind(self._handle, L.ptr(self._flat[0]), L.ptr(self._flat_grad),
                                          L.ptr(self._flat[1]), L.ptr(self._flat[2]), L.ptr(self._ws),
                                          self._ws.numel()))
            self._plan_key = key

    def set_seed(self, seed: int):
        """dropout stream for training-mode forwards (counter-based RNG in the kernels)"""
        self._seed_ctr = int(seed) & 0x7FFFFFFF

    def _plan_is_grouped(self):
        return self._plan_key is not None and self._plan_key[4] is not None

    def _engine_forward(self, img, ids, seg, mask, prec=0, frozen_flags=0, maps=None):
        """maps: None, or the device int32 group | offsets of a grouped batch (img then holds its NI images)"""
        d = self._desc
        if d.encoder == L.ENC_FEEDBACK and not 2 <= ids.shape[1] <= L.FB_MAX_T:
            raise ValueError(f"the feedback-transformer takes 2 <= T <= {L.FB_MAX_T} tokens, not T={ids.shape[1]}: one token "
                             f"has no keys to attend to, and beyond {L.FB_MAX_T} the reference truncates its memory (not built)")
        if not img.is_cuda:
            raise L.MMVQAError("mm-vqa_amd runs on the GPU only: move the model and inputs to 'cuda' "
                               "(there is no CPU fallback by design)")
        img = img.contiguous().float()
        ids, seg, mask = (t.contiguous().long() for t in (ids, seg, mask))
        B, T = ids.shape
        NI = None if maps is None else img.shape[0]
        self._ensure_plan(B, T, img.shape[2], img.shape[3], NI)
        rows = B if d.head_kind == L.HEAD_VQA else B * T
        V = d.hidden if d.head_kind == L.HEAD_NONE else d.n_classes   # headless: the buffer receives h
        ld = (V + 3) & ~3
        # (pad columns V..ld-1 are never read: the loss kernels mask them and the engine's GEMMs contract over V)
        buf = torch.empty(rows, ld, dtype=torch.float32, device=img.device)
        if ld != V:
            buf[:, V:].zero_()
        feat = torch.empty(B, d.feat_dim, dtype=torch.float32, device=img.device) if d.supcon else None
        self._seed_ctr = (self._seed_ctr * 1103515245 + 12345) & 0x7FFFFFFF
        L.check(L.lib().mmvqa_engine_set_precision(self._handle, int(prec)))
        L.check(L.lib().mmvqa_engine_set_frozen(self._handle, int(frozen_flags)))   # recorded by the forward for its backward
        if maps is None:
            L.check(L.lib().mmvqa_engine_forward(self._handle, L.stream_ptr(), L.ptr(img), L.ptr(ids), L.ptr(seg),
                                                 L.ptr(mask), L.ptr(buf), ld, L.ptr(feat), 1 if self.training else 0,
                                                 self._seed_ctr))
        else:
            L.check(L.lib().mmvqa_engine_forward_grouped(self._handle, L.stream_ptr(), L.ptr(img), L.ptr(maps),
                                                         C.c_void_p(maps.data_ptr() + 4 * B), L.ptr(ids), L.ptr(seg),
                                                         L.ptr(mask), L.ptr(buf), ld, L.ptr(feat),
                                                         1 if self.training else 0, self._seed_ctr))
        self._fwd_state = (img, ids, seg, mask, rows, V, ld)
        logits = buf[:, :V]
        logits = logits.view(B, T, V) if d.head_kind != L.HEAD_VQA else logits
        return (logits, feat) if d.supcon else logits

    def _engine_backward(self, dlogits, dfeat=None, prec=0, frozen=_NOT_FROZEN):
        img, ids, seg, mask, rows, V, ld = self._fwd_state
        first = next((p for n, p in self._params_by_name.items() if not n.startswith(_NEVER_USED) and p.requires_grad), None)
        if first is not None and first.grad is None:           # optimizer.zero_grad(set_to_none=True) semantics
            self._flat_grad.zero_()
        g = dlogits.reshape(rows, V) if dlogits.dim() == 3 else dlogits
        if not (g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= ld and g.data_ptr() % 16 == 0):
            pad = torch.zeros(rows, ld, dtype=torch.float32, device=g.device)
            pad[:, :V] = g
            g = pad
        gld = g.stride(0)
        if dfeat is not None:
            dfeat = dfeat.contiguous()
        L.check(L.lib().mmvqa_engine_set_precision(self._handle, int(prec)))   # the mode of this backward's forward
        L.check(L.lib().mmvqa_engine_backward(self._handle, L.stream_ptr(), L.ptr(g), gld, L.ptr(dfeat)))
        if getattr(self, "_cb_error", None) is not None:
            err, self._cb_error = self._cb_error, None
            raise err
        for lo, hi in frozen[1]:         # no gradient for these: whatever the engine computed there is discarded
            self._flat_grad[lo:hi].zero_()
        self.attach_grads()

    def feature_gradient(self, img, input_ids, segment_ids, input_mask, target=None):
        """Attribution pass (vqamed2019/grad_cam2.py:139-145, batched): an eval-mode forward, then the gradient of
        logits[b, target[b]] with respect to the deepest backbone feature map A of sample b (ResNet: layer4's output,
        EfficientNet: the last block's, o[4]).  Returns (logits [B, classes], A, dA, target) with A, dA NHWC
        [B, H, W, C] fp32.  target=None: the predicted class.  Data gradients only: parameters, .grad, BatchNorm buffers
        and self.training are as before; nothing here waits for the device.  fp32 only (NotImplementedError inside
        torch.autocast), VQA head only."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("attribution (feature_gradient / grad_cam) is fp32 in this version: call it outside "
                                      "torch.autocast")
        logits, A = self.feature_map(img, input_ids, segment_ids, input_mask)
        B, V = logits.shape
        ld = self._fwd_state[6]
        if target is None:
            target = logits.argmax(1)
        target = torch.as_tensor(target, device=logits.device).long().reshape(B)
        g = torch.zeros(B, ld, dtype=torch.float32, device=logits.device)
        g.scatter_(1, target.view(B, 1), 1.0)
        dA = torch.empty_like(A)
        L.check(L.lib().mmvqa_engine_backward_feature(self._handle, L.stream_ptr(), L.ptr(g), ld, L.ptr(dA)))
        return logits, A, dA, target

    def feature_map(self, img, input_ids, segment_ids, input_mask):
        """The forward half of feature_gradient: an eval-mode forward under no_grad -> (logits [B, classes], A [B, H, W, C]),
        A a copy of the deepest backbone feature map.  Same refusals, and self.training is restored."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("attribution (feature_gradient / grad_cam) is fp32 in this version: call it outside "
                                      "torch.autocast")
        d = self._desc
        if d.head_kind != 1:
            raise NotImplementedError("feature_gradient needs the VQA head (dataset='VQA-Med'): one row of logits per sample")
        self._refuse_after_grouped("feature_gradient / feature_map")
        lib = L.lib()
        was_training = self.training
        self.train(False)
        try:
            with torch.no_grad():
                logits = self._engine_forward(img, input_ids, segment_ids, input_mask, L.PREC_F32)
        finally:
            self.train(was_training)
        B = logits.shape[0]
        ap, fh, fw, fc = C.c_void_p(), C.c_int(), C.c_int(), C.c_int()
        L.check(lib.mmvqa_engine_feature_map(self._handle, C.byref(ap), C.byref(fh), C.byref(fw), C.byref(fc)))
        H, W, Cc = fh.value, fw.value, fc.value
        off = ap.value - self._ws.data_ptr()
        A = self._ws[off:off + 4 * B * H * W * Cc].view(torch.float32).view(B, H, W, Cc).clone()   # (the next forward overwrites the workspace)
        return logits, A

    def _refuse_after_grouped(self, who):
        """attribution and cached-token forwards are not built for grouped batches: directly after forward_grouped the
        engine's plan, its tokens and its feature maps are those of NI images for B rows, which these entries would
        silently re-plan away.  A plain forward() in between (which re-plans) makes them valid again."""
        if self._plan_is_grouped():
            raise L.MMVQAError(f"{who}: the last step was a grouped one (forward_grouped); attribution and cached visual "
                               "tokens are not built for grouped batches -- run forward() first")

    def deepest_tap(self):
        """-> (weight [hidden, C] of the 1x1 tap that the deepest feature map feeds, the visual-token row it fills, its
        activation): conv2 / row 0 for the ResNets, conv7 / row 4 for EfficientNet (engine.cpp, feature_tap)"""
        name, k = ("conv7", 4) if self._desc.cnn == 1 else ("conv2", 0)
        w = self._params_by_name[f"transformer.trans.{name}.weight"]
        return w.detach().reshape(w.shape[0], -1).contiguous(), k, (L.ACT_RELU if self._desc.use_relu else L.ACT_SERF)

    def visual_tokens(self, img):
        """The num_vis visual tokens of `img` [B, 3, H, W] -> [B, num_vis, hidden] fp32: the eval-mode backbone and its
        taps under no_grad (self.training and the dropout stream's counter are restored).  Implemented as one whole eval
        forward with a dummy text that fills two positions after the num_vis visual rows, whose output is discarded: the engine has no backbone-only entry, and the backbone is at least 80 % of a
        forward.  fp32 only (NotImplementedError inside torch.autocast)."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("visual tokens (visual_tokens / forward_tokens) are fp32 in this version: call it "
                                      "outside torch.autocast")
        self._run_backbone_eval(img)
        return self._read_visual_tokens(img.shape[0])

    def _run_backbone_eval(self, img):
        """visual_tokens' forward: afterwards the tokens of `img` are in the workspace (mmvqa_engine_visual_tokens)"""
        B = img.shape[0]
        T = self._desc.num_vis + 2
        ids = torch.zeros(B, T, dtype=torch.long, device=img.device)
        ones = torch.ones(B, T, dtype=torch.long, device=img.device)
        was_training, seed_ctr = self.training, self._seed_ctr
        self.train(False)
        try:
            with torch.no_grad():
                self._engine_forward(img, ids, ids, ones, L.PREC_F32)
        finally:
            self.train(was_training)
            self._seed_ctr = seed_ctr                                        # an eval forward draws nothing: later training steps see the same stream

    def _read_visual_tokens(self, B):
        """the tokens the last forward left in the workspace, copied out as [B, num_vis, hidden]"""
        d = self._desc
        vp = C.c_void_p()
        L.check(L.lib().mmvqa_engine_visual_tokens(self._handle, C.byref(vp)))
        off = vp.value - self._ws.data_ptr()
        vis = self._ws[off:off + 4 * d.num_vis * B * d.hidden].view(torch.float32).view(d.num_vis, B, d.hidden)
        return vis.permute(1, 0, 2).contiguous()

    def forward_tokens(self, vis, input_ids, segment_ids, input_mask):
        """The encoder and the heads from given visual tokens, without the backbone: vis [B, num_vis, hidden] (what
        visual_tokens returns; rows may repeat one image's tokens for several questions, whatever batch size they were
        computed at) -> the same tuple as forward.  Always eval mode and no_grad; self.training, parameters, .grad and
        BatchNorm buffers are as before.  No backward of any kind is valid after it (the engine refuses).  fp32 only
        (NotImplementedError inside torch.autocast)."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("visual tokens (visual_tokens / forward_tokens) are fp32 in this version: call it "
                                      "outside torch.autocast")
        d = self._desc
        self._refuse_after_grouped("forward_tokens")
        if not vis.is_cuda:
            raise L.MMVQAError("mm-vqa_amd runs on the GPU only: move the model and inputs to 'cuda' "
                               "(there is no CPU fallback by design)")
        ids, seg, mask = (t.contiguous().long() for t in (input_ids, segment_ids, input_mask))
        B, T = ids.shape
        if tuple(vis.shape) != (B, d.num_vis, d.hidden):
            raise ValueError(f"vis must be [B={B}, {d.num_vis}, {d.hidden}], not {tuple(vis.shape)}")
        if d.encoder == L.ENC_FEEDBACK and not 2 <= T <= L.FB_MAX_T:
            raise ValueError(f"the feedback-transformer takes 2 <= T <= {L.FB_MAX_T} tokens, not T={T}")
        vis_e = vis.detach().float().permute(1, 0, 2).contiguous()            # the engine's [num_vis][B][hidden]
        # the backbone is not run, but the workspace is laid out for an image size: a small one, so that hundreds of
        # token rows (Ablation-CAM's variants) do not reserve the backbone's activations at 224 x 224
        self._ensure_plan(B, T, _TOKEN_PLAN_HW, _TOKEN_PLAN_HW)
        rows = B if d.head_kind == L.HEAD_VQA else B * T
        V = d.hidden if d.head_kind == L.HEAD_NONE else d.n_classes
        ld = (V + 3) & ~3
        buf = torch.empty(rows, ld, dtype=torch.float32, device=vis.device)
        if ld != V:
            buf[:, V:].zero_()
        feat = torch.empty(B, d.feat_dim, dtype=torch.float32, device=vis.device) if d.supcon else None
        L.check(L.lib().mmvqa_engine_set_precision(self._handle, L.PREC_F32))
        L.check(L.lib().mmvqa_engine_forward_tokens(self._handle, L.stream_ptr(), L.ptr(vis_e), L.ptr(ids), L.ptr(seg),
                                                    L.ptr(mask), L.ptr(buf), ld, L.ptr(feat)))
        logits = buf[:, :V]
        logits = logits.view(B, T, V) if d.head_kind != L.HEAD_VQA else logits
        out = (logits, feat) if d.supcon else logits
        if self.dataset == "VQA-Med":
            return out, 0, 0
        return out

    # ------------------------------------------------------------------ training from cached visual tokens
    def token_range(self):
        """[lo, hi) of the flat parameter / gradient buffers that holds transformer.trans.*: the CNN body and the five tap
        convolutions, everything in front of the visual tokens (the engine's [emb_hi, enc_lo))"""
        rows = [(lo, hi) for name, _, lo, hi in self._param_ranges() if name.startswith("transformer.trans.")]
        lo, hi = min(r[0] for r in rows), max(r[1] for r in rows)
        assert sum(h - l for l, h in rows) == hi - lo, "transformer.trans.* is one contiguous range of the engine's layout"
        return lo, hi

    def forward_cached(self, cache, index, view, input_ids, segment_ids, input_mask):
        """forward for a batch whose visual tokens come from a tokens.TokenCache instead of the backbone: row b reads
        cache.tokens[index[b], view[b]].  Returns the same tuple as forward, honours self.training (dropout with the
        probabilities and the stream of forward: the same seed gives the same masks) and advances the dropout counter
        as forward does.  With grad enabled, backward reaches the heads, the encoder and the embeddings; parameters
        under transformer.trans. (backbone and taps) receive nothing: their .grad and their range of flat_grads are
        untouched, and no BatchNorm buffer is written.  Every other parameter behaves as under forward.

        index / view are HOST integer tensors or sequences of length B, validated before anything is launched
        (ValueError names the offending position) and uploaded from pinned memory without waiting for the device.
        fp32 only (NotImplementedError inside torch.autocast)."""
        if torch.is_autocast_enabled("cuda"):
            raise NotImplementedError("visual tokens (visual_tokens / forward_tokens) are fp32 in this version: call it "
                                      "outside torch.autocast")
        d = self._desc
        ids = input_ids
        if ids.dim() != 2:
            raise ValueError(f"forward_cached takes input_ids [B, T], not {tuple(ids.shape)}")
        tokens = cache.tokens
        if tuple(tokens.shape[2:]) != (d.num_vis, d.hidden):
            raise ValueError(f"the cache holds tokens of [{tokens.shape[2]}, {tokens.shape[3]}], the model's are "
                             f"[{d.num_vis}, {d.hidden}]")
        maps = cached_maps(index, view, tokens.shape[0], tokens.shape[1], ids.shape[0])
        self._refuse_after_grouped("forward_cached")
        if not (tokens.is_cuda and ids.is_cuda):
            raise L.MMVQAError("mm-vqa_amd runs on the GPU only: move the model and inputs to 'cuda' "
                               "(there is no CPU fallback by design)")
        pinned = torch.empty(maps.numel(), dtype=torch.int32, pin_memory=True)   # (the caching host allocator: no
        pinned.copy_(maps)                                                       # allocation after the first steps)
        maps = pinned.to(tokens.device, non_blocking=True)                       # index and view go up in one copy
        frozen = self._frozen_state() if torch.is_grad_enabled() else _NOT_FROZEN
        out = _CachedModelFn.apply(self, self._anchor, tokens, maps, input_ids, segment_ids, input_mask, frozen)
        if self.dataset == "VQA-Med":
            return out, 0, 0
        return out

    def _engine_forward_cached(self, tokens, maps, ids, seg, mask):
        d = self._desc
        ids, seg, mask = (t.contiguous().long() for t in (ids, seg, mask))
        B, T = ids.shape
        if d.encoder == L.ENC_FEEDBACK and not 2 <= T <= L.FB_MAX_T:
            raise ValueError(f"the feedback-transformer takes 2 <= T <= {L.FB_MAX_T} tokens, not T={T}")
        self._ensure_plan(B, T, _TOKEN_PLAN_HW, _TOKEN_PLAN_HW)    # the backbone is not run: forward_tokens' layout
        rows = B if d.head_kind == L.HEAD_VQA else B * T
        V = d.hidden if d.head_kind == L.HEAD_NONE else d.n_classes
        ld = (V + 3) & ~3
        buf = torch.empty(rows, ld, dtype=torch.float32, device=ids.device)
        if ld != V:
            buf[:, V:].zero_()
        feat = torch.empty(B, d.feat_dim, dtype=torch.float32, device=ids.device) if d.supcon else None
        self._seed_ctr = (self._seed_ctr * 1103515245 + 12345) & 0x7FFFFFFF
        N, K = tokens.shape[0], tokens.shape[1]
        L.check(L.lib().mmvqa_engine_set_precision(self._handle, L.PREC_F32))
        L.check(L.lib().mmvqa_engine_forward_cached(self._handle, L.stream_ptr(), L.ptr(tokens), N, K, L.ptr(maps),
                                                    C.c_void_p(maps.data_ptr() + 4 * B), L.ptr(ids), L.ptr(seg),
                                                    L.ptr(mask), L.ptr(buf), ld, L.ptr(feat), 1 if self.training else 0,
                                                    self._seed_ctr))
        self._fwd_state = (None, ids, seg, mask, rows, V, ld)
        logits = buf[:, :V]
        logits = logits.view(B, T, V) if d.head_kind != L.HEAD_VQA else logits
        return (logits, feat) if d.supcon else logits

    def _engine_backward_cached(self, dlogits, dfeat=None, frozen=_NOT_FROZEN):
        _, ids, seg, mask, rows, V, ld = self._fwd_state
        t_lo, t_hi = self.token_range()
        live = [(n, p) for n, p in self._params_by_name.items()
                if not n.startswith(_NEVER_USED) and not n.startswith("transformer.trans.") and p.requires_grad]
        if live and live[0][1].grad is None:                    # zero_grad(set_to_none=True): everything this backward adds to
            self._flat_grad[:t_lo].zero_()
            self._flat_grad[t_hi:].zero_()
        g = dlogits.reshape(rows, V) if dlogits.dim() == 3 else dlogits
        if not (g.stride(1) == 1 and g.stride(0) % 4 == 0 and g.stride(0) >= ld and g.data_ptr() % 16 == 0):
            pad = torch.zeros(rows, ld, dtype=torch.float32, device=g.device)
            pad[:, :V] = g
            g = pad
        if dfeat is not None:
            dfeat = dfeat.contiguous()
        L.check(L.lib().mmvqa_engine_set_precision(self._handle, L.PREC_F32))
        L.check(L.lib().mmvqa_engine_backward_cached(self._handle, L.stream_ptr(), L.ptr(g), g.stride(0), L.ptr(dfeat)))
        if getattr(self, "_cb_error", None) is not None:
            err, self._cb_error = self._cb_error, None
            raise err
        for lo, hi in frozen[1]:         # frozen outside transformer.trans.: computed, then discarded, as under forward
            if lo < t_lo:
                self._flat_grad[lo:min(hi, t_lo)].zero_()
            if hi > t_hi:
                self._flat_grad[max(lo, t_hi):hi].zero_()
        shapes = {name: (shp, off, cl) for name, kind, shp, off, cl in self._table if kind == 0}
        for name, p in live:
            if p.grad is None:
                p.grad = self._view(self._flat_grad, *shapes[name])

    def forward(self, img, input_ids, segment_ids, input_mask):
        """Inside torch.autocast("cuda", dtype=torch.float16) the forward and its backward run in the mixed-precision
        mode: both operands of every contraction of the implicit GEMM (every ResNet convolution with the stem,
        the downsample branches and the five tap 1x1 convolutions; every nn.Linear of the encoder and the heads;
        forward, data gradient and weight gradient) are rounded to fp16 nearest-even (bit-equal to .half()) and
        accumulated in fp32.  Everything else stays fp32: activations, gradients and parameters in storage,
        BatchNorm statistics, epilogues, LayerNorm, softmax, attention's QK^T and PV products, embeddings, losses
        and the returned logits.  This rounds strictly less than torch's autocast, which also rounds each
        conv / linear output to fp16 and runs BatchNorm and elementwise ops on fp16 tensors: results are close
        to, not bit-equal to, the reference under autocast.  Other autocast dtypes (bf16) and EfficientNet
        under fp16 autocast raise NotImplementedError.  Outside autocast everything is fp32 as before.

        requires_grad is honoured per parameter, read at each forward that runs with grad enabled: a parameter with
        requires_grad=False gets no .grad and its range of flat_grads is zero after backward.  When every parameter of
        the CNN body (transformer.trans.model.*) is frozen, its backward pass is not run at all (freeze_backbone()); the
        gradient of any other frozen tensor is still computed and then discarded.  With a gradient-ready hook, such a
        discarded range is announced as computed and zeroed when backward ends."""
        prec = autocast_precision(self._desc)
        frozen = self._frozen_state() if torch.is_grad_enabled() else _NOT_FROZEN
        out = _ModelFn.apply(self, self._anchor, img, input_ids, segment_ids, input_mask, prec, frozen)
        if self.dataset == "VQA-Med":
            return out, 0, 0   # models/mmbert.py:167
        return out

    def forward_grouped(self, img, group, input_ids, segment_ids, input_mask):
        """forward for a batch in which several text rows ask about one image (VQA-Med: four questions per image):
        img [NI, 3, H, W] holds each image once, input_ids / segment_ids / input_mask are [B, T] with B >= NI, and
        group[b] in [0, NI) names the image of row b.  The model is the reference's with one change: the visual-token
        rows of sample b are those of image group[b].  The backbone and its taps run once on the NI images, forward and
        backward; the gradient of an image's tokens is the sum over its rows.  Train-mode BatchNorm therefore sees each
        image once.  Same return contract, autocast, requires_grad and frozen-backbone handling
        as forward.

        group is a HOST integer tensor or sequence of length B (what data.collate_grouped produces), non-decreasing from
        0 to NI - 1 in steps of at most 1; it is validated before anything is launched (ValueError), nothing is read back
        from the device."""
        ids = input_ids
        if ids.dim() != 2 or img.dim() != 4:
            raise ValueError(f"forward_grouped takes img [NI, 3, H, W] and input_ids [B, T], not {tuple(img.shape)} and "
                             f"{tuple(ids.shape)}")
        maps = group_maps(group, img.shape[0], ids.shape[0])
        if not img.is_cuda:
            raise L.MMVQAError("mm-vqa_amd runs on the GPU only: move the model and inputs to 'cuda' "
                               "(there is no CPU fallback by design)")
        prec = autocast_precision(self._desc)
        frozen = self._frozen_state() if torch.is_grad_enabled() else _NOT_FROZEN
        maps = maps.to(img.device, non_blocking=True)                        # group and offsets go up in one copy
        out = _GroupedModelFn.apply(self, self._anchor, img, maps, input_ids, segment_ids, input_mask, prec, frozen)
        if self.dataset == "VQA-Med":
            return out, 0, 0
        return out

    # ------------------------------------------------------------------ data-parallel overlap
    def set_grad_ready_hook(self, fn, with_event=False):
        """fn(lo, hi) is called during backward as soon as flat_grads[lo:hi] is final (ordered on the current
        stream), in an order that partitions the whole buffer; pass None to remove.  Used by ddp.GradReducer to
        start the RCCL all-reduce of finished ranges while the backbone backward is still running.
        with_event=True: fn(lo, hi, ready) also receives a torch.cuda.Event recorded on the engine's stream at the
        announcement, i.e. after that stream has been ordered behind the side stream's weight gradients of the range
        (csrc/engine.cpp notify()): any other stream that waits on it may read the range."""
        self._cb_error = None
        if fn is None:
            self._cb = None
            L.check(L.lib().mmvqa_engine_set_grad_callback(self._handle, None, None))
            return

        def tramp(_user, lo, hi):
            try:
                if with_event:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream())   # the stream backward was given: already behind the join
                    fn(int(lo), int(hi), ev)
                else:
                    fn(int(lo), int(hi))
            except BaseException as ex:   # exceptions cannot cross the C frame
                self._cb_error = ex

        self._cb = C.CFUNCTYPE(None, C.c_void_p, C.c_longlong, C.c_longlong)(tramp)
        L.check(L.lib().mmvqa_engine_set_grad_callback(self._handle, C.cast(self._cb, C.c_void_p), None))

    # ------------------------------------------------------------------ per-shape kernel tuning
    def tune(self, img, input_ids, segment_ids, input_mask):
        """Time the candidate tile / split-K configurations of every GEMM shape of one training step
        (forward + backward on the given batch) and keep the fastest.  Parameters, BatchNorm buffers
        and gradients are left untouched (the pass itself computes garbage)."""
        lib = L.lib()
        bufs, nbt = self._flat[1].clone(), self._flat[2].clone()
        was_training = self.training
        self.train()
        L.check(min(0, lib.mmvqa_engine_tune(self._handle, 1)))
        cb = getattr(self, "_cb", None)
        if cb is not None:   # the throw-away pass must not trigger gradient all-reduces
            L.check(lib.mmvqa_engine_set_grad_callback(self._handle, None, None))
        prec = autocast_precision(self._desc)   # under fp16 autocast the f16-operand shapes are tuned
        try:
            out = self._engine_forward(img, input_ids, segment_ids, input_mask, prec)
            logits = out[0] if isinstance(out, tuple) else out
            feat = out[1] if isinstance(out, tuple) else None
            self._engine_backward(torch.zeros_like(logits), None if feat is None else torch.zeros_like(feat), prec=prec)
            torch.cuda.synchronize()
        finally:
            n = lib.mmvqa_engine_tune(self._handle, 0)
            if cb is not None:
                L.check(lib.mmvqa_engine_set_grad_callback(self._handle, C.cast(cb, C.c_void_p), None))
            self._flat[1].copy_(bufs)
            self._flat[2].copy_(nbt)
            self._flat_grad.zero_()
            self.train(was_training)
        return n

    # ------------------------------------------------------------------ profiling (bench.py)
    def profile(self, enable, serialized: bool = False):
        """per-launch HIP-event timing of the next step; serialized=True puts every launch on one stream"""
        L.check(L.lib().mmvqa_engine_profile(self._handle, (2 if serialized else 1) if enable else 0))

    REGIONS = ("backbone", "tap", "qkv", "attention", "encoder_rest", "heads", "embed", "bn_coef", "qkv_attention_fused")
    # igemm_kernel | attention kernels | launches without matrix work | matrix work outside igemm_kernel (tapthin.hip, se.hip)
    PROFILE_CLASSES = ("igemm", "attention", "other", "matrix_other")

    def profile_read_regions(self):
        """{region: {class: {launches, ms, flops}}} of the profiled step (mmvqa_engine_profile_read_region)"""
        out = {}
        for r, rn in enumerate(self.REGIONS):
            out[rn] = {}
            for cls, nm in enumerate(self.PROFILE_CLASSES):
                n, ms, fl = C.c_longlong(), C.c_double(), C.c_double()
                L.check(L.lib().mmvqa_engine_profile_read_region(self._handle, r, cls, C.byref(n), C.byref(ms),
                                                                 C.byref(fl)))
                out[rn][nm] = dict(launches=n.value, ms=ms.value, flops=fl.value)
        return out

    HBM_KERNELS = ("bn_add_relu", "maxpool_fwd", "maxpool_bwd", "layernorm_fwd", "layernorm_bwd", "dropout_copy", "bn_act_add",
                   "dwconv_fwd", "dwconv_bwd_data", "dwconv_bwd_weight", "se_pool", "se_dgate", "act_bwd_stats",
                   "tap_thin_fwd", "tap_thin_bwd",
                   "fb_weight_gradients")   # (not a kernel: the feedback encoder's weight-gradient block after its time loop)

    def profile_read_hbm(self):
        """{kernel: {launches, ms, bytes}} of the HBM-bound kernels of the profiled step (mmvqa_engine_profile_read_hbm)"""
        out = {}
        for k, nm in enumerate(self.HBM_KERNELS, start=1):
            n, ms, by = C.c_longlong(), C.c_double(), C.c_double()
            L.check(L.lib().mmvqa_engine_profile_read_hbm(self._handle, k, C.byref(n), C.byref(ms), C.byref(by)))
            if n.value:
                out[nm] = dict(launches=n.value, ms=ms.value, bytes=by.value)
        return out

    def profile_read(self):
        out = {}
        for cls, nm in enumerate(self.PROFILE_CLASSES):
            n, ms, fl = C.c_longlong(), C.c_double(), C.c_double()
            L.check(L.lib().mmvqa_engine_profile_read(self._handle, cls, C.byref(n), C.byref(ms), C.byref(fl)))
            out[nm] = dict(launches=n.value, ms=ms.value, flops=fl.value)
        return out
