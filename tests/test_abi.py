"""CPU checks of the drop-in boundary: the shared library loads, exports every symbol that
include/mmvqa.h declares, and the ctypes mirror agrees with the header (argument counts, struct sizes).
No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_functions():
    src = open(os.path.join(ROOT, "include", "mmvqa.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = src[src.index("typedef struct mmvqa_engine mmvqa_engine;"):]
    out = {}
    for m in re.finditer(r"\b([A-Za-z_][\w\s\*]*?)\b(mmvqa_\w+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = m.group(3).strip()
        n = 0 if args in ("", "void") else len([a for a in args.split(",") if a.strip()])
        out[m.group(2)] = n
    return out


def test_library_exports_every_declared_symbol():
    from mmvqa_amd import _lib as L
    lib = L.lib()   # raises if a declared symbol is missing (getattr on the CDLL)
    decl = header_functions()
    assert len(decl) >= 40
    for name, nargs in decl.items():
        assert hasattr(lib, name), f"{name} declared in include/mmvqa.h but not exported"
        assert name in L.SIGNATURES, f"{name} has no ctypes signature"
        assert len(L.SIGNATURES[name][1]) == nargs, f"{name}: header has {nargs} args, ctypes {len(L.SIGNATURES[name][1])}"
    assert set(L.SIGNATURES) == set(decl)
    assert lib.mmvqa_version() >= 100
    assert lib.mmvqa_sizeof_gemm_desc() == C.sizeof(L.GemmDesc)
    assert lib.mmvqa_sizeof_attn_desc() == C.sizeof(L.AttnDesc)
    assert lib.mmvqa_sizeof_model_desc() == C.sizeof(L.ModelDesc)


def test_error_reporting_without_gpu():
    from mmvqa_amd import _lib as L
    lib = L.lib()
    d = L.ModelDesc()   # all zeros: invalid
    h = C.c_void_p()
    rc = lib.mmvqa_engine_create(C.byref(d), C.byref(h))
    assert rc != 0 and b"engine_create" in lib.mmvqa_last_error()
    with pytest.raises(L.MMVQAError):
        L.check(rc)


def test_igemm_refuses_inconsistent_descriptors():
    """misuse returns MMVQA_ERR_ARG on the host instead of reading outside the caller's buffers on the device
    (the loaders address operands from the descriptor's dimensions alone)"""
    from mmvqa_amd import _lib as L
    lib = L.lib()

    def desc():
        d = L.GemmDesc()
        d.M, d.N, d.K = 64, 64, 64
        d.A, d.B, d.C = 0x1000, 0x2000, 0x3000          # never dereferenced: every case below is refused first
        d.a_ld, d.b_ld, d.c_ld, d.g_Cs = 64, 64, 64, 64
        d.g_SH = d.g_SW = d.g_OH = d.g_OW = 1
        d.g_KH = d.g_KW = 1
        d.g_stride, d.g_pad = 1, 0
        return d

    def refused(d, kind, what):
        rc = lib.mmvqa_igemm(C.byref(d), kind, 0, 0, None)
        assert rc == -1, f"{what}: rc {rc}"
        assert b"igemm:" in lib.mmvqa_last_error(), what

    d = desc(); d.K = 96                       # K != taps * Cs
    refused(d, L.KIND_FWD, "K mismatch")
    d = desc(); d.a_ld = 32                    # rows shorter than the contraction
    refused(d, L.KIND_FWD, "a_ld")
    d = desc(); d.b_ld = 8
    refused(d, L.KIND_FWD, "b_ld")
    d = desc(); d.A = None
    refused(d, L.KIND_FWD, "null A")
    d = desc(); d.a_pro = L.PRO_DZ             # BatchNorm-backward prologue without its second tensor / coefficients
    refused(d, L.KIND_DGRAD, "PRO_DZ without A2")
    d = desc(); d.g_KH = d.g_KW = 3; d.g_pad = 1; d.g_SH = d.g_SW = d.g_OH = d.g_OW = 8; d.M = 100   # M not whole images
    d.K = 9 * 64; d.b_ld = 9 * 64
    refused(d, L.KIND_FWD, "M not a multiple of OH*OW")
    d = desc(); d.N = 100                      # wgrad: N != taps * Cs
    refused(d, L.KIND_WGRAD, "wgrad N")
    d = desc(); d.dact = L.ACT_GELU            # act' epilogue without the saved pre-activation
    refused(d, L.KIND_DGRAD, "dact without Pre")
    d = desc(); d.drop_p = 1.5
    refused(d, L.KIND_FWD, "dropout p")
    d = desc(); d.reserved1 = 256              # the slot that selected the removed persistent form
    refused(d, L.KIND_FWD, "non-zero reserved1")
    assert b"persistent form was removed" in lib.mmvqa_last_error()
    refused(desc(), 7, "unknown kind")


def test_supcon_refuses_bad_arguments_on_the_host():
    """both SupCon entry points share one launcher and one set of argument checks: each case returns MMVQA_ERR_ARG and
    names the offending argument before any HIP call"""
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000                                 # never dereferenced: every case below is refused first
    # (f, loss, df, ws, N, D) -> what the message must name
    cases = (((None, p, p, p, 4, 8), b"f is null"), ((p, None, p, p, 4, 8), b"loss is null"),
             ((p, p, p, None, 4, 8), b"ws is null"), ((p, p, p, p, 0, 8), b"N=0"), ((p, p, p, p, 4, 0), b"D=0"),
             ((p, p, p, p, 4, 257), b"D=257"))
    for (f, loss, df, ws, N, D), what in cases:
        rc = lib.mmvqa_supcon_loss(None, f, loss, df, ws, N, D, 0.07, 0.07, 1.0)
        err = lib.mmvqa_last_error()
        assert rc == -1 and err.startswith(b"supcon: ") and what in err, (what, rc, err)
        rc = lib.mmvqa_supcon_loss_masked(None, f, p, loss, df, ws, N, D, 0.07, 0.07, 1.0)
        err = lib.mmvqa_last_error()
        assert rc == -1 and err.startswith(b"supcon_masked: ") and what in err, (what, rc, err)
    # a null mask is an error of the masked entry point, not a way to the unmasked kernels
    rc = lib.mmvqa_supcon_loss_masked(None, p, None, p, p, p, 4, 8, 0.07, 0.07, 1.0)
    err = lib.mmvqa_last_error()
    assert rc == -1 and err.startswith(b"supcon_masked: ") and b"mask is null" in err, (rc, err)


def test_entry_points_refuse_bad_arguments_on_the_host():
    """every argument check of an op entry point answers an ABI caller the same wherever the check lives: each row is
    refused with MMVQA_ERR_ARG and its message before any HIP call (no GPU here, the pointers are never dereferenced)"""
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p, q = 0x1000, 0x2000

    def gemm(**kw):
        d = L.GemmDesc()
        d.M, d.N, d.K = 64, 64, 64
        d.A, d.B, d.C = 0x1000, 0x2000, 0x3000
        d.a_ld, d.b_ld, d.c_ld, d.g_Cs = 64, 64, 64, 64
        d.g_SH = d.g_SW = d.g_OH = d.g_OW = d.g_KH = d.g_KW = d.g_stride = 1
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    def attn(**kw):
        d = L.AttnDesc()
        d.q = d.k = d.v = d.out = d.mask = d.probs = d.dout = d.dq = d.dk = d.dv = p
        d.row_stride = d.out_row_stride = 96
        d.head_stride = d.out_head_stride = 8
        d.B, d.T, d.heads, d.sqrt_d = 2, 16, 12, 8.0 ** 0.5
        for k, v in kw.items():
            setattr(d, k, v)
        return C.byref(d)

    def fold(bwd):
        f = L.BnFold()
        f.stat, f.slots, f.bwd, f.count, f.gamma, f.beta = p, 1, bwd, 8.0, p, p
        return C.byref(f)

    dw = (p, p, p, p, p, p, 2, 8, 8)            # z1, s1, b1, w, z2, stat, N, H, W  (then C, OH, OW, stride, pad)
    table = (
        ("bn_add_relu", (None, p, p, p, q, None, None, p, 8, 6), b"bn_add_relu: C % 4 != 0"),
        ("maxpool_fwd", (None, p, p, p, p, p, 2, 8, 8, 6, 4, 4), b"maxpool: C % 4 != 0"),
        ("maxpool_bwd", (None, p, p, None, p, p, p, p, p, p, p, 2, 8, 8, 24, 4, 4), b"maxpool_bwd: C/4 must divide 256 (C=24)"),
        ("qkv_attention_fwd", (None, p, p, p, p, p, p, p, 0, 16, 768, 12, 0.0, 1), b"qkv_attention_fwd: B=0 drop_p=0"),
        ("qkv_attention_fwd", (None, p, p, p, p, p, p, p, 2, 16, 768, 12, 1.0, 1), b"qkv_attention_fwd: B=2 drop_p=1"),
        ("amp_unscale", (None, None, 64, p, p, 1), b"amp_unscale: null pointer"),
        ("amp_unscale", (None, p, 64, None, p, 1), b"amp_unscale: null pointer"),
        ("amp_update_scale", (None, p, p, p, 2.0, 0.5, 0), b"amp_update_scale: growth_interval=0"),
        ("pixmask", (None, None, 2, 4, 4, 8, 8, 3, 3, 2, 1), b"pixmask: null output"),
        ("bn_add_relu_fold", (None, None, fold(0), q, None, p, 8, 64), b"bn_add_relu_fold: null operand"),
        ("attention", (attn(q=None), 8, 0, None), b"attention: null operand"),
        ("attention", (attn(row_stride=6), 8, 0, None), b"attention: strides must be multiples of 4"),
        ("attention", (attn(dq=None), 8, 1, None), b"attention backward: null gradient pointer"),
        ("fb_attention", (None, 0, None), b"fb_attention: null descriptor"),
        ("igemm", (gemm(a_ld=6), L.KIND_FWD, 0, 0, None), b"igemm: a_ld=6 b_ld=64 g_Cs=64 must be multiples of 4"),
        ("igemm", (gemm(N=6), L.KIND_DGRAD, 0, 0, None), b"igemm dgrad: N=6 must be a multiple of 4"),
        ("dwconv_fwd", (None,) + dw + (48, 8, 8, 1, 1), b"dwconv: C=48 must be a multiple of 32"),
        ("dwconv_fwd_fold", (None,) + dw + (32, 8, 8, 1, 1, fold(1)), b"dwconv: the fold must be a forward one"),
        ("se_pool_fold", (None, p, p, p, p, 2, 64, 32, fold(1)), b"se_pool: the fold must be a forward one and C a multiple of 4"),
        ("embed_bwd", (None, p, p, p, p, p, p, p, p, p, p, p, p, 2, 16, 6, 4, 0.0, 1, 0), b"embed: H=6 unsupported"),
    )
    for name, args, what in table:
        rc = getattr(lib, "mmvqa_" + name)(*args)
        err = lib.mmvqa_last_error()
        assert rc == -1 and what in err, (name, what, rc, err)


def test_missing_library_fails_loudly(monkeypatch):
    from mmvqa_amd import _lib as L
    monkeypatch.setattr(L, "_lib", None)
    monkeypatch.setattr(L, "LIB_PATH", "/nonexistent/libmmvqa_hip.so")
    with pytest.raises(L.MMVQAError, match="no CPU fallback"):
        L.lib()


def test_model_protocol_on_cpu():
    """Model(args) builds its parameter table from the engine without a GPU: state_dict names/shapes equal
    the reference's (via the oracle classes, which are pinned to the reference), ResNet-152 has the
    published parameter count, unknown options raise NotImplementedError, forward on CPU refuses."""
    import torch
    import mmvqa_amd
    from oracle import mmbert_oracle as O
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=2, heads=12,
                       vocab_size=50, emb_vocab=50, bert_max_pos=32)
    for tm, ds, sc in (("transformer", "roco", False), ("realformer", "roco", True), ("transformer", "VQA-Med", False)):
        a = O.make_args(**{**vars(args), "transformer_model": tm, "dataset": ds, "supcon": sc})
        m = mmvqa_amd.Model(a)
        o = O.OracleModel(a)
        sd, osd = m.state_dict(), o.state_dict()
        assert set(sd) == set(osd)
        assert all(sd[k].shape == osd[k].shape for k in sd)
        m.load_state_dict(osd)
        assert all(torch.equal(m.state_dict()[k], osd[k]) for k in osd)
    full = mmvqa_amd.Model(O.make_args())
    n_backbone = sum(p.numel() for n, p in full.named_parameters() if n.startswith("transformer.trans.model."))
    assert n_backbone == 60192808                       # torchvision resnet152
    assert sum(p.numel() for p in full.parameters()) == 140_024_674   # = the oracle's (reference-pinned) Model
    # timm tf_efficientnetv2_m(features_only=True): published body size, oracle-identical state_dict
    eff = mmvqa_amd.Model(O.make_args(cnn_encoder="tf_efficientnetv2_m", transformer_model="realformer"))
    n_eff = sum(p.numel() for n, p in eff.named_parameters() if n.startswith("transformer.trans.model."))
    assert n_eff == 52200436
    ea = O.make_args(cnn_encoder="tf_efficientnetv2_m", effnet_depth_div=8, hidden_size=96, n_layers=1, vocab_size=50,
                     emb_vocab=50, bert_max_pos=32)
    esd, eosd = mmvqa_amd.Model(ea).state_dict(), O.OracleModel(ea).state_dict()
    assert set(esd) == set(eosd) and all(esd[k].shape == eosd[k].shape for k in esd)
    with pytest.raises(NotImplementedError):
        mmvqa_amd.Model(O.make_args(transformer_model="lstm"))
    with pytest.raises(NotImplementedError):
        mmvqa_amd.Model(O.make_args(cnn_encoder="vgg16"))
    # mmvqa_engine_tune: 0 / 1 switch the tuning pass, anything else (2 was a query once) is refused and changes nothing
    from mmvqa_amd import _lib as L
    lib = L.lib()
    assert lib.mmvqa_engine_tune(m._handle, 2) == -1 and b"tune:" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_tune(m._handle, 0) == 0
    with pytest.raises(mmvqa_amd.MMVQAError):
        m(torch.zeros(1, 3, 32, 32), torch.zeros(1, 8, dtype=torch.long), torch.zeros(1, 8, dtype=torch.long),
          torch.ones(1, 8, dtype=torch.long))


def test_comm_library_exports_every_declared_symbol():
    """include/mmvqa_comm.h (the RCCL wrappers of SURVEY 8(b)): libmmvqa_comm.so loads and exports every entry point;
    no collective is issued (no GPU here)"""
    src = open(os.path.join(ROOT, "include", "mmvqa_comm.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = set(re.findall(r"\b(mmvqa_\w+)\s*\(", src))
    assert {"mmvqa_allreduce_bucket", "mmvqa_allgather", "mmvqa_broadcast", "mmvqa_comm_create", "mmvqa_comm_unique_id"} <= names
    from mmvqa_amd.ddp import NativeComm
    lib = NativeComm.lib()
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mmvqa_comm.h but not exported"
    assert lib.mmvqa_comm_rccl_version() > 20000
