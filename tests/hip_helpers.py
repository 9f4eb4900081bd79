"""Helpers for the GPU parity tests: build C-ABI descriptors from torch tensors."""
import ctypes as C
import math

import torch

import mmvqa_amd
from mmvqa_amd import _lib as L


def dev():
    return torch.device("cuda:0")


def P(t):
    return None if t is None else t.data_ptr()


def nhwc(x):
    """NCHW tensor -> contiguous NHWC copy on the GPU"""
    return x.permute(0, 2, 3, 1).contiguous().to(dev())


def from_nhwc(x, N, H, W, Cc):
    return x.view(N, H, W, Cc).permute(0, 3, 1, 2).contiguous().cpu()


def w_ohwi(w):
    """OIHW conv weight -> [O][KH][KW][I] on the GPU"""
    return w.permute(0, 2, 3, 1).contiguous().to(dev())


def linear_geom(d):
    d.g_SH = d.g_SW = d.g_OH = d.g_OW = 1
    d.g_KH = d.g_KW = 1
    d.g_stride = 1
    d.g_pad = 0


def run_igemm(d, kind, nchw=0, tile=0):
    L.check(L.lib().mmvqa_igemm(C.byref(d), kind, nchw, tile, L.stream_ptr()))
    torch.cuda.synchronize()


def conv_desc_fwd(x_nhwc, w_ohwi_t, N, H, W, Cin, Cout, K, stride, pad, out):
    OH = (H + 2 * pad - K) // stride + 1
    OW = (W + 2 * pad - K) // stride + 1
    d = L.GemmDesc()
    d.M, d.N, d.K = N * OH * OW, Cout, K * K * Cin
    d.A, d.a_ld = P(x_nhwc), Cin
    d.B, d.b_ld = P(w_ohwi_t), K * K * Cin
    d.g_SH, d.g_SW, d.g_Cs, d.g_OH, d.g_OW = H, W, Cin, OH, OW
    d.g_KH = d.g_KW = K
    d.g_stride, d.g_pad = stride, pad
    d.C, d.c_ld = P(out), Cout
    return d, OH, OW


def conv_desc_dgrad(dz_nhwc, w_ohwi_t, N, H, W, Cin, Cout, K, stride, pad, out):
    OH = (H + 2 * pad - K) // stride + 1
    OW = (W + 2 * pad - K) // stride + 1
    d = L.GemmDesc()
    d.M, d.N, d.K = N * H * W, Cin, K * K * Cout
    d.A, d.a_ld = P(dz_nhwc), Cout
    d.g_SH, d.g_SW, d.g_Cs, d.g_OH, d.g_OW = OH, OW, Cout, H, W
    d.g_KH = d.g_KW = K
    d.g_stride, d.g_pad = stride, pad
    d.B, d.b_ld, d.b_tapstride = P(w_ohwi_t), K * K * Cin, Cin
    d.C, d.c_ld = P(out), Cin
    return d


def conv_desc_wgrad(dz_nhwc, x_nhwc, N, H, W, Cin, Cout, K, stride, pad, out):
    OH = (H + 2 * pad - K) // stride + 1
    OW = (W + 2 * pad - K) // stride + 1
    d = L.GemmDesc()
    d.M, d.N, d.K = Cout, K * K * Cin, N * OH * OW
    d.A, d.a_ld = P(dz_nhwc), Cout
    d.B, d.b_ld = P(x_nhwc), Cin
    d.g_SH, d.g_SW, d.g_Cs, d.g_OH, d.g_OW = H, W, Cin, OH, OW
    d.g_KH = d.g_KW = K
    d.g_stride, d.g_pad = stride, pad
    d.C, d.c_ld, d.c_atomic = P(out), K * K * Cin, 1
    return d


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def assert_close(a, b, tol, what=""):
    e = relerr(a, b)
    assert e <= tol, f"{what}: rel-to-max error {e:.3e} > {tol:.1e}"


# ----------------------------------------------------------------------------- per-element error bounds
# assert_close measures the error against the tensor's maximum, so a wrong value in a low-magnitude region (the rows of one
# image, one border of a padded convolution) can hide under it.  The bound below holds for every element on its own.
U23 = 2.0 ** -23


def dot_ulps(K):
    """c of a K-term fp32 dot product, in units of 2^-23 of sum_k |a_k b_k|.

    Whatever the kernel's association order -- MFMA accumulator chains, the two K halves of the 8-wave tile, split-K
    partial tiles, float atomics into C -- every output element is a binary tree over its K products (zero-padded K
    terms add exactly).  A product passes its own rounding and at most K - 1 additions, each <= 2^-24 relative, so
    |err| <= gamma_K * sum_k |a_k b_k| with gamma_K = K 2^-24 / (1 - K 2^-24) (Higham, Accuracy and Stability of
    Numerical Algorithms, 3.1).  The + 1 absorbs the rounding of that quotient."""
    return math.ceil(K / (2.0 * (1.0 - K * 2.0 ** -24))) + 1


def assert_within(out, ref, bound, what=""):
    """|out - ref| <= bound for every element (NaN / Inf in out fail)"""
    out, ref, bound = out.double().cpu(), ref.double().cpu(), bound.double().cpu()
    err = (out - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.argmax(torch.where(bad, err / bound.clamp_min(1e-300), torch.zeros_like(err)).reshape(-1)))
        idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), out.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {out.numel()} elements outside the bound; worst at {idx}: "
                             f"out {out[idx].item():.9g} ref {ref[idx].item():.9g} |err| {err[idx].item():.3e} "
                             f"bound {bound[idx].item():.3e}")


def assert_gemm_close(out, ref, mag, c, what="", tol=1e-4):
    """per element |out - ref| <= c * 2^-23 * mag, mag = |A'| @ |B'| (or a larger magnitude that also covers the
    prologue's own rounding), then the max-relative check of the other op tests"""
    assert_within(out, ref, c * U23 * mag.double() + 1e-30, what)
    assert_close(out, ref, tol, what)
