"""mmvqa_attention_len_fwd (csrc/bertattn.hip) against float64 softmax attention.

Bound: 4 x the error of torch's own fp32 attention on the CPU against the same float64 values, measured here per launch
(maximum absolute error over the output).  The kernel's summation order differs from torch's (2-wide MFMA chunks, online
rescaling per 32-key tile); the number of roundings an output passes through does not."""
import pytest
import torch

import teacher_helpers as TH

pytestmark = pytest.mark.gpu

LENS = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129, 500)
GRID = ((2, 2, 37), (1, 12, 130), (2, 2, 512))


def _inputs(B, heads, T, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple(torch.randn(B, T, heads, 64, generator=g) for _ in range(3))      # q.k / 8 has unit variance


def _forms(q, k, v, dev, which):
    """the same values as slices of one fused [B, T, 3 * hidden] buffer, as three tensors, and at a base that is not
    16-byte aligned (element loads)"""
    B, T, heads, _ = q.shape
    H = heads * 64
    if which == "fused":
        qkv = torch.cat([t.reshape(B, T, H) for t in (q, k, v)], dim=2).to(dev)
        return tuple(qkv[:, :, i * H:(i + 1) * H].view(B, T, heads, 64) for i in range(3))
    if which == "separate":
        return tuple(t.contiguous().to(dev) for t in (q, k, v))
    out = []
    for t in (q, k, v):
        buf = torch.empty(t.numel() + 4, device=dev)
        view = buf[1:1 + t.numel()].view(t.shape)
        view.copy_(t)
        out.append(view)
    return tuple(out)


def _groups(B, T):
    lens = [n for n in LENS if n <= T] + [T]
    lens += lens[:(-len(lens)) % B]
    return [lens[i:i + B] for i in range(0, len(lens), B)]


@pytest.fixture(scope="module")
def cases():
    """per shape: the inputs and, per group of lengths, the float64 attention and torch's fp32 error against it"""
    out = {}
    for B, heads, T in GRID:
        q, k, v = _inputs(B, heads, T, 100 + T)
        refs = []
        for lens in _groups(B, T):
            r64 = TH.attention_ref(q.double(), k.double(), v.double(), lens)
            r32 = TH.attention_ref(q, k, v, lens)
            refs.append((lens, r64, float((r32.double() - r64).abs().max())))
        out[(B, heads, T)] = (q, k, v, refs)
    return out


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "B%d_h%d_T%d" % s)
@pytest.mark.parametrize("form", ["fused", "separate", "unaligned"])
def test_attention_len_fwd_against_float64(cases, shape, form):
    from mmvqa_amd.teacher import attention_len_fwd
    dev = torch.device("cuda:0")
    q, k, v, refs = cases[shape]
    dq, dk, dv = _forms(q, k, v, dev, form)
    worst = 0.0
    for lens, r64, e32 in refs:
        out = attention_len_fwd(dq, dk, dv, torch.tensor(lens, dtype=torch.int32, device=dev))
        err = float((out.cpu().double() - r64).abs().max())
        ratio = err / e32 if e32 > 0.0 else (0.0 if err == 0.0 else float("inf"))   # one key: both are exact (out = v[0])
        worst = max(worst, ratio)
        print(f"{shape} {form} lens {lens}: |err| {err:.3e}, torch fp32 on the CPU {e32:.3e}, ratio {ratio:.2f}")
        assert err <= 4.0 * e32, (shape, form, lens, err, e32)
    print(f"{shape} {form}: worst ratio {worst:.2f}")


def test_rescale_is_forced_by_a_late_spike():
    """a key in the LAST tile that matches its query: the running maximum jumps there and every earlier tile's
    contribution is rescaled by a tiny factor (random data alone moves the maximum by a few units at most)"""
    from mmvqa_amd.teacher import attention_len_fwd
    dev = torch.device("cuda:0")
    q, k, v = _inputs(2, 2, 130, 7)
    k[:, 128] = 3.0 * q[:, 5]                      # query 5 of every (b, head) against key 128: score ~ 3 * 64 / 8
    k[0, 40] = 2.0 * q[0, 100]                     # and a jump in the middle tile for another row
    lens = [129, 130]
    r64 = TH.attention_ref(q.double(), k.double(), v.double(), lens)
    e32 = float((TH.attention_ref(q, k, v, lens).double() - r64).abs().max())
    out = attention_len_fwd(q.to(dev), k.to(dev), v.to(dev), torch.tensor(lens, dtype=torch.int32, device=dev))
    err = float((out.cpu().double() - r64).abs().max())
    print(f"spiked: |err| {err:.3e}, torch fp32 {e32:.3e}, ratio {err / e32:.2f}")
    assert err <= 4.0 * e32


def test_exactness_properties():
    from mmvqa_amd.teacher import attention_len_fwd
    dev = torch.device("cuda:0")
    B, heads, T = 2, 2, 130
    q, k, v = _inputs(B, heads, T, 11)
    lens = [33, 129]
    q[0, 33 + 7] = q[0, 3]                         # a padded query row (tile 1, lane 8) with a valid row's q (tile 0, lane 3)
    q[1, 129] = q[1, 64]
    dl = torch.tensor(lens, dtype=torch.int32, device=dev)
    dq, dk, dv = q.to(dev), k.to(dev), v.to(dev)
    a = attention_len_fwd(dq, dk, dv, dl)
    b = attention_len_fwd(dq, dk, dv, dl)
    assert torch.equal(a, b)                                        # bit-equal from launch to launch
    assert torch.isfinite(a).all()
    # rows >= len of k / v are never read: any value there leaves every output bit as it was
    k2, v2 = dk.clone(), dv.clone()
    for s, n in enumerate(lens):
        k2[s, n:] = 1e30
        v2[s, n:] = 1e30
    assert torch.equal(attention_len_fwd(dq, k2, v2, dl), a)
    k2[0, 33:] = float("nan")
    v2[0, 33:] = float("inf")
    assert torch.equal(attention_len_fwd(dq, k2, v2, dl), a)
    # a query row >= len is computed like any other row: same q, same bits
    assert torch.equal(a[0, 40], a[0, 3]) and torch.equal(a[1, 129], a[1, 64])
    # a bad length: NaN rows in that sample only, the other sample untouched
    for bad in (0, -5, T + 1):
        o = attention_len_fwd(dq, dk, dv, torch.tensor([bad, 129], dtype=torch.int32, device=dev))
        assert torch.isnan(o[0]).all() and torch.equal(o[1], a[1]), bad
    o = attention_len_fwd(dq, dk, dv, torch.tensor([33, 0], dtype=torch.int32, device=dev))
    assert torch.isnan(o[1]).all() and torch.equal(o[0], a[0])
    # the output buffer may have its own strides: rows of a wider buffer
    wide = torch.zeros(B, T, 3 * heads * 64, device=dev)
    view = wide[:, :, heads * 64:2 * heads * 64].view(B, T, heads, 64)
    attention_len_fwd(dq, dk, dv, dl, out=view)
    assert torch.equal(view, a) and float(wide[:, :, :heads * 64].abs().max()) == 0.0 and float(wide[:, :, 2 * heads * 64:].abs().max()) == 0.0
