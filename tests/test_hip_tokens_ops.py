"""The two kernels of the visual-token cache (csrc/tokens.hip) against torch indexing.  Both are pure copies, so every
comparison is torch.equal: mmvqa_tokens_gather is cache[idx, view] in the engine's [num_vis][B][hidden] layout,
mmvqa_tokens_scatter its inverse for one view and distinct rows."""
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import P, dev  # noqa: E402

NUM_VIS = 5
HIDDEN = (8, 96, 312, 768, 1024)     # one lane of a wave, a partial wave, more than one 64-lane pass with a ragged tail, full
BATCH = (1, 3, 67)                   # 67 x 5 rows: more than one workgroup of four rows, the last one partial


def gather(cache, idx, view):
    N, K, nv, H = cache.shape
    B = idx.numel()
    out = torch.full((nv, B, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_tokens_gather(L.stream_ptr(), P(cache), N, K, P(idx), P(view), P(out), B, H, nv))
    return out


def scatter(vis, idx, view, cache):
    N, K, nv, H = cache.shape
    L.check(L.lib().mmvqa_tokens_scatter(L.stream_ptr(), P(vis), P(idx), view, P(cache), N, K, idx.numel(), H, nv))


def index_patterns(N, K, B):
    """(idx, view) [B] each: one index repeated; the first and the last image alternating at the last view; a seeded mix"""
    g = torch.Generator().manual_seed(100 * N + 10 * K + B)
    yield torch.full((B,), N // 2), torch.randint(0, K, (B,), generator=g)
    yield torch.tensor([0, N - 1] * B)[:B], torch.full((B,), K - 1)
    yield torch.randint(0, N, (B,), generator=g), torch.randint(0, K, (B,), generator=g)


@pytest.mark.parametrize("H", HIDDEN)
def test_gather_is_indexing(H):
    """torch.equal to cache[idx, view].permute(1, 0, 2) for every batch size, K in (1, 3), N in (1, 11) and index pattern"""
    for N, K in itertools.product((1, 11), (1, 3)):
        cache = torch.randn(N, K, NUM_VIS, H, generator=torch.Generator().manual_seed(N + K + H)).to(dev())
        for B in BATCH:
            for idx, view in index_patterns(N, K, B):
                out = gather(cache, idx.int().to(dev()), view.int().to(dev()))
                ref = cache[idx.to(dev()), view.to(dev())].permute(1, 0, 2)
                assert torch.equal(out, ref), (N, K, B, idx.tolist(), view.tolist())


@pytest.mark.parametrize("H", HIDDEN)
def test_scatter_then_gather_round_trips_and_spares_the_other_rows(H):
    """distinct rows of one view are written bit for bit (the gather reads them back), every other row of the cache keeps
    its sentinel"""
    SENTINEL = -7.25
    for N, K, B in ((1, 1, 1), (11, 3, 3), (67, 1, 67), (80, 3, 67)):
        g = torch.Generator().manual_seed(N + K + B + H)
        for view in sorted({0, K - 1}):
            cache = torch.full((N, K, NUM_VIS, H), SENTINEL, device=dev())
            idx = torch.randperm(N, generator=g)[:B]
            if B > 1:                                        # the last and the first image are among the distinct rows
                inner = 1 + torch.randperm(N - 2, generator=g)[:B - 2]
                idx = torch.cat([torch.tensor([N - 1, 0]), inner])[torch.randperm(B, generator=g)]
            n = idx.numel()
            assert n == B and torch.unique(idx).numel() == B
            vis = torch.randn(NUM_VIS, n, H, generator=g).to(dev())
            didx = idx.int().to(dev())
            scatter(vis, didx, view, cache)
            back = gather(cache, didx, torch.full((n,), view, dtype=torch.int32, device=dev()))
            assert torch.equal(back, vis), (N, K, B, view)
            assert torch.equal(cache[idx.to(dev()), view], vis.permute(1, 0, 2))
            untouched = torch.ones(N, K, dtype=torch.bool)
            untouched[idx, view] = False
            rest = cache.cpu()[untouched]
            assert rest.numel() == (N * K - n) * NUM_VIS * H and bool((rest == SENTINEL).all()), (N, K, B, view)
