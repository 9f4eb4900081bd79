"""The two kernels of a grouped batch (csrc/group.hip) through the C ABI, bit for bit.

mmvqa_vis_expand is a gather of whole rows: the reference is index_select.  mmvqa_dvis_group_sum adds the rows of an
image in ascending b starting from the first row; the reference is that loop in fp32 on the host.  It is additions only
(no product that could be contracted into an FMA), each one correctly rounded, so the IEEE result of the stated order is
unique and there is no tolerance.  Both ops run twice and must repeat themselves exactly (no atomics)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from hip_helpers import dev, P  # noqa: E402

NUM_VIS = 5
# smallest the engine allows | the reference's default, 78 float4 per row: the wave's second pass is partial | config width
HIDDEN = (8, 312, 768)
# smallest | uneven groups | identity: both ops equal a copy | one group longer than any workgroup
GROUPS = ((1, 1, [1]), (3, 7, [1, 4, 2]), (5, 5, [1] * 5), (1, 130, [130]))


def maps(counts):
    group = torch.repeat_interleave(torch.arange(len(counts)), torch.tensor(counts)).int()
    offsets = torch.tensor([0] + torch.tensor(counts).cumsum(0).tolist(), dtype=torch.int32)
    return group, offsets


def expand(vis_i, group, B, H):
    NI = vis_i.shape[1]
    out = torch.full((NUM_VIS, B, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_vis_expand(L.stream_ptr(), P(vis_i), P(group), P(out), NI, B, H, NUM_VIS))
    torch.cuda.synchronize()
    return out


def group_sum(dvis_q, offsets, NI, H):
    B = dvis_q.shape[1]
    out = torch.full((NUM_VIS, NI, H), float("nan"), device=dev())
    L.check(L.lib().mmvqa_dvis_group_sum(L.stream_ptr(), P(dvis_q), P(offsets), P(out), NI, B, H, NUM_VIS))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("NI,B,counts", GROUPS)
def test_vis_expand_is_index_select(NI, B, counts, H):
    assert sum(counts) == B and len(counts) == NI
    g = torch.Generator().manual_seed(100 * B + H)
    vis_i = torch.randn(NUM_VIS, NI, H, generator=g)
    group, _ = maps(counts)
    ref = vis_i.index_select(1, group.long())
    out = expand(vis_i.to(dev()), group.to(dev()), B, H)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(expand(vis_i.to(dev()), group.to(dev()), B, H), out)
    if NI == B:
        assert torch.equal(out.cpu(), vis_i)


@pytest.mark.parametrize("H", HIDDEN)
@pytest.mark.parametrize("NI,B,counts", GROUPS)
def test_dvis_group_sum_is_the_sequential_fp32_loop(NI, B, counts, H):
    g = torch.Generator().manual_seed(200 * B + H)
    # magnitudes spread over several binades, so that another order of the same additions rounds differently
    dq = torch.randn(NUM_VIS, B, H, generator=g) * torch.exp2(torch.randint(-6, 7, (NUM_VIS, B, 1), generator=g).float())
    _, offsets = maps(counts)
    ref = torch.empty(NUM_VIS, NI, H)
    for i in range(NI):
        b0, b1 = int(offsets[i]), int(offsets[i + 1])
        acc = dq[:, b0].clone()                       # starts from the first row, not from zero
        for b in range(b0 + 1, b1):                   # ascending b, one fp32 addition each
            acc = acc + dq[:, b]
        ref[:, i] = acc
    out = group_sum(dq.to(dev()), offsets.to(dev()), NI, H)
    assert torch.equal(out.cpu(), ref)
    assert torch.equal(group_sum(dq.to(dev()), offsets.to(dev()), NI, H), out)
    if NI == B:
        assert torch.equal(out.cpu(), dq)


def test_a_negative_zero_survives_the_sum():
    """the sum starts from the first row: a group of one row is a copy, -0.0 included (0.0 + -0.0 would be +0.0)"""
    dq = torch.zeros(NUM_VIS, 2, 8)
    dq[:, 0] = -0.0
    _, offsets = maps([1, 1])
    out = group_sum(dq.to(dev()), offsets.to(dev()), 2, 8).cpu()
    assert torch.equal(torch.signbit(out), torch.signbit(dq))


def test_argument_checks():
    lib = L.lib()
    p = 0x1000   # never dereferenced: every case is refused first
    for fn, who in ((lib.mmvqa_vis_expand, b"vis_expand"), (lib.mmvqa_dvis_group_sum, b"dvis_group_sum")):
        # (a, idx, c, NI, B, H, num_vis)
        for args in ((None, p, p, 2, 4, 8, 5), (p, None, p, 2, 4, 8, 5), (p, p, None, 2, 4, 8, 5),   # null pointers
                     (p, p, p, 0, 4, 8, 5),                                                          # NI < 1
                     (p, p, p, 5, 4, 8, 5),                                                          # B < NI
                     (p, p, p, 2, 4, 10, 5),                                                         # H % 4
                     (p, p, p, 2, 4, 8, 0)):                                                         # num_vis < 1
            rc = fn(None, *args)
            assert rc == -1 and lib.mmvqa_last_error().startswith(who + b":"), (who, args, rc, lib.mmvqa_last_error())
