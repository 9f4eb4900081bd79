"""The weight average of mmvqa_adam_ema / mmvqa_adam_groups_ema restated in float64, and the bound the fp32 kernel is
held to against it (tests/test_hip_adam_ema.py, tests/test_hip_ema_loop.py)."""
import torch

U24 = 2.0 ** -24


def omd32(decay):
    """(float)(1.0 - decay) as the launcher forms it: the double difference rounded once to fp32, back as a Python float"""
    return torch.tensor(1.0 - float(decay), dtype=torch.float64).float().double().item()


def ema_f64_step(E, p_new, decay):
    """E <- E + (p_new - E) * double(omd) in float64; p_new is the kernel's own fp32 parameter after the step"""
    return E + (p_new.detach().double().cpu() - E) * omd32(decay)


def ema_bound(K, M):
    """|ema - E| after K steps, elementwise: a step rounds the difference p_new - e (<= 2^-24 of a value <= 2 M, then
    multiplied by omd < 1) and the fused multiply-add (<= 2^-24 of a value <= M), so it adds at most 3 * 2^-24 * M; the
    error carried over is multiplied by decay < 1, so nothing grows: 3 K 2^-24 M, M the largest magnitude of p and ema
    over the run"""
    return 3.0 * K * U24 * M


def magnitude(*tensors):
    return max(float(t.detach().abs().max()) for t in tensors)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))
