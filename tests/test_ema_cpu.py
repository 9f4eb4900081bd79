"""Host side of the weight average (no GPU): what mmvqa_adam_ema, mmvqa_adam_groups_ema and mmvqa_swap refuse before any
HIP call, the warm-up schedule of the decay, the parser's refusals and averaged() without averaging."""
import argparse
import contextlib
import ctypes as C

import pytest
import torch

from mmvqa_amd import _lib as L

B1, B2, EPS = 0.9, 0.999, 1e-8
# small host addresses, 4 KiB apart: never dereferenced, every call below is refused first
PP, PG, PM, PV, PE = 0x10000, 0x11000, 0x12000, 0x13000, 0x14000


def adam_ema(ema=PE, n=64, decay=0.9, p=PP):
    return L.lib().mmvqa_adam_ema(None, p, PG, PM, PV, ema, n, 1e-3, B1, B2, EPS, 1, 1.0, 1, decay)


def one_segment(n):
    host = (L.AdamSeg * 1)()
    host[0].begin, host[0].end, host[0].lr, host[0].weight_decay, host[0].mode = 0, n, 1e-3, 0.0, L.ADAM_L2
    return host


def groups_ema(ema=PE, lo=0, n=64, decay=0.9, extent=64, nseg=1):
    host = one_segment(extent)
    return L.lib().mmvqa_adam_groups_ema(None, PP, PG, PM, PV, ema, lo, n, C.cast(host, C.c_void_p), 0x20000, nseg,
                                         B1, B2, EPS, 1, 1.0, 1, decay)


def refused(rc, prefix, what):
    err = L.lib().mmvqa_last_error()
    assert rc == L.ERR_ARG and err.startswith(prefix) and what in err, (rc, err)


@pytest.mark.parametrize("call, prefix", [(adam_ema, b"adam_ema: "), (groups_ema, b"adam_groups_ema: ")])
def test_averaging_entry_points_refuse_on_the_host(call, prefix):
    refused(call(ema=None), prefix, b"ema is null")
    for d in (1.0, -0.01, 1.5, float("nan"), float("inf")):
        refused(call(decay=d), prefix, b"ema_decay")
    # the average against each of the other four buffers: the same start, its last float on their first, their last
    # float on its first
    for base, name in ((PP, b"p"), (PG, b"g"), (PM, b"m"), (PV, b"v")):
        for ema in (base, base - 4 * 63, base + 4 * 63):
            refused(call(ema=ema), prefix, b"ema overlaps " + name)


def test_groups_form_checks_the_range_of_the_launch():
    """a ranged launch: [ema + lo, ema + lo + n) against the whole of the other buffers (the table's extent)"""
    # 128 floats per buffer; the average's range [64, 128) of this launch, placed on p's [0, 64): refused although p's
    # own range of the launch is [64, 128)
    refused(groups_ema(ema=PP - 4 * 64, lo=64, n=64, extent=128), b"adam_groups_ema: ", b"ema overlaps p")
    # what mmvqa_adam_groups checks is checked the same way, with its message
    refused(groups_ema(n=6), b"adam_groups: ", b"multiples of 4")
    refused(groups_ema(nseg=0), b"adam_groups: ", b"nseg=0")
    refused(groups_ema(n=68), b"adam_groups: ", b"beyond the table")
    refused(adam_ema(n=6), b"adam: ", b"multiple of 4")


def test_swap_refuses_on_the_host():
    lib = L.lib()
    for n in (1, 2, 3, 6, 2050):
        refused(lib.mmvqa_swap(None, PP, PG, n), b"swap: ", b"multiple of 4")
    refused(lib.mmvqa_swap(None, None, PG, 4), b"swap: ", b"null pointer")
    refused(lib.mmvqa_swap(None, PP, None, 4), b"swap: ", b"null pointer")
    refused(lib.mmvqa_swap(None, PP, PP + 16, 8), b"swap: ", b"overlap")
    refused(lib.mmvqa_swap(None, PP + 4, PG, 4), b"swap: ", b"aligned")


def test_warmup_schedule():
    from mmvqa_amd.optim import ema_decay_at
    d = 0.999
    assert ema_decay_at(d, 0, True) == 0.1                      # (1 + 0) / (10 + 0)
    assert ema_decay_at(d, 1, True) == 2.0 / 11.0
    assert ema_decay_at(d, 90, True) == 0.91                    # 91 / 100
    # (1 + t) / (10 + t) >= 0.999  <=>  t >= (10 * 0.999 - 1) / (1 - 0.999) = 8990
    assert ema_decay_at(d, 8989, True) == 8990.0 / 8999.0 < d
    assert ema_decay_at(d, 8990, True) == d and ema_decay_at(d, 10 ** 6, True) == d
    # a small decay is reached at once: (1 + 0) / 10 = 0.1 >= 0.05
    assert ema_decay_at(0.05, 0, True) == 0.05
    for t in (0, 1, 90, 8990):
        assert ema_decay_at(d, t, False) == d                   # without warm-up: the decay itself
    # non-decreasing in t
    seq = [ema_decay_at(d, t, True) for t in range(0, 9100, 13)]
    assert all(a <= b for a, b in zip(seq, seq[1:]))


def test_parser_refusals(capsys):
    from mmvqa_amd import train
    for mode in ("mlm", "supcon", "distill", "vqa"):
        for bad in ("1.0", "-0.1", "1.5", "nan"):
            with pytest.raises(SystemExit):
                train.parse_args([mode, "--ema_decay", bad])
            assert "--ema_decay" in capsys.readouterr().err
        with pytest.raises(SystemExit):
            train.parse_args([mode, "--ema_warmup"])
        assert "--ema_warmup requires --ema_decay" in capsys.readouterr().err
        _, args = train.parse_args([mode])
        assert args.ema_decay is None and args.ema_warmup is False
        assert "ema_decay" not in train.optimizer_groups(args)          # flag off: the optimizer is built as before
        _, args = train.parse_args([mode, "--ema_decay", "0.99", "--ema_warmup"])
        kw = train.optimizer_groups(args)
        assert kw["ema_decay"] == 0.99 and kw["ema_warmup"] is True
        _, args = train.parse_args([mode, "--ema_decay", "0"])
        assert train.optimizer_groups(args)["ema_decay"] == 0.0
    with pytest.raises(ValueError, match="outside"):
        train.check_optimizer_args(argparse.Namespace(ema_decay=1.0))
    with pytest.raises(ValueError, match="requires --ema_decay"):
        train.check_optimizer_args(argparse.Namespace(ema_decay=None, ema_warmup=True))


class Flat:
    def __init__(self, n):
        self.flat_params = torch.arange(n, dtype=torch.float32)
        self.flat_grads = torch.zeros(n)


def test_optimizer_without_and_with_averaging_on_the_host():
    import mmvqa_amd
    opt = mmvqa_amd.FusedAdam(Flat(8), lr=1e-3)
    assert opt.ema is None and opt.ema_decay is None
    ctx = opt.averaged()
    assert isinstance(ctx, contextlib.nullcontext)
    with ctx:
        pass
    assert not {"ema", "ema_decay", "ema_warmup", "ema_updates"} & set(opt.state_dict())
    for bad in (1.0, -0.5, float("nan")):
        with pytest.raises(ValueError, match="ema_decay"):
            mmvqa_amd.FusedAdam(Flat(8), ema_decay=bad)
    with pytest.raises(ValueError, match="ema_warmup"):
        mmvqa_amd.FusedAdam(Flat(8), ema_warmup=True)
    flat = Flat(8)
    avg = mmvqa_amd.FusedAdam(flat, ema_decay=0.9, ema_warmup=True)
    assert torch.equal(avg.ema, flat.flat_params) and avg.ema.data_ptr() != flat.flat_params.data_ptr()
    assert avg.ema_updates == 0
    sd = avg.state_dict()
    assert (sd["ema_decay"], sd["ema_warmup"], sd["ema_updates"]) == (0.9, True, 0) and sd["ema"] is avg.ema
    # a checkpoint with an average into a plain optimizer: ignored
    opt.load_state_dict(sd)
    assert opt.ema is None
