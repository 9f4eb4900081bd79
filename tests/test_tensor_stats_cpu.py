"""Host-side checks of the per-tensor statistics (--watch): known answers of the numpy restatement the GPU tests compare
the kernels with, its anchor against torch.histc, the argument checks of the two C ABI entry points (refused on the host
before any HIP call: no GPU here), the train.py flags and the JSON line."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

from tensor_stats_helpers import BINS, bins_of, restate


# ------------------------------------------------------------------------------------------------ the restatement
def test_power_of_two_range_centres_and_edges_land_in_their_bins():
    w = 4.0 / BINS                                            # min = -2, max = 2: every edge and centre is exact
    lower = np.float32(-2.0) + np.arange(BINS, dtype=np.float32) * np.float32(w)
    centre = lower + np.float32(w / 2)
    x = np.concatenate([lower, centre, np.float32([2.0])])
    r = restate(x)
    assert r["min"] == -2.0 and r["max"] == 2.0
    assert bins_of(lower, r["min"], r["max"]).tolist() == list(range(BINS))
    assert bins_of(centre, r["min"], r["max"]).tolist() == list(range(BINS))
    assert bins_of(np.float32([2.0]), r["min"], r["max"]).tolist() == [63]        # x == max
    want = np.full(BINS, 2)
    want[63] = 3
    assert r["hist"].tolist() == want.tolist()


def test_all_nan_is_an_empty_histogram():
    r = restate(np.full(7, np.nan, dtype=np.float32))
    assert r["n_finite"] == 0 and r["n_nan"] == 7 and r["hist"].sum() == 0
    assert r["min"] == np.inf and r["max"] == -np.inf and r["sum"] == 0.0 and r["sumsq"] == 0.0


def test_width_that_overflows_fp32():
    x = np.float32([-3e38, 3e38, 0, 1e38])
    with np.errstate(over="ignore"):
        assert not np.isfinite(np.float32(3e38) - np.float32(-3e38))               # the fp32 form of the rule breaks here
    r = restate(x)
    assert bins_of(x, r["min"], r["max"]).tolist() == [0, 63, 32, 42]
    assert sorted(np.nonzero(r["hist"])[0].tolist()) == [0, 32, 42, 63]


def test_denormal_width_is_spread_not_collapsed():
    tiny = np.float32(1.401298464324817e-45)                                       # the smallest denormal
    x = (np.arange(65, dtype=np.float32) * tiny).astype(np.float32)                # 65 distinct values, width 64 denormals
    assert len(np.unique(x)) == 65
    with np.errstate(over="ignore", divide="ignore"):
        assert not np.isfinite(np.float32(64.0) / (x.max() - x.min()))             # 64 / w overflows fp32
    r = restate(x)
    want = np.ones(BINS, dtype=np.int64)
    want[63] = 2
    assert r["hist"].tolist() == want.tolist()


def test_max_equals_min_and_signed_zeros():
    r = restate(np.float32([0.0, -0.0, 0.0]))
    assert r["n_zero"] == 3 and r["min"] == 0.0 and r["max"] == 0.0 and r["hist"][0] == 3 and r["hist"].sum() == 3
    r = restate(np.float32([np.inf, -np.inf, np.nan, 1.5, np.inf]))
    assert (r["n_finite"], r["n_nan"], r["n_posinf"], r["n_neginf"]) == (1, 1, 2, 1)
    assert r["min"] == r["max"] == 1.5 and r["hist"][0] == 1 and r["sum"] == 1.5 and r["sumsq"] == 2.25


def test_restatement_agrees_with_torch_histc():
    """the rule, not the kernel: torch.histc(bins=64) between min and max computes the position in fp32, so a value on an
    edge may fall to the other side; the summed absolute count difference is 0 for every size but the largest, where at
    most two elements (4 counts) may differ"""
    rng = np.random.default_rng(0)
    for n in (3, 4, 5, 1000, 16383, 16385, 50000, 2 ** 20):
        x = rng.normal(0.0, 1e-3, n).astype(np.float32)
        ref = torch.histc(torch.from_numpy(x), bins=BINS).numpy().astype(np.int64)
        diff = int(np.abs(restate(x)["hist"] - ref).sum())
        print(f"n={n}: summed |count difference| against torch.histc = {diff}")
        assert diff <= (4 if n == 2 ** 20 else 0), (n, diff)


# ------------------------------------------------------------------------------------------------ the C ABI on the host
def table(rows, fill=True):
    from mmvqa_amd import _lib as L
    host = (L.StatSeg * len(rows))()
    for h, (off, n) in zip(host, rows):
        h.offset, h.numel = off, n
    ws = L.lib().mmvqa_tensor_stats_workspace(C.cast(host, C.c_void_p), len(rows)) if fill else 0
    return host, ws


def test_workspace_query_fills_chunk0():
    from mmvqa_amd import _lib as L
    ck = L.TENSOR_STATS_CHUNK
    host, ws = table([(0, 0), (0, 5), (8, ck), (8 + ck, ck + 1), (4 * ck, 3 * ck - 1)])
    assert [h.chunk0 for h in host] == [0, 1, 2, 3, 5]           # an empty segment owns one chunk
    assert ws == 8 * 48
    assert L.lib().mmvqa_sizeof_stat_seg() == C.sizeof(L.StatSeg) == 24
    assert L.lib().mmvqa_sizeof_tensor_stat() == C.sizeof(L.TensorStat) == 320


def test_tensor_stats_refuses_bad_arguments_on_the_host():
    """every row is refused with MMVQA_ERR_ARG and its message before any HIP call (no GPU here; the pointers are never
    dereferenced on the device)"""
    from mmvqa_amd import _lib as L
    lib = L.lib()
    p = 0x1000
    good, ws = table([(0, 10), (12, 20), (32, 0)])
    host = C.cast(good, C.c_void_p)

    def call(base=p, n=64, segs=host, dev=p, nseg=3, out=p, wsp=p, ws_bytes=ws, flags=0):
        return lib.mmvqa_tensor_stats(None, base, n, segs, dev, nseg, out, wsp, ws_bytes, flags)

    def tab(rows):
        return C.cast(table(rows, fill=False)[0], C.c_void_p)

    cases = (
        (dict(base=None), b"null pointer"), (dict(segs=None), b"null pointer"), (dict(dev=None), b"null pointer"),
        (dict(out=None), b"null pointer"), (dict(wsp=None), b"null pointer"),
        (dict(nseg=0), b"nseg=0"), (dict(nseg=-3), b"nseg=-3"),
        (dict(segs=tab([(-4, 10), (12, 20), (32, 0)])), b"negative offset=-4"),
        (dict(segs=tab([(0, -1), (12, 20), (32, 0)])), b"numel=-1"),
        (dict(segs=tab([(0, 2 ** 32), (2 ** 33, 20), (2 ** 34, 0)])), b"more than a 32-bit histogram count holds"),
        (dict(n=31), b"reaches beyond the buffer's 31 floats"),
        (dict(n=-1), b"reaches beyond the buffer"),
        (dict(segs=tab([(0, 13), (12, 20), (32, 0)])), b"starts before the end 13"),          # overlapping
        (dict(segs=tab([(12, 20), (0, 10), (32, 0)])), b"starts before the end 32"),          # unsorted
        (dict(ws_bytes=ws - 1), b"workspace of 143 bytes, 144 needed"),
        (dict(flags=2), b"unknown flags=2"),
    )
    for kw, what in cases:
        rc = call(**kw)
        err = lib.mmvqa_last_error()
        assert rc == -1 and err.startswith(b"tensor_stats: ") and what in err, (kw, what, rc, err)
    stale = table([(0, 10), (12, 20), (32, 0)])[0]
    stale[2].chunk0 = 5                                          # a table the query did not fill
    rc = call(segs=C.cast(stale, C.c_void_p))
    assert rc == -1 and b"chunk0=5, expected 2" in lib.mmvqa_last_error()
    # the query applies the same table checks and answers 0
    for rows, what in (([(0, -1)], b"numel=-1"), ([(8, 4), (4, 4)], b"starts before the end 12")):
        host_bad, got = table(rows)
        err = lib.mmvqa_last_error()
        assert got == 0 and err.startswith(b"tensor_stats_workspace: ") and what in err, (rows, got, err)
    assert lib.mmvqa_tensor_stats_workspace(None, 3) == 0 and lib.mmvqa_tensor_stats_workspace(host, 0) == 0


# ------------------------------------------------------------------------------------------------ train.py and the line
def test_watch_flags_parse():
    from mmvqa_amd import train
    for mode in ("mlm", "supcon", "distill", "vqa"):
        _, a = train.parse_args([mode])
        assert a.watch is None and a.watch_freq == 1000
        _, a = train.parse_args([mode, "--watch", "gradients", "--watch_freq", "7"])
        assert a.watch == "gradients" and a.watch_freq == 7
    for what in ("parameters", "all"):
        assert train.parse_args(["mlm", "--watch", what])[1].watch == what
    assert train.parse_args(["mlm", "--watch", "parameters", "--overlap_adam"])[1].overlap_adam


@pytest.mark.parametrize("argv, what", [
    (["mlm", "--watch", "all", "--overlap_adam"], "--watch all cannot be combined with --overlap_adam"),
    (["vqa", "--watch", "gradients", "--overlap_adam"], "--watch gradients cannot be combined with --overlap_adam"),
    (["mlm", "--watch", "everything"], "invalid choice"),
    (["mlm", "--watch", "all", "--watch_freq", "0"], "--watch_freq 0 must be at least 1"),
])
def test_watch_flags_refused(argv, what, capsys):
    from mmvqa_amd import train
    with pytest.raises(SystemExit) as ex:
        train.parse_args(argv)
    assert ex.value.code == 2 and what in capsys.readouterr().err


def test_json_line_round_trips():
    from mmvqa_amd import watch as W
    rng = np.random.default_rng(1)

    def record(x, hist=True):
        r = restate(x)
        return dict(n_finite=r["n_finite"], n_nan=r["n_nan"], n_posinf=r["n_posinf"], n_neginf=r["n_neginf"],
                    n_zero=r["n_zero"], min=float(r["min"]), max=float(r["max"]), sum=r["sum"], sumsq=r["sumsq"],
                    hist=r["hist"].astype(np.uint32) if hist else None)

    a = rng.normal(0, 1e-3, 100).astype(np.float32)
    b = np.float32([np.nan, np.inf])
    names, numel, frozen = ["w", "b", "f"], [100, 2, 100], [False, False, True]
    grad = {"w": record(a), "b": record(b), "f": record(np.zeros(100, np.float32))}
    param = {"w": record(a * 3), "b": record(a[:2]), "f": record(a)}
    line = W.step_line(6, 1, "mlm", 0.5, 65536.0, names, numel, frozen, grad, param)
    assert "\n" not in line and "NaN" not in line and "Infinity" not in line          # strict JSON
    d = json.loads(line)
    assert json.dumps(d) == line
    assert (d["step"], d["epoch"], d["loop"], d["grad_scale"], d["loss_scale"]) == (6, 1, "mlm", 0.5, 65536.0)
    assert list(d["tensors"]) == names
    w = d["tensors"]["w"]
    assert w["numel"] == 100 and "frozen" not in w and len(w["grad"]["hist"]) == 64 and sum(w["grad"]["hist"]) == 100
    assert w["grad"]["edges"] == [float(a.min()), float(a.max())] and w["grad"]["sum"] == grad["w"]["sum"]
    assert w["param"]["edges"] == [float((a * 3).min()), float((a * 3).max())]
    assert d["tensors"]["b"]["grad"]["edges"] == [None, None] and d["tensors"]["b"]["grad"]["n_nan"] == 1
    f = d["tensors"]["f"]
    assert f["frozen"] is True and "grad" not in f and sum(f["param"]["hist"]) == 100
    # gradients only, no scaler
    d = json.loads(W.step_line(2, 0, "vqa", 1.0, None, names, numel, frozen, grad, None))
    assert d["loss_scale"] is None and "param" not in d["tensors"]["w"] and d["tensors"]["f"] == {"numel": 100, "frozen": True}
    # the line of a skipped step names the tensors with non-finite gradients, in buffer order
    moments = {k: record(v, hist=False) for k, v in (("w", a), ("b", b), ("f", np.float32([-np.inf])))}
    d = json.loads(W.skipped_line(9, 2, "mlm", 1024.0, moments))
    assert d == dict(step=9, epoch=2, loop="mlm", loss_scale=1024.0, skipped=True, nonfinite={"b": [1, 1, 0], "f": [0, 0, 1]})
