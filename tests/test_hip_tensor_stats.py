"""mmvqa_tensor_stats on the GPU, through the C ABI, against the numpy restatement (tensor_stats_helpers.restate).

One buffer of about a quarter of a million floats holds every segment shape the kernels treat differently; every gap
between segments and the tail behind the last one are NaN, so a kernel that read padding would count it.  Counts, min,
max and all 64 bins must EQUAL the restatement; the fp64 sums are held to the worst-case bound of a summation in any
order (derived in the helper, not measured)."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mmvqa_amd import _lib as L  # noqa: E402
from mmvqa_amd.watch import RECORD  # noqa: E402
from tensor_stats_helpers import BINS, assert_record, restate  # noqa: E402

CK = L.TENSOR_STATS_CHUNK
TINY = np.float32(1.401298464324817e-45)


def run(buf, rows, flags=0, out=None):
    """one call over the device tensor `buf` (float32) with the table [(offset, numel)] -> (records, device bytes)"""
    lib = L.lib()
    host = (L.StatSeg * len(rows))()
    for h, (off, n) in zip(host, rows):
        h.offset, h.numel = off, n
    ws = lib.mmvqa_tensor_stats_workspace(C.cast(host, C.c_void_p), len(rows))
    assert ws > 0, lib.mmvqa_last_error()
    dev = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).cuda()
    if out is None:
        out = torch.zeros(len(rows) * RECORD.itemsize, dtype=torch.uint8, device="cuda")
    wsb = torch.empty(ws, dtype=torch.uint8, device="cuda")
    L.check(lib.mmvqa_tensor_stats(L.stream_ptr(), L.ptr(buf), buf.numel(), C.cast(host, C.c_void_p), L.ptr(dev), len(rows),
                                   L.ptr(out), L.ptr(wsb), ws, flags))
    torch.cuda.synchronize()
    raw = out.cpu().numpy().copy()
    return np.frombuffer(raw, dtype=RECORD), raw


def layout(parts, first_offset=0, gap=4):
    """place the arrays one after another on multiples of 4 floats with at least `gap` floats of NaN between them and a
    NaN tail -> (host buffer, [(offset, numel)])"""
    rows, pos = [], first_offset
    for x in parts:
        rows.append((pos, len(x)))
        pos = (pos + len(x) + gap + 3) // 4 * 4
    buf = np.full(pos + 64, np.nan, dtype=np.float32)
    for (off, n), x in zip(rows, parts):
        buf[off:off + n] = x
    return buf, rows


def segments():
    rng = np.random.default_rng(7)
    N = lambda n, s=1e-3: rng.normal(0.0, s, n).astype(np.float32)   # noqa: E731
    w = np.float32(4.0 / BINS)
    lower = np.float32(-2.0) + np.arange(BINS, dtype=np.float32) * w
    mixed = N(1000)
    mixed[[3, 500, 999]] = np.inf
    mixed[[4, 77]] = -np.inf
    mixed[[0, 5, 6, 640]] = np.nan
    conc = N(200_000, 1e-4)
    conc[1234], conc[150_001] = 0.05, -0.05
    return [
        ("first, 5", N(5)), ("empty", N(0)), ("1", N(1)), ("3", N(3)), ("4", N(4)),
        ("chunk - 1", N(CK - 1)), ("chunk", N(CK)), ("chunk + 1", N(CK + 1)),
        ("four chunks, ragged end", N(3 * CK + 37)),
        ("all nan", np.full(100, np.nan, dtype=np.float32)),
        ("inf, -inf and nan mixed in", mixed),
        ("all zero", np.zeros(300, dtype=np.float32)),
        ("signed zeros", np.float32([-0.0, 0.0, 1.0, -1.0, 0.0, -0.0])),
        ("power-of-two edges", np.concatenate([lower, lower + w / 2, np.float32([2.0])])),
        ("width overflows fp32", np.float32([-3e38, 3e38, 0, 1e38])),
        ("denormal width", (np.arange(65, dtype=np.float32) * TINY).astype(np.float32)),
        ("concentrated", conc),
        ("last, 7", N(7)),
    ]


@pytest.fixture(scope="module")
def big():
    """the buffer, its table, the restatement of every segment (computed once) and the records of one call"""
    segs = segments()
    host, rows = layout([x for _, x in segs])
    assert host.size < 1_000_000 and rows[0][0] == 0
    want = [restate(x) for _, x in segs]
    buf = torch.from_numpy(host).cuda()
    rec, raw = run(buf, rows)
    return dict(names=[n for n, _ in segs], rows=rows, want=want, buf=buf, rec=rec, raw=raw)


def test_every_segment_equals_the_restatement(big):
    assert np.isnan(big["buf"].cpu().numpy()[-64:]).all()
    for name, r, w in zip(big["names"], big["rec"], big["want"]):
        assert_record(r, w, name)
    by = dict(zip(big["names"], big["rec"]))
    e = by["empty"]
    assert e["n_finite"] == 0 and e["sum"] == 0 and e["sumsq"] == 0 and e["min"] == np.inf and e["max"] == -np.inf
    assert e["hist"].sum() == 0 and by["all nan"]["hist"].sum() == 0 and by["all nan"]["min"] == np.inf
    assert by["all zero"]["hist"][0] == 300 and by["all zero"]["n_zero"] == 300
    assert by["signed zeros"]["n_zero"] == 4
    assert sorted(np.nonzero(by["width overflows fp32"]["hist"])[0].tolist()) == [0, 32, 42, 63]
    assert by["denormal width"]["hist"].tolist() == [1] * 63 + [2]
    assert np.count_nonzero(by["concentrated"]["hist"]) <= 6 and by["concentrated"]["hist"].sum() == 200_000
    assert by["inf, -inf and nan mixed in"]["n_posinf"] == 3 and by["inf, -inf and nan mixed in"]["n_neginf"] == 2


def test_two_calls_give_identical_bytes(big):
    _, raw = run(big["buf"], big["rows"])
    assert np.array_equal(raw, big["raw"])


def test_moments_only_leaves_the_histogram_words_alone(big):
    out = torch.full((len(big["rows"]) * RECORD.itemsize,), 0xAB, dtype=torch.uint8, device="cuda")
    rec, _ = run(big["buf"], big["rows"], flags=L.TENSOR_STATS_MOMENTS_ONLY, out=out)
    assert (rec["hist"] == 0xABABABAB).all()
    for k in RECORD.names:
        if k != "hist":
            assert rec[k].tobytes() == big["rec"][k].tobytes(), k


@pytest.mark.parametrize("shift", [0, 1])
def test_table_of_one_segment(shift):
    """shift 1: the base pointer is 4 bytes past a 16-byte boundary, the path without float4 loads"""
    rng = np.random.default_rng(11)
    x = rng.normal(0.0, 1.0, 2 * CK + 1001).astype(np.float32)
    x[17] = np.nan
    host, rows = layout([x], first_offset=4)
    buf = torch.from_numpy(np.concatenate([np.full(shift, np.nan, np.float32), host])).cuda()
    rec, _ = run(buf[shift:], rows)
    assert len(rec) == 1
    assert_record(rec[0], restate(x), f"shift {shift}")


def test_a_thousand_tiny_segments():
    rng = np.random.default_rng(13)
    parts = [rng.normal(0.0, 1e-2, int(n)).astype(np.float32) for n in rng.integers(1, 65, 1000)]
    host, rows = layout(parts, gap=0)
    rec, _ = run(torch.from_numpy(host).cuda(), rows)
    for i, (r, x) in enumerate(zip(rec, parts)):
        assert_record(r, restate(x), f"segment {i} of {len(x)}")
