"""CPU checks of Grad-CAM's host side: the new ABI symbols, the refusal of a backward before any forward, the sub-command's
options, the host colour table, and the test yardstick itself (two restatements of the formula agree)."""
import ctypes as C
import subprocess
import sys

import numpy as np
import pytest
import torch

from mmvqa_amd import _lib as L
from oracle import mmbert_oracle as O

import gradcam_helpers as GH


def test_new_symbols_and_refusal_before_forward():
    lib = L.lib()
    for name, nargs in (("mmvqa_engine_backward_feature", 5), ("mmvqa_engine_feature_map", 5), ("mmvqa_gradcam", 16)):
        assert hasattr(lib, name)
        assert len(L.SIGNATURES[name][1]) == nargs and L.SIGNATURES[name][0] is C.c_int
    import mmvqa_amd
    args = O.make_args(resnet_layers=(1, 1, 1, 1), resnet_width=8, hidden_size=96, n_layers=1, heads=12, vocab_size=11,
                       emb_vocab=50, bert_max_pos=32, dataset="VQA-Med")
    m = mmvqa_amd.Model(args)                       # CPU: the engine handle exists, nothing planned or run
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    rc = lib.mmvqa_engine_backward_feature(m._handle, None, p, 12, p)
    assert rc != 0 and b"forward" in lib.mmvqa_last_error()
    assert lib.mmvqa_engine_backward_feature(None, None, p, 12, p) != 0
    assert lib.mmvqa_gradcam(None, p, p, 1, 20, 20, 8, p, p, None, 0, 0, None, None, 0.4, None) != 0   # 400 positions
    assert b"gradcam" in lib.mmvqa_last_error()


def _help(mode):
    r = subprocess.run([sys.executable, "-m", "mmvqa_amd.train", mode, "--help"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r.stdout


def test_cli_options():
    g, e = _help("gradcam"), _help("eval")
    assert "--target" in g and "--limit" in g and "{answer,predicted}" in g
    assert "--target" not in e and "--limit" not in e
    assert "--category" in g and "--model_dir" in g and "--test_samples" in g     # the options of `eval`


def test_jet_table():
    from mmvqa_amd.gradcam import jet_table
    t = jet_table()
    assert t.shape == (256, 3) and t.dtype == np.uint8
    assert t[0].tolist() == [0, 0, 128] and t[255].tolist() == [128, 0, 0]           # dark blue -> dark red
    # the five breakpoints x = 1/8, 3/8, 1/2, 5/8, 7/8 of clamp(1.5 - |4x - k|): pure blue, cyan, mid green, yellow, red
    knots = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8]) / 8.0
    r9 = np.array([0, 0, 0, 0, .5, 1, 1, 1, .5])
    want = np.stack([np.interp(np.arange(256) / 255.0, knots, ch) for ch in (r9, np.array([0, 0, .5, 1, 1, 1, .5, 0, 0]), r9[::-1])], 1)
    assert np.abs(t.astype(np.float64) - want * 255.0).max() <= 0.5 + 1e-9
    for i, rgb in ((32, [0, 0, 255]), (96, [0, 255, 255]), (159, [255, 255, 0]), (223, [255, 0, 0])):
        assert np.abs(t[i].astype(int) - np.array(rgb)).max() <= 2, (i, t[i])
    assert abs(int(t[128][1]) - 255) == 0 and abs(int(t[128][0]) - int(t[128][2])) <= 4
    for ch, peak in ((0, (159, 223)), (1, (96, 159)), (2, (32, 96))):                # up, plateau, down
        d = np.diff(t[:, ch].astype(int))
        assert (d[:peak[0]] >= 0).all() and (d[peak[1]:] <= 0).all() and (t[peak[0]:peak[1], ch] >= 254).all()


def test_reference_cam_agrees_with_loops():
    g = torch.Generator().manual_seed(3)
    A = torch.randn(3, 4, 5, 8, generator=g).abs()
    dA = torch.randn(3, 4, 5, 8, generator=g)
    dA[2] = -dA[2].abs()                                                              # no positive evidence
    cam, valid = GH.reference_cam(A, dA)
    loops = GH.reference_cam_loops(A, dA)
    assert valid.tolist() == [True, True, False] and float(cam[2].abs().max()) == 0.0
    assert float((cam - loops).abs().max()) < 1e-12
    assert float(cam[:2].flatten(1).max(1).values.min()) == 1.0 and float(cam.min()) >= 0.0
    up = GH.bilinear_resize(cam, 8, 10)                                               # 2x: interior samples are 3:1 blends
    assert abs(float(up[0, 0, 0]) - float(cam[0, 0, 0])) < 1e-12                      # edge clamp
    want = 0.75 * (0.75 * cam[0, 0, 0] + 0.25 * cam[0, 0, 1]) + 0.25 * (0.75 * cam[0, 1, 0] + 0.25 * cam[0, 1, 1])
    assert abs(float(up[0, 1, 1]) - float(want)) < 1e-12
