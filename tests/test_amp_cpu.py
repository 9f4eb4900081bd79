"""CPU checks of mixed-precision training's host side: the flag on every subcommand, its refusal together with
--overlap_adam, a disabled GradScaler passing everything through, and the f16 operand field of the GEMM descriptor."""
import ctypes as C

import pytest
import torch

from mmvqa_amd import _lib as L
from mmvqa_amd import train
from mmvqa_amd.amp import GradScaler


@pytest.mark.parametrize("mode", ["mlm", "supcon", "vqa", "eval"])
def test_every_subcommand_accepts_mixed_precision(mode, monkeypatch):
    seen = {}
    monkeypatch.setattr(train, "run_" + mode, lambda args: seen.setdefault("args", args))
    train.main([mode, "--mixed_precision"])
    assert seen["args"].mixed_precision is True


def test_overlap_adam_with_mixed_precision_refused(monkeypatch):
    monkeypatch.setattr(train, "run_mlm", lambda args: pytest.fail("must not run"))
    with pytest.raises(SystemExit):
        train.main(["mlm", "--mixed_precision", "--overlap_adam"])


def test_disabled_scaler_passes_everything_through():
    class Opt:
        calls = []

        def step(self, *a, **k):
            self.calls.append((a, k))
            return "stepped"

    sc = GradScaler(enabled=False)
    loss = torch.tensor(3.0)
    assert sc.scale(loss) is loss
    opt = Opt()
    sc.unscale_(opt)
    assert sc.step(opt, grad_scale=0.5, zero_grad=True) == "stepped"
    assert opt.calls == [((), {"grad_scale": 0.5, "zero_grad": True})]
    sc.update()
    assert sc.get_scale() == 1.0 and sc.state_dict() == {}
    assert not sc.is_enabled()


def test_igemm_f16_refusals():
    """the operand-precision field: unknown values and the prologues the f16 family lacks are refused on the host"""
    lib = L.lib()
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p).value

    def desc():
        d = L.GemmDesc()
        d.M, d.N, d.K = 64, 64, 64
        d.A = d.B = d.C = p
        d.a_ld = d.b_ld = d.c_ld = 64
        d.g_SH = d.g_SW = d.g_OH = d.g_OW = 1
        d.g_KH = d.g_KW = d.g_stride = 1
        d.g_Cs = 64
        return d

    d = desc()
    d.reserved0 = 7
    assert lib.mmvqa_igemm(C.byref(d), L.KIND_FWD, 0, 0, None) != 0
    assert b"precision" in lib.mmvqa_last_error()
    d = desc()
    d.reserved0 = L.PREC_F16
    d.a_pro, d.a_c0, d.a_c1 = L.PRO_AFFINE_SILU, p, p
    assert lib.mmvqa_igemm(C.byref(d), L.KIND_FWD, 0, 0, None) != 0
    assert b"f16" in lib.mmvqa_last_error()
