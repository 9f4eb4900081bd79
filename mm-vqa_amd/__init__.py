"""mm-vqa_amd: MI355X-native (gfx950) MMBERT training hot path of DannielSilva/MM-VQA.

Import as ``mmvqa_amd`` (the directory name carries a hyphen; the top-level ``mmvqa_amd`` package
points here).  All arithmetic is in libmmvqa_hip.so (mm-vqa_amd/csrc, C ABI in include/mmvqa.h).
"""
from . import _lib
from ._lib import MMVQAError
from .model import Model, desc_from_args
from .functional import mlm_loss, asl_loss, supcon_loss, split_feat, jaccard_mask, embedding_mask
from .functional import soft_ce_loss, CategorySmoothing, LabelSmoothing, distill_loss
from .optim import FusedAdam, no_decay
from .teacher import BertTeacher, bertscore_mask
from . import synth
from . import amp

__all__ = ["Model", "desc_from_args", "mlm_loss", "asl_loss", "supcon_loss", "split_feat", "jaccard_mask", "embedding_mask", "FusedAdam", "synth",
           "MMVQAError", "amp", "soft_ce_loss", "CategorySmoothing", "LabelSmoothing", "distill_loss", "BertTeacher",
           "bertscore_mask", "no_decay"]
