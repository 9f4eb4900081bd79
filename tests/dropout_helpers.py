"""Host restatement of the dropout stream ("Dropout stream"): the counter-based hash of csrc/common.h in
numpy, the site seeds of csrc/engine.cpp, and the oracle's nn.Dropout modules replaced by the masks the kernels draw.
With the masks known, a training-mode step is a deterministic function and is held to the dropout-free tolerances."""
import numpy as np
import torch

from oracle import mmbert_oracle as O

EMB_LAYER = 100   # the embedding dropout is site (100, 0)


def _u32(v):
    return np.uint32(int(v) & 0xFFFFFFFF)


def rng_uniform(seed, idx):
    """common.h rng_uniform: (seed, index) -> float32 in [0, 1), uint32 wraparound arithmetic"""
    seed = _u32(seed)
    with np.errstate(over="ignore"):
        x = np.asarray(idx).astype(np.uint32) * np.uint32(0x9E3779B1) + seed
        x ^= x >> np.uint32(16)
        x *= np.uint32(0x7FEB352D)
        x ^= x >> np.uint32(15)
        x *= np.uint32(0x846CA68B)
        x ^= x >> np.uint32(16)
        x += seed * np.uint32(0x85EBCA6B)
        x ^= x >> np.uint32(13)
        x *= np.uint32(0xC2B2AE35)
        x ^= x >> np.uint32(16)
        return (x >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def site_seed(seed, layer, site):
    """engine.cpp site_seed: the stream of dropout site `site` of encoder layer `layer` in a step with base seed `seed`"""
    return (int(seed) + 0x9E3779B9 * (layer * 8 + site + 1)) & 0xFFFFFFFF


def engine_seed(s):
    """the base seed Model._engine_forward hands to the engine in the first forward after Model.set_seed(s)"""
    return ((int(s) & 0x7FFFFFFF) * 1103515245 + 12345) & 0x7FFFFFFF


def all_sites(n_layers):
    """every (layer, site) a step of an n_layers encoder draws from"""
    return [(EMB_LAYER, 0)] + [(i, s) for i in range(n_layers) for s in range(3)]


def keep_mask(seed, shape, p):
    """bool array of `shape`: element with linear index i (contiguous layout) is kept iff rng_uniform(seed, i) >= p"""
    n = int(np.prod(shape))
    return (rng_uniform(seed, np.arange(n, dtype=np.uint32)) >= np.float32(p)).reshape(shape)


def keep_tensor(seed, shape, p):
    return torch.from_numpy(keep_mask(seed, tuple(shape), p))


class SiteDropout(torch.nn.Module):
    """nn.Dropout replaced by the kernels' mask of one site.  Holds numbers only (no tensors), so that
    copy.deepcopy(model).double() keeps working.  layer=None: a module shared by all layers (OracleBertLayer.drop1 /
    drop2); its layer is the number of calls since the root module's forward began."""

    def __init__(self, p, seed, layer, site):
        super().__init__()
        self.p, self.seed, self.layer, self.site = float(p), int(seed), layer, int(site)
        self.calls = 0

    def forward(self, x):
        layer = self.calls if self.layer is None else self.layer
        self.calls += 1
        if self.p == 0.0 or not self.training:
            return x
        keep = keep_tensor(site_seed(self.seed, layer, self.site), x.shape, self.p)
        return x * (keep.to(x.dtype) / (1.0 - self.p))

    def extra_repr(self):
        return f"p={self.p}, seed={self.seed}, layer={self.layer}, site={self.site}"


def _reset_calls(module, args):
    for m in module.modules():
        if isinstance(m, SiteDropout):
            m.calls = 0


def inject_dropout(orc, seed):
    """replace every nn.Dropout below `orc` (an oracle model, or one of its encoders / embeddings) by the site it is in
    the engine; `seed` is the engine's base seed of the step.  Nothing under oracle/ changes: the instance does."""
    for m in list(orc.modules()):
        if isinstance(m, O.OracleBertEmbeddings):
            m.dropout = SiteDropout(m.dropout.p, seed, EMB_LAYER, 0)
        elif isinstance(m, O.OracleBertLayer):
            for i, att in enumerate(m.attention):
                att.drop = SiteDropout(att.drop.p, seed, i, 0)
            m.drop1 = SiteDropout(m.drop1.p, seed, None, 1)
            m.drop2 = SiteDropout(m.drop2.p, seed, None, 2)
        elif isinstance(m, O.OracleRealFormer):
            for i, blk in enumerate(m.mains):
                blk.dp = SiteDropout(blk.dp.p, seed, i, 1)
                blk.ff[3] = SiteDropout(blk.ff[3].p, seed, i, 2)
    left = [n for n, m in orc.named_modules() if isinstance(m, torch.nn.Dropout)]
    assert not left, f"nn.Dropout modules without a site: {left}"
    orc.register_forward_pre_hook(_reset_calls)
    return orc
