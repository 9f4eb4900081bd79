"""Device input pipeline: the reference's image transforms on the GPU.

Reference (host, per sample, torchvision transforms on PIL images):
  pretrain/roco_train.py:98-112   Resize(224) CenterCrop(224) RandomResizedCrop(224, (0.95,1.05), (0.95,1.05))
                                  RandomRotation(5) ColorJitter(0.05 x4) ToTensor Normalize(0.5, 0.5)
  vqamed2019/train.py:179-200     same chain with scale/ratio (0.75,1.25), RandomRotation(10), ColorJitter(0.4 x4)
  validation / test               Resize(224) CenterCrop(224) ToTensor Normalize
Here: decoded uint8 RGB images (JPEG decoding stays on the host: the image has no GPU JPEG decoder) are copied to
HBM once and every transform runs as a HIP kernel (csrc/augment.hip) that restates Pillow's byte arithmetic bit for
bit; the random parameters are drawn on the host from torch's generator in torchvision's order (torchvision is a
third-party dependency, unpinned by the reference and absent from the build image: its thin parameter-sampling
wrappers are restated from the published source -- "parity unpinned" for the draw order; the pixel arithmetic is
pinned against Pillow itself, tests/test_augment.py).

    aug = DeviceAugment(train=True)                      # ROCO pre-training settings
    x = aug(list_of_uint8_HWC_arrays)                    # -> float32 [B, 3, 224, 224] on the GPU

For a training loop, run_packed() takes a ragged batch that is already on the device and only enqueues work on a
stream: one pinned blob of tables / jobs / records goes up by one async copy, then Resize+CenterCrop (2 launches) and
the rest of the train chain in ONE launch (mmvqa_aug_train_fused), no host sync.  run_packed(..., views=2) is SupCon's
TwoCropTransform: both views of every image from one resize, in one launch (mmvqa_aug_train_fused_views).
"""
from __future__ import annotations

import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib as L


# --------------------------------------------------------------------------- geometry helpers (torchvision semantics)
def resized_size(w, h, size):
    """transforms.Resize(int): the shorter side becomes `size`, the other int(size * long / short)"""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = size, int(size * long / short)
    return (new_short, new_long) if w <= h else (new_long, new_short)


def center_crop_offset(w, h, size):
    """transforms.CenterCrop: int(round((dim - size) / 2.0)) (Python's round-half-to-even)"""
    return int(round((w - size) / 2.0)), int(round((h - size) / 2.0))


def sample_params(n, size=224, scale=(0.95, 1.05), ratio=(0.95, 1.05), degrees=5.0,
                  jitter=(0.05, 0.05, 0.05, 0.05), generator=None):
    """Per-image random parameters in the order torchvision's Compose draws them:
    RandomResizedCrop.get_params -> RandomRotation.get_params -> ColorJitter.get_params."""
    g = generator

    def uni(a, b):
        return torch.empty(1).uniform_(a, b, generator=g).item()

    out = []
    for _ in range(n):
        height = width = size
        area = height * width
        log_ratio = torch.log(torch.tensor(ratio))
        box = None
        for _try in range(10):
            target_area = area * uni(scale[0], scale[1])
            aspect = math.exp(uni(float(log_ratio[0]), float(log_ratio[1])))
            w = int(round(math.sqrt(target_area * aspect)))
            h = int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= width and 0 < h <= height:
                i = int(torch.randint(0, height - h + 1, size=(1,), generator=g).item())
                j = int(torch.randint(0, width - w + 1, size=(1,), generator=g).item())
                box = (i, j, h, w)
                break
        if box is None:   # fallback: central crop
            in_ratio = float(width) / float(height)
            if in_ratio < min(ratio):
                w = width
                h = int(round(w / min(ratio)))
            elif in_ratio > max(ratio):
                h = height
                w = int(round(h * max(ratio)))
            else:
                w, h = width, height
            box = ((height - h) // 2, (width - w) // 2, h, w)
        angle = float(uni(-float(degrees), float(degrees)))
        order = torch.randperm(4, generator=g).tolist()
        b = float(uni(max(0.0, 1 - jitter[0]), 1 + jitter[0]))
        c = float(uni(max(0.0, 1 - jitter[1]), 1 + jitter[1]))
        s = float(uni(max(0.0, 1 - jitter[2]), 1 + jitter[2]))
        hh = float(uni(-jitter[3], jitter[3]))
        out.append(dict(box=box, angle=angle, order=order, brightness=b, contrast=c, saturation=s, hue=hh))
    return out


def hue_shift_u8(hue_factor):
    """torchvision F_pil.adjust_hue: np_h += np.array(hue_factor * 255).astype("uint8") (uint8 wrap-around)"""
    with np.errstate(invalid="ignore"):
        return int(np.array(np.int64(hue_factor * 255)).astype("uint8"))


def rotate_fix(angle, w, h):
    """Image.rotate's matrix (PIL/Image.py) turned into the 16.16 coefficients of Geometry.c affine_fixed"""
    angle = angle % 360.0
    cx, cy = w / 2.0, h / 2.0
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]
    m[2] = m[0] * (-cx) + m[1] * (-cy) + m[2]
    m[5] = m[3] * (-cx) + m[4] * (-cy) + m[5]
    m[2] += cx
    m[5] += cy
    if angle == 0:
        m = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0]      # Image.rotate returns a copy

    def fix(v):
        v = v * 65536.0 + 0.5
        return int(v) if v >= 0 else int(math.floor(v))

    return [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]


def coeffs(in_size, in0, in1, out_size):
    """(bounds [out][2] int32, kk [out][ksize] int32, ksize) from the library's HOST routine"""
    lib = L.lib()
    ks = lib.mmvqa_resample_coeffs(in_size, float(in0), float(in1), out_size, None, None, 0)
    if ks <= 0:
        L.check(ks)
    b = np.zeros((out_size, 2), np.int32)
    k = np.zeros((out_size, ks), np.int32)
    r = lib.mmvqa_resample_coeffs(in_size, float(in0), float(in1), out_size, b.ctypes.data_as(C.c_void_p),
                                  k.ctypes.data_as(C.c_void_p), ks)
    if r != ks:
        L.check(r if r < 0 else -1)
    return b, k, ks


@functools.lru_cache(maxsize=4096)
def _coeffs_cached(in_size, out_size):
    b, k, ks = coeffs(in_size, 0, in_size, out_size)
    b.setflags(write=False)
    k.setflags(write=False)
    return b, k, ks


def _window_rows(vb, oy, S):
    """rows [ty0, ty0 + tyn) of the box that the vertical pass of output rows [oy, oy + S) reads"""
    w = vb[oy:oy + S]
    ty0 = int(w[:, 0].min())
    return ty0, int((w[:, 0] + w[:, 1]).max()) - ty0


class _Pack:
    """host-side builder of one int32 table blob + job array, uploaded with two copies per stage"""

    def __init__(self):
        self.tabs, self.n = [], 0

    def add(self, arr):
        a = np.ascontiguousarray(arr, np.int32).reshape(-1)
        off = self.n
        self.tabs.append(a)
        self.n += a.size
        return off

    def upload(self, dev):
        blob = np.concatenate(self.tabs) if self.tabs else np.zeros(1, np.int32)
        return torch.from_numpy(blob).to(dev)


class DeviceAugment:
    def __init__(self, size=224, train=True, scale=(0.95, 1.05), ratio=(0.95, 1.05), degrees=5.0,
                 jitter=(0.05, 0.05, 0.05, 0.05), mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), device="cuda"):
        self.size, self.train = int(size), bool(train)
        self.scale, self.ratio, self.degrees, self.jitter = tuple(scale), tuple(ratio), float(degrees), tuple(jitter)
        self.mean = (C.c_float * 3)(*mean)
        self.std = (C.c_float * 3)(*std)
        self.dev = torch.device(device)

    # ---- one resample stage: list of (src_ptr, sh, sw, box(x,y,w,h), (rw,rh), (ox,oy)) -> uint8 [B,S,S,3]
    def _resample(self, specs):
        S, dev, lib = self.size, self.dev, L.lib()
        B = len(specs)
        pack, metas = _Pack(), []
        cache = {}
        for (_src, _sh, _sw, (bx, by, bw, bh), (rw, rh), (ox, oy)) in specs:
            kh = ("h", bw, rw)
            if kh not in cache:
                b, k, ks = coeffs(bw, 0, bw, rw)
                cache[kh] = (pack.add(b), pack.add(k), ks, b)
            kv = ("v", bh, rh)
            if kv not in cache:
                b, k, ks = coeffs(bh, 0, bh, rh)
                cache[kv] = (pack.add(b), pack.add(k), ks, b)
            vb = cache[kv][3][oy:oy + S]
            ty0 = int(vb[:, 0].min())
            tyn = int((vb[:, 0] + vb[:, 1]).max()) - ty0
            metas.append((cache[kh], cache[kv], ty0, tyn))
        tabs = pack.upload(dev)
        max_rows = max(m[3] for m in metas)
        tmp = torch.empty(B, max_rows, S, 3, dtype=torch.uint8, device=dev)
        dst = torch.empty(B, S, S, 3, dtype=torch.uint8, device=dev)
        jobs = (L.ResampleJob * B)()
        base = tabs.data_ptr()
        for n, ((src, sh, sw, (bx, by, bw, bh), (rw, rh), (ox, oy)), (ch, cv, ty0, tyn)) in enumerate(zip(specs, metas)):
            j = jobs[n]
            j.src, j.sh, j.sw, j.spitch = src, sh, sw, sw * 3
            j.bx, j.by, j.bw, j.bh, j.rw, j.rh, j.ox, j.oy, j.ty0, j.tyn = bx, by, bw, bh, rw, rh, ox, oy, ty0, tyn
            j.tmp = tmp[n].data_ptr()
            j.dst, j.dpitch = dst[n].data_ptr(), S * 3
            j.hb, j.hk, j.hks = base + 4 * ch[0], base + 4 * ch[1], ch[2]
            j.vb, j.vk, j.vks = base + 4 * cv[0], base + 4 * cv[1], cv[2]
        jobs_dev = torch.frombuffer(bytearray(bytes(jobs)), dtype=torch.uint8).to(dev)
        L.check(lib.mmvqa_aug_resample(L.stream_ptr(), L.ptr(jobs_dev), B, max_rows, S, S))
        self._keep = (tabs, tmp, jobs_dev)     # alive until the stream has consumed them (next call replaces them)
        return dst

    def __call__(self, images, params=None, generator=None):
        """images: list of uint8 [H, W, 3] numpy arrays / CPU tensors (decoded RGB).  Returns fp32 [B, 3, S, S]."""
        if self.dev.type != "cuda":
            raise L.MMVQAError("DeviceAugment runs on the GPU only (no CPU fallback)")
        S, dev, lib = self.size, self.dev, L.lib()
        B = len(images)
        arrs = [np.ascontiguousarray(im.numpy() if isinstance(im, torch.Tensor) else im, dtype=np.uint8) for im in images]
        for a in arrs:
            if a.ndim != 3 or a.shape[2] != 3:
                raise ValueError("images must be uint8 [H, W, 3]")
        offs = np.cumsum([0] + [a.size for a in arrs])
        host = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs]))
        src = host.to(dev, non_blocking=False)            # the one host->device copy of the batch
        specs = []
        for n, a in enumerate(arrs):
            h, w = a.shape[:2]
            rw, rh = resized_size(w, h, S)
            ox, oy = center_crop_offset(rw, rh, S)
            specs.append((src.data_ptr() + int(offs[n]), h, w, (0, 0, w, h), (rw, rh), (ox, oy)))
        a0 = self._resample(specs)                         # Resize(S) + CenterCrop(S)
        keep = [self._keep, src]
        if self.train:
            if params is None:
                params = sample_params(B, S, self.scale, self.ratio, self.degrees, self.jitter, generator)
            specs = [(a0[n].data_ptr(), S, S, (p["box"][1], p["box"][0], p["box"][3], p["box"][2]), (S, S), (0, 0))
                     for n, p in enumerate(params)]
            a1 = self._resample(specs)                     # RandomResizedCrop
            keep.append(self._keep)
            fix = torch.tensor([rotate_fix(p["angle"], S, S) for p in params], dtype=torch.int32).to(dev)
            a2 = torch.empty_like(a1)
            L.check(lib.mmvqa_aug_rotate(L.stream_ptr(), L.ptr(a1), L.ptr(a2), L.ptr(fix), B, S, S))
            if getattr(self, "debug", False):
                self.stages = dict(resize_crop=a0.clone(), resized_crop=a1.clone(), rotate=a2.clone())
            lsum = torch.zeros(B, dtype=torch.int64, device=dev)
            for rnd in range(4):                           # ColorJitter: image b applies its rnd-th op of the permutation
                ops = [p["order"][rnd] for p in params]
                fac = [(p["brightness"], p["contrast"], p["saturation"], float(hue_shift_u8(p["hue"])))[o]
                       for o, p in zip(ops, params)]
                op_d = torch.tensor(ops, dtype=torch.int32).to(dev)
                fac_d = torch.tensor(fac, dtype=torch.float32).to(dev)
                L.check(lib.mmvqa_aug_jitter_round(L.stream_ptr(), L.ptr(a2), L.ptr(op_d), L.ptr(fac_d), L.ptr(lsum), B, S * S))
                keep += [op_d, fac_d]
            final = a2
            keep += [a0, a1, fix, lsum]
        else:
            final = a0
        out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
        L.check(lib.mmvqa_aug_to_tensor(L.stream_ptr(), L.ptr(final), L.ptr(out), B, S * S, self.mean, self.std))
        self._keep_all = keep + [final]
        self.last_uint8 = final                             # [B, S, S, 3] after the last byte-valued stage (tests)
        return out

    def fused_fits(self):
        """whether the library's one-launch train chain takes S x S images on this device (asked once per device)"""
        key = (self.dev.index if self.dev.index is not None else torch.cuda.current_device(), self.size)
        if key not in _FUSED_FITS:
            with torch.cuda.device(key[0]):
                rc = L.lib().mmvqa_aug_train_fused_fits(self.size)
            if rc < 0:
                L.check(rc)
            _FUSED_FITS[key] = bool(rc)
        return _FUSED_FITS[key]

    # ---- non-blocking entry point (training loops): ragged device batch in, work enqueued on `stream` only
    def run_packed(self, src_dev, offsets, shapes, params=None, stream=None, fused=True, out=None, generator=None,
                   views=1):
        """src_dev: uint8 device tensor holding B decoded RGB images back to back, image n = [h_n, w_n, 3] at byte
        offsets[n]; shapes: [B, 2] (h, w).  Enqueues Resize+CenterCrop and, for training, the rest of the chain on
        `stream` (default: the current stream) and returns fp32 [B, 3, S, S] (`out`, if given, is filled).  No host
        sync: everything the kernels read (coefficient tables, jobs, records) goes up as ONE pinned blob with one async
        copy.  fused=False runs the multi-launch stages of __call__ instead (the reference the tests compare with); they
        also run when S x S images do not fit the device's LDS (fused_fits(), decided before anything is packed).
        last_uint8 is the last byte stage.

        views=V (training only) runs the random part of the chain V times per image, as SupCon's TwoCropTransform
        does: Resize+CenterCrop once per image, then RandomResizedCrop -> ... -> Normalize on each view, fused into
        one launch (mmvqa_aug_train_fused_views, which only reads the resized image).  params then holds V * B sets in
        the reference's draw order, params[n * V + v] = view v of image n, i.e. sample_params(V * B, ...): consecutive
        sets are the V calls of TwoCropTransform on one image.  The output is view-major, row v * B + n = view v of
        image n (process_tensors' layout): out [V * B, 3, S, S], last_uint8 [V * B, S, S, 3]."""
        if self.dev.type != "cuda":
            raise L.MMVQAError("DeviceAugment runs on the GPU only (no CPU fallback)")
        S, lib = self.size, L.lib()
        shapes = [(int(h), int(w)) for h, w in (shapes.tolist() if isinstance(shapes, torch.Tensor) else shapes)]
        offsets = [int(o) for o in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
        B, V = len(shapes), int(views)
        if V < 1 or (V > 1 and not self.train):
            raise ValueError(f"run_packed: views = {views}: need >= 1, and more than one only for training")
        R = V * B                                           # output rows: view v of image n is row v * B + n
        if B == 0 or len(offsets) != B:
            raise ValueError("run_packed: need one offset per image and at least one image")
        if src_dev.dtype != torch.uint8 or src_dev.device.type != "cuda" or not src_dev.is_contiguous():
            raise ValueError("run_packed: src_dev must be a contiguous uint8 tensor on the GPU")
        for o, (h, w) in zip(offsets, shapes):
            if h <= 0 or w <= 0 or o < 0 or o + h * w * 3 > src_dev.numel():
                raise ValueError(f"run_packed: image ({h}, {w}) at offset {o} lies outside the {src_dev.numel()}-byte batch")
        if self.train:
            if params is None:
                params = sample_params(R, S, self.scale, self.ratio, self.degrees, self.jitter, generator)
            if len(params) != R:
                raise ValueError("run_packed: one parameter set per image and view")
            for p in params:
                i, j, h, w = p["box"]
                if not (0 <= i and 0 <= j and 0 < h and 0 < w and i + h <= S and j + w <= S):
                    raise ValueError(f"run_packed: crop box {p['box']} outside the {S}x{S} image")
        stream = stream if stream is not None else torch.cuda.current_stream(self.dev)
        use_fused = self.train and fused and self.fused_fits()
        rows = params if V == 1 or not self.train else [params[n * V + v] for v in range(V) for n in range(B)]
        with torch.cuda.stream(stream):
            pack = _Pack()
            tabs = {}

            def tab(n_in, n_out):
                if (n_in, n_out) not in tabs:
                    b, k, ks = _coeffs_cached(n_in, n_out)
                    tabs[(n_in, n_out)] = (pack.add(b), pack.add(k), ks, b)
                return tabs[(n_in, n_out)]

            st1 = []                                        # Resize(S) + CenterCrop(S) of the ragged sources
            for (h, w) in shapes:
                rw, rh = resized_size(w, h, S)
                ox, oy = center_crop_offset(rw, rh, S)
                ch, cv = tab(w, rw), tab(h, rh)
                st1.append((h, w, rw, rh, ox, oy, ch, cv) + _window_rows(cv[3], oy, S))
            st2 = []                                        # RandomResizedCrop box -> (S, S)
            for p in (rows if self.train else []):
                i, j, h, w = p["box"]
                ch, cv = tab(w, S), tab(h, S)
                st2.append((j, i, w, h, ch, cv) + _window_rows(cv[3], 0, S))
            tables = np.concatenate(pack.tabs)
            njob = C.sizeof(L.ResampleJob)
            lay = {}

            def put(name, nbytes):
                lay[name] = -(-sum_n[0] // 16) * 16
                sum_n[0] = lay[name] + nbytes

            sum_n = [0]
            put("tables", tables.nbytes)
            put("jobs1", B * njob)
            if use_fused:
                put("recs", R * C.sizeof(L.AugRecord))
            elif self.train:
                put("jobs2", R * njob)
                put("fix", R * 6 * 4)
                put("ops", 4 * R * 4)
                put("facs", 4 * R * 4)
            blob = torch.empty(sum_n[0], dtype=torch.uint8, device=self.dev)
            base = blob.data_ptr()
            rows1 = max(m[-1] for m in st1)
            tmp1 = torch.empty(B, rows1, S, 3, dtype=torch.uint8, device=self.dev)
            a0 = torch.empty(B, S, S, 3, dtype=torch.uint8, device=self.dev)
            if out is None:
                out = torch.empty(R, 3, S, S, dtype=torch.float32, device=self.dev)
            elif out.shape != (R, 3, S, S) or out.dtype != torch.float32 or not out.is_contiguous() or out.device != a0.device:
                raise ValueError("run_packed: out must be a contiguous fp32 [views * B, 3, S, S] tensor on the device")
            tb = base + lay["tables"]

            def job(jb, src, sh, sw, box, rsz, off, ch, cv, ty0, tyn, tmp, dst):
                jb.src, jb.sh, jb.sw, jb.spitch = src, sh, sw, sw * 3
                (jb.bx, jb.by, jb.bw, jb.bh), (jb.rw, jb.rh), (jb.ox, jb.oy) = box, rsz, off
                jb.ty0, jb.tyn, jb.tmp, jb.dst, jb.dpitch = ty0, tyn, tmp, dst, S * 3
                jb.hb, jb.hk, jb.hks = tb + 4 * ch[0], tb + 4 * ch[1], ch[2]
                jb.vb, jb.vk, jb.vks = tb + 4 * cv[0], tb + 4 * cv[1], cv[2]

            jobs1 = (L.ResampleJob * B)()
            for n, (h, w, rw, rh, ox, oy, ch, cv, ty0, tyn) in enumerate(st1):
                job(jobs1[n], src_dev.data_ptr() + offsets[n], h, w, (0, 0, w, h), (rw, rh), (ox, oy), ch, cv, ty0, tyn,
                    tmp1[n].data_ptr(), a0[n].data_ptr())
            host = torch.empty(sum_n[0], dtype=torch.uint8, pin_memory=True)
            hv = host.numpy()
            hv[lay["tables"]:lay["tables"] + tables.nbytes] = tables.view(np.uint8)

            def emit(name, obj):
                raw = np.frombuffer(bytes(obj), np.uint8) if not isinstance(obj, np.ndarray) else obj.reshape(-1).view(np.uint8)
                hv[lay[name]:lay[name] + raw.size] = raw

            emit("jobs1", jobs1)
            keep = [blob, tmp1, a0]
            if use_fused:
                recs = (L.AugRecord * R)()
                for n, (p, (bx, by, bw, bh, ch, cv, ty0, tyn)) in enumerate(zip(rows, st2)):
                    r = recs[n]
                    r.bx, r.by, r.bw, r.bh, r.ty0, r.tyn = bx, by, bw, bh, ty0, tyn
                    r.hb, r.hk, r.hks, r.vb, r.vk, r.vks = ch[0], ch[1], ch[2], cv[0], cv[1], cv[2]
                    r.fix[:] = rotate_fix(p["angle"], S, S)
                    r.op[:] = list(p["order"])
                    r.factor[:] = [_factor(p, o) for o in p["order"]]
                emit("recs", recs)
                if V > 1:                                   # the views' scratch: a0 stays the read-only source
                    scratch = torch.empty(R, S, S, 3, dtype=torch.uint8, device=self.dev)
                    keep.append(scratch)
            elif self.train:
                rows2 = max(m[-1] for m in st2)
                tmp2 = torch.empty(R, rows2, S, 3, dtype=torch.uint8, device=self.dev)
                a1 = torch.empty(R, S, S, 3, dtype=torch.uint8, device=self.dev)
                a2 = torch.empty_like(a1)
                lsum = torch.empty(R, dtype=torch.int64, device=self.dev)
                jobs2 = (L.ResampleJob * R)()
                for n, (bx, by, bw, bh, ch, cv, ty0, tyn) in enumerate(st2):    # row n reads image n % B of a0
                    job(jobs2[n], a0[n % B].data_ptr(), S, S, (bx, by, bw, bh), (S, S), (0, 0), ch, cv, ty0, tyn,
                        tmp2[n].data_ptr(), a1[n].data_ptr())
                emit("jobs2", jobs2)
                emit("fix", np.array([rotate_fix(p["angle"], S, S) for p in rows], np.int32))
                emit("ops", np.array([[p["order"][r] for p in rows] for r in range(4)], np.int32))
                emit("facs", np.array([[_factor(p, p["order"][r]) for p in rows] for r in range(4)], np.float32))
                keep += [tmp2, a1, a2, lsum]
            blob.copy_(host, non_blocking=True)             # the one upload (the pinned block is held until it is done)
            sp = C.c_void_p(stream.cuda_stream)
            L.check(lib.mmvqa_aug_resample(sp, C.c_void_p(base + lay["jobs1"]), B, rows1, S, S))
            final = a0
            if use_fused and V == 1:
                L.check(lib.mmvqa_aug_train_fused(sp, L.ptr(a0), L.ptr(out), C.c_void_p(base + lay["recs"]),
                                                  C.c_void_p(tb), B, S, self.mean, self.std))
            elif use_fused:
                L.check(lib.mmvqa_aug_train_fused_views(sp, L.ptr(a0), L.ptr(scratch), L.ptr(out),
                                                        C.c_void_p(base + lay["recs"]), C.c_void_p(tb), B, V, S,
                                                        self.mean, self.std))
                final = scratch
            elif self.train:
                L.check(lib.mmvqa_aug_resample(sp, C.c_void_p(base + lay["jobs2"]), R, rows2, S, S))
                L.check(lib.mmvqa_aug_rotate(sp, L.ptr(a1), L.ptr(a2), C.c_void_p(base + lay["fix"]), R, S, S))
                for r in range(4):
                    L.check(lib.mmvqa_aug_jitter_round(sp, L.ptr(a2), C.c_void_p(base + lay["ops"] + 4 * R * r),
                                                       C.c_void_p(base + lay["facs"] + 4 * R * r), L.ptr(lsum), R, S * S))
                final = a2
            if not use_fused:
                L.check(lib.mmvqa_aug_to_tensor(sp, L.ptr(final), L.ptr(out), R, S * S, self.mean, self.std))
        # Every buffer above was allocated on `stream` and is used on it only, so the caching allocator may hand its
        # block out again as soon as it is freed: later work on `stream` is ordered after these launches.
        self.last_fused = use_fused
        self.last_uint8 = final                             # [V * B, S, S, 3] after the last byte-valued stage (tests)
        self.last_resized = a0       # [B, S, S, 3] Resize + CenterCrop (tests; the one-view fused launch overwrites it)
        self._packed_keep = keep
        return out


_FUSED_FITS = {}      # (device index, S) -> mmvqa_aug_train_fused_fits


def _factor(p, op):
    """the factor a ColorJitter round of op `op` applies (hue: the uint8 shift, as the kernels take it)"""
    return (p["brightness"], p["contrast"], p["saturation"], float(hue_shift_u8(p["hue"])))[op]
