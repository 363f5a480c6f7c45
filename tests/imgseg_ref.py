"""NumPy restatements of the two resizes of the image-segmentation tool (``test_image_seg.py:44-64``, ``:95-124``), each taking
explicit parameters.  A helper for tests/test_image_seg_device_*.py, not a test.

``np_resize_bilinear``   Pillow's ``Image.resize((w, h), Image.BILINEAR)`` on uint8 RGB: libImaging/Resample.c's 8-bit path
                         restated as its C loops (the tables in Python floats = C doubles, the passes in integers).
``np_norm``              ToTensor + Normalize in float32.
``np_upsample_round``    the rule of ``vfn_imgseg_upsample_round`` (include/vfn_hip.h) in float32, operation by operation.
``bilinear64``           the same interpolation in float64 (for the near-tie band around 0.5).
"""
import math
import os

import numpy as np

f32 = np.float32
MEAN = np.array([0.485, 0.456, 0.406], f32)
STD = np.array([0.229, 0.224, 0.225], f32)
TAU = 2.0 ** -13          # see ``in_band``
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'image_seg_c1.npz')


def bilinear_coeffs(n_in, n_out):
    """``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the triangle filter (support 1), in0 = 0, in1 = n_in:
    (bounds [(xmin, count)], integer coefficients [[...]], ksize)."""
    scale = filterscale = n_in / n_out
    if filterscale < 1.0:
        filterscale = 1.0
    support = 1.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds, kk = [], []
    for xx in range(n_out):
        center = 0.0 + (xx + 0.5) * scale
        ww = 0.0
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > n_in:
            xmax = n_in
        xmax -= xmin
        k = []
        for x in range(xmax):
            t = (x + xmin - center + 0.5) * ss
            if t < 0.0:
                t = -t
            w = 1.0 - t if t < 1.0 else 0.0
            k.append(w)
            ww += w
        for x in range(xmax):
            if ww != 0.0:
                k[x] /= ww
        k += [0.0] * (ksize - xmax)
        kk.append([int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in k])
        bounds.append((xmin, xmax))
    return bounds, kk, ksize


def _pass(a, n_out, axis):
    """One resampling pass of uint8 [H, W, 3] along ``axis`` (0 vertical, 1 horizontal)."""
    n_in = a.shape[axis]
    bounds, kk, _ = bilinear_coeffs(n_in, n_out)
    src = np.moveaxis(a, axis, 0).astype(np.int64)
    out = np.empty((n_out,) + src.shape[1:], np.uint8)
    for o, ((lo, n), k) in enumerate(zip(bounds, kk)):
        s = np.full(src.shape[1:], 1 << 21, np.int64)
        for q in range(n):
            s += k[q] * src[lo + q]
        out[o] = np.clip(s >> 22, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, axis))


def np_resize_bilinear(a, h, w):
    """uint8 [H, W, 3] -> uint8 [h, w, 3]: the horizontal pass, rounded to uint8, then the vertical one; a pass whose size does
    not change is skipped."""
    a = np.ascontiguousarray(a)
    if a.shape[1] != w:
        a = _pass(a, w, 1)
    if a.shape[0] != h:
        a = _pass(a, h, 0)
    return a


def np_norm(u8):
    """uint8 [h, w, 3] -> float32 [3, h, w] = (float(u8) / 255 - mean) / std, every operation in float32."""
    t = u8.transpose(2, 0, 1).astype(f32) / f32(255.0)
    return (t - MEAN[:, None, None]) / STD[:, None, None]


def _axis(n_in, n_out):
    s = f32(n_in) / f32(n_out)
    f = np.maximum(s * (np.arange(n_out).astype(f32) + f32(0.5)) - f32(0.5), f32(0.0))
    i0 = f.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1)
    w1 = f - i0.astype(f32)
    w0 = f32(1.0) - w1
    assert f.dtype == w1.dtype == w0.dtype == f32
    return i0, i1, w0, w1


def np_upsample_value(p, H, W):
    """float32 [h, w] -> float32 [H, W]: the value ``vfn_imgseg_upsample_round`` rounds."""
    p = np.ascontiguousarray(p, f32)
    y0, y1, wy0, wy1 = _axis(p.shape[0], H)
    x0, x1, wx0, wx1 = _axis(p.shape[1], W)
    a = wx0[None, :] * p[y0][:, x0] + wx1[None, :] * p[y0][:, x1]
    b = wx0[None, :] * p[y1][:, x0] + wx1[None, :] * p[y1][:, x1]
    v = wy0[:, None] * a + wy1[:, None] * b
    assert v.dtype == f32
    return v


def np_upsample_round(p, H, W):
    """-> uint8 [H, W] labels: rint (halves to even) of the value clamped to [0, 255]."""
    return np.rint(np.clip(np_upsample_value(p, H, W), f32(0.0), f32(255.0))).astype(np.uint8)


def bilinear64(p, H, W):
    """The same interpolation with the coordinates, weights and sums in float64."""
    p = np.asarray(p, np.float64)

    def axis(n_in, n_out):
        f = np.maximum((n_in / n_out) * (np.arange(n_out) + 0.5) - 0.5, 0.0)
        i0 = f.astype(np.int64)
        return i0, i0 + (i0 < n_in - 1), f - i0
    y0, y1, ly = axis(p.shape[0], H)
    x0, x1, lx = axis(p.shape[1], W)
    a = (1 - lx)[None, :] * p[y0][:, x0] + lx[None, :] * p[y0][:, x1]
    b = (1 - lx)[None, :] * p[y1][:, x0] + lx[None, :] * p[y1][:, x1]
    return (1 - ly)[:, None] * a + ly[:, None] * b


def in_band(p, H, W):
    """bool [H, W]: the pixels where two correct float32 evaluations of the enlargement may round to different labels,
    |v - 0.5| <= TAU with v in float64.  TAU = 2^-13: a source coordinate below 512 is a float32 with an ulp of at most 2^-15
    after one product and one difference each rounded to half an ulp of a number below 512 (2^-15 each), i.e. at most 2^-14 of
    error in the fractional weight per axis; the values lie in [0, 1], so the two axes move v by at most 2 * 2^-14 = 2^-13 (the
    roundings of the products and sums themselves are 2^-24 each and vanish beside it)."""
    assert max(p.shape) <= 512
    return np.abs(bilinear64(p, H, W) - 0.5) <= TAU


# ------------------------------------------------------------------------------------------------ shared cases
# (H, W) -> (h, w): both axes down by non-integer factors, both up, one axis unchanged (each way), a 1-pixel-wide source
RESIZE_CASES = [((95, 131), (32, 64)), ((20, 24), (32, 64)), ((40, 64), (32, 64)), ((32, 100), (32, 64)), ((37, 1), (32, 64))]


def photo(seed, H, W):
    """A uint8 RGB image with smooth structure and noise (so that rounding after the horizontal pass matters)."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([127 + 120 * np.sin(xx / 7.0 + c) * np.cos(yy / 5.0 - c) for c in range(3)], -1)
    return np.clip(base + g.integers(-40, 41, (H, W, 3)), 0, 255).astype(np.uint8)


def standin_prob(name):
    """The stand-in's probability map [416, 416] for a golden frame, and the photograph's size."""
    import torch
    from PIL import Image
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    from tools import synth
    from tools.standin import StandIn
    g = np.load(GOLD)
    seed, H, W = [int(x) for x in g[f'{name}_seed_hw']]
    frames, _ = synth.clip(seed, 1, H, W)
    u8 = (frames[0] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    x = image_seg.norm_imagenet(Image.fromarray(u8), (416, 416)).unsqueeze(0)
    return StandIn().predict(x)[0, 0].numpy(), H, W


def smooth_map(seed, h, w):
    import torch
    g = torch.Generator().manual_seed(seed)
    z = torch.nn.functional.avg_pool2d(torch.randn(1, 1, h + 4, w + 4, generator=g), 5, 1)
    return torch.sigmoid(6.0 * z)[0, 0].contiguous().numpy()
