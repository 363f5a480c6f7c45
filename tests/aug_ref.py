"""Two forms of every operation of the training augmentation (``video_module/dataset/Water_DS.py:53-83``), each taking
explicit parameters: ``pil_*`` calls Pillow the way torchvision's PIL back end does, ``np_*`` restates Pillow's C arithmetic
in NumPy (integers, float32 and float64 where the C code uses them).  A helper for tests/test_train_aug_*.py, not a test.

Images are uint8 [H, W, 3] (RGB) or uint8 [H, W] (palette indices).
"""
import math
import os

import numpy as np
from PIL import Image, ImageEnhance

f32 = np.float32


# ======================================================================================================== Pillow
def _img(a):
    return Image.fromarray(np.ascontiguousarray(a), 'RGB' if a.ndim == 3 else 'P')


def pil_hflip(a):
    return np.array(_img(a).transpose(Image.FLIP_LEFT_RIGHT))


def pil_brightness(a, factor):
    return np.array(ImageEnhance.Brightness(_img(a)).enhance(factor))


def pil_contrast(a, factor):
    return np.array(ImageEnhance.Contrast(_img(a)).enhance(factor))


def pil_saturation(a, factor):
    return np.array(ImageEnhance.Color(_img(a)).enhance(factor))


def pil_rgb2hsv(a):
    return np.array(_img(a).convert('HSV'))


def pil_hsv2rgb(a):
    return np.array(Image.fromarray(np.ascontiguousarray(a), 'HSV').convert('RGB'))


def pil_hue(a, hue_factor):
    """torchvision ``adjust_hue`` on a PIL image."""
    h, s, v = _img(a).convert('HSV').split()
    np_h = np.array(h, dtype=np.uint8)
    with np.errstate(over='ignore'):
        np_h += np.array(int(hue_factor * 255)).astype(np.uint8)
    return np.array(Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB'))


def pil_affine(a, matrix, resample):
    """``Image.transform(size, AFFINE, matrix, resample, fillcolor=0)``; resample 'bicubic' or 'nearest'."""
    im = _img(a)
    rs = Image.BICUBIC if resample == 'bicubic' else Image.NEAREST
    return np.array(im.transform(im.size, Image.AFFINE, tuple(float(v) for v in matrix), rs, fillcolor=0))


def pil_crop_resize(a, i, j, h, w, S, resample):
    """torchvision ``resized_crop``: ``crop((j, i, j + w, i + h)).resize((S, S), resample)``."""
    rs = Image.BICUBIC if resample == 'bicubic' else Image.NEAREST
    return np.array(_img(a).crop((j, i, j + w, i + h)).resize((S, S), rs))


# ======================================================================================================== the matrix
def inverse_affine_matrix(W, H, angle, translate, scale, shear_x):
    """torchvision ``_get_inverse_affine_matrix`` with centre (W * 0.5, H * 0.5) and shear (shear_x, 0), in Python floats."""
    cx, cy = W * 0.5, H * 0.5
    tx, ty = float(translate[0]), float(translate[1])
    rot, sx, sy = math.radians(angle), math.radians(shear_x), math.radians(0.0)
    a = math.cos(rot - sy) / math.cos(sy)
    b = -math.cos(rot - sy) * math.tan(sx) / math.cos(sy) - math.sin(rot)
    c = math.sin(rot - sy) / math.cos(sy)
    d = -math.sin(rot - sy) * math.tan(sx) / math.cos(sy) + math.cos(rot)
    m = [d, -b, 0.0, -c, a, 0.0]
    m = [x / scale for x in m]
    m[2] += m[0] * (-cx - tx) + m[1] * (-cy - ty)
    m[5] += m[3] * (-cx - tx) + m[4] * (-cy - ty)
    m[2] += cx
    m[5] += cy
    return m


# ======================================================================================================== NumPy
def np_hflip(a):
    return np.ascontiguousarray(a[:, ::-1])


def np_L(a):
    r, g, b = (a[..., k].astype(np.int64) for k in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def np_blend(deg, img, alpha):
    """``ImagingBlend(degenerate, image, alpha)``: float32 throughout."""
    alpha = f32(alpha)
    if alpha == f32(1.0):
        return img.copy()
    d = np.broadcast_to(deg, img.shape).astype(np.int32)
    t = d.astype(f32) + alpha * (img.astype(np.int32) - d).astype(f32)
    if f32(0.0) <= alpha <= f32(1.0):
        return t.astype(np.int32).astype(np.uint8)
    out = t.astype(np.int32)                           # truncation
    out[t <= 0] = 0
    out[t >= 255] = 255
    return out.astype(np.uint8)


def np_brightness(a, factor):
    return np_blend(np.uint8(0), a, factor)


def np_contrast_mean(a):
    L = np_L(a)
    return int(float(int(L.sum(dtype=np.int64))) / float(L.size) + 0.5)


def np_contrast(a, factor):
    return np_blend(np.uint8(np_contrast_mean(a)), a, factor)


def np_saturation(a, factor):
    return np_blend(np_L(a)[..., None], a, factor)


def np_rgb2hsv(a):
    r, g, b = (a[..., k].astype(np.int32) for k in range(3))
    mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = mx == mn
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (mx - mn).astype(f32)
        s = cr / mx.astype(f32)
        rc, gc, bc = ((mx - c).astype(f32) / cr for c in (r, g, b))
        rc64, gc64, bc64 = rc.astype(np.float64), gc.astype(np.float64), bc.astype(np.float64)
        h = np.where(r == mx, bc64 - gc64, np.where(g == mx, 2.0 + rc64 - bc64, 4.0 + gc64 - rc64)).astype(f32)
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
        H = np.clip((h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip((s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H, S = np.where(grey, 0, H), np.where(grey, 0, S)
    return np.stack([H, S, mx], -1).astype(np.uint8)


def _round_away(x):
    return np.where(x >= 0, np.floor(x + 0.5), np.ceil(x - 0.5))


def np_hsv2rgb(a):
    h, s, v = (a[..., k].astype(np.float64) for k in range(3))
    i = np.floor(h * 6.0 / 255.0)
    f = (h * 6.0 / 255.0 - i).astype(f32)
    fs = (s / 255.0).astype(f32)
    f64, fs64 = f.astype(np.float64), fs.astype(np.float64)
    p = _round_away(v * (1.0 - fs64))
    q = _round_away(v * (1.0 - fs64 * f64))
    t = _round_away(v * (1.0 - fs64 * (1.0 - f64)))
    p, q, t = (np.clip(x, 0, 255) for x in (p, q, t))
    k = i.astype(np.int64) % 6
    R = np.choose(k, [v, q, p, p, t, v])
    G = np.choose(k, [t, v, v, q, p, p])
    B = np.choose(k, [p, p, t, v, v, q])
    grey = a[..., 1] == 0
    out = np.stack([np.where(grey, v, R), np.where(grey, v, G), np.where(grey, v, B)], -1)
    return out.astype(np.uint8)


def np_hue(a, shift):
    """``shift`` is the uint8 added to H: ``int(hue_factor * 255) % 256``."""
    hsv = np_rgb2hsv(a)
    hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
    return np_hsv2rgb(hsv)


def hue_shift(hue_factor):
    return int(hue_factor * 255) % 256


def _floor_c(v):
    """Pillow's FLOOR macro (toward minus infinity for negatives, truncation otherwise), as int64."""
    return np.floor(v).astype(np.int64)


def _bicubic_horner(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def np_affine_bicubic(a, m):
    """``ImagingGenericTransform`` with ``affine_transform`` and ``bicubic_filter8`` per channel, fill 0."""
    H, W = a.shape[:2]
    src = (a[:, :, None] if a.ndim == 2 else a).astype(np.float64)
    m = [float(v) for v in m]
    y, x = np.mgrid[0:H, 0:W]
    xc, yc = x + 0.5, y + 0.5
    xin = m[0] * xc + m[1] * yc + m[2]
    yin = m[3] * xc + m[4] * yc + m[5]
    outside = (xin < 0.0) | (xin >= W) | (yin < 0.0) | (yin >= H)
    xin, yin = xin - 0.5, yin - 0.5
    x0, y0 = _floor_c(xin), _floor_c(yin)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    cols = [np.clip(x0 - 1 + k, 0, W - 1) for k in range(4)]

    def row(yy):
        return _bicubic_horner(src[yy, cols[0]], src[yy, cols[1]], src[yy, cols[2]], src[yy, cols[3]], dx)
    v1 = row(np.clip(y0 - 1, 0, H - 1))
    rows = [v1]
    for k in range(3):                               # rows y0, y0 + 1, y0 + 2: outside -> the previous row's VALUE
        yy = y0 + k
        ok = ((yy >= 0) & (yy < H))[..., None]
        rows.append(np.where(ok, row(np.clip(yy, 0, H - 1)), rows[-1]))
    v = _bicubic_horner(rows[0], rows[1], rows[2], rows[3], dy)
    out = v.astype(np.int64)                         # truncation
    out[v <= 0.0] = 0
    out[v >= 255.0] = 255
    out[outside] = 0
    return out.astype(np.uint8).reshape(a.shape)


def _fix(v):
    return int(math.floor(v * 65536.0 + 0.5))


def nearest_scale_table(a0, a2, n_out, n_in):
    """``ImagingScaleAffine``'s index table: an accumulation; -1 where the source index falls outside."""
    o = a2 + a0 * 0.5
    tab = np.full(n_out, -1, np.int64)
    for k in range(n_out):
        idx = -1 if o < 0.0 else int(o)
        if 0 <= idx < n_in:
            tab[k] = idx
        o += a0
    return tab


def np_affine_nearest(a, m):
    """``ImagingTransformAffine`` with the nearest filter: the scaling path when m1 == m3 == 0, else 16.16 fixed point."""
    H, W = a.shape[:2]
    m = [float(v) for v in m]
    out = np.zeros_like(a)
    if m[1] == 0 and m[3] == 0:
        xt, yt = nearest_scale_table(m[0], m[2], W, W), nearest_scale_table(m[4], m[5], H, H)
        ok = (yt >= 0)[:, None] & (xt >= 0)[None, :]
        g = a[np.clip(yt, 0, None)[:, None], np.clip(xt, 0, None)[None, :]]
        out[ok] = g[ok]
        return out
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xx = _fix(m[2] + m[0] * 0.5 + m[1] * 0.5) + _fix(m[1]) * y + _fix(m[0]) * x
    yy = _fix(m[5] + m[3] * 0.5 + m[4] * 0.5) + _fix(m[4]) * y + _fix(m[3]) * x
    sx, sy = xx >> 16, yy >> 16
    ok = (sx >= 0) & (sx < W) & (sy >= 0) & (sy < H)
    out[ok] = a[sy[ok], sx[ok]]
    return out


def _bicubic_half(x):
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def np_resize_coeffs(n_in, n_out):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bicubic filter: (bounds [n_out, 2], k [n_out, ksize])."""
    scale = fscale = n_in / n_out
    if fscale < 1.0:
        fscale = 1.0
    support = 2.0 * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    bounds, kk = np.zeros((n_out, 2), np.int64), np.zeros((n_out, ksize), np.int64)
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        w = [_bicubic_half((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        kk[xx, :xmax] = [int(-0.5 + v * (1 << 22)) if v < 0 else int(0.5 + v * (1 << 22)) for v in w]
    return bounds, kk


def np_resize_pass(a, bounds, kk, axis):
    """One pass of ``ImagingResample`` (8 bits per channel) along ``axis`` (0: vertical, 1: horizontal)."""
    src = np.moveaxis(a.astype(np.int64), axis, 0)
    out = np.empty((len(bounds),) + src.shape[1:], np.int64)
    for o, (lo, n) in enumerate(bounds):
        k = kk[o, :n].reshape((n,) + (1,) * (src.ndim - 1))
        out[o] = ((1 << 21) + (k * src[lo:lo + n]).sum(0)) >> 22
    return np.moveaxis(np.clip(out, 0, 255).astype(np.uint8), 0, axis)


def np_crop_resize_bicubic(a, i, j, h, w, S):
    c = a[i:i + h, j:j + w]
    if w != S:
        c = np_resize_pass(c, *np_resize_coeffs(w, S), axis=1)
    if h != S:
        c = np_resize_pass(c, *np_resize_coeffs(h, S), axis=0)
    return np.ascontiguousarray(c)


def np_crop_resize_nearest(a, i, j, h, w, S):
    c = a[i:i + h, j:j + w]
    if (h, w) == (S, S):
        return np.ascontiguousarray(c)
    xt, yt = nearest_scale_table(w / S, 0.0, S, w), nearest_scale_table(h / S, 0.0, S, h)
    out = np.zeros((S, S) + a.shape[2:], a.dtype)
    ok = (yt >= 0)[:, None] & (xt >= 0)[None, :]
    g = c[np.clip(yt, 0, None)[:, None], np.clip(xt, 0, None)[None, :]]
    out[ok] = g[ok]
    return out


def np_to_tensor(a):
    """torchvision ``ToTensor``: uint8 [H, W, 3] -> float32 [3, H, W] = u8 / 255 in float32."""
    return np.ascontiguousarray(a.transpose(2, 0, 1)).astype(f32) / f32(255)


def np_onehot(mask, obj_list):
    """``ToOnehot`` with a given object list, first ``len(obj_list) + 1`` channels, float32."""
    out = np.zeros((len(obj_list) + 1,) + mask.shape, np.uint8)
    for k, o in enumerate(obj_list):
        out[k + 1] = mask == o
    out[0] = 1 - out.sum(0)
    return out.astype(f32)


JITTER_OPS = {0: 'brightness', 1: 'contrast', 2: 'saturation', 3: 'hue'}


def _frame(a, mask, p, S, flip, bri, con, sat, hue, aff_b, aff_n, crop_b, crop_n):
    if p.get('flip'):
        a, mask = flip(a), flip(mask)
    if p.get('jitter') is not None:
        order, (fb, fc, fsat, shift) = p['jitter']
        for op in order:
            fn, arg = ((bri, fb), (con, fc), (sat, fsat), (hue, shift))[op]
            a = fn(a, arg)
    if p.get('affine') is not None:
        a, mask = aff_b(a, p['affine']), aff_n(mask, p['affine'])
    i, j, h, w = p['crop']
    return crop_b(a, i, j, h, w, S), crop_n(mask, i, j, h, w, S)


def np_clip(img, mask, params, S, obj_list):
    """The composed ``np_*`` pipeline for explicit per-frame parameters: dicts with ``flip``, ``jitter`` = (order, (b, c, s,
    hue shift)) or None, ``affine`` = inverse matrix or None, ``crop`` = (i, j, h, w).  -> (frames f32 [T, 3, S, S],
    masks f32 [T, len(obj_list) + 1, S, S], resized label maps uint8 [T, S, S])."""
    fr, ms, lab = [], [], []
    for p in params:
        a, m = _frame(img, mask, p, S, np_hflip, np_brightness, np_contrast, np_saturation, np_hue,
                      np_affine_bicubic, np_affine_nearest, np_crop_resize_bicubic, np_crop_resize_nearest)
        fr.append(np_to_tensor(a))
        ms.append(np_onehot(m, obj_list))
        lab.append(m)
    return np.stack(fr), np.stack(ms), np.stack(lab)


def pil_clip(img, mask, params, S, obj_list):
    """The same pipeline through Pillow (hue takes the uint8 shift: it is applied to the H band as torchvision does)."""
    def hue(a, shift):
        hsv = pil_rgb2hsv(a)
        hsv[..., 0] = (hsv[..., 0].astype(np.int32) + int(shift)) & 255
        return pil_hsv2rgb(hsv)
    fr, ms, lab = [], [], []
    for p in params:
        a, m = _frame(img, mask, p, S, pil_hflip, pil_brightness, pil_contrast, pil_saturation, hue,
                      lambda x, mm: pil_affine(x, mm, 'bicubic'), lambda x, mm: pil_affine(x, mm, 'nearest'),
                      lambda x, *c: pil_crop_resize(x, *c, 'bicubic'), lambda x, *c: pil_crop_resize(x, *c, 'nearest'))
        fr.append(np_to_tensor(a))
        ms.append(np_onehot(m, obj_list))
        lab.append(m)
    return np.stack(fr), np.stack(ms), np.stack(lab)


# ======================================================================================================== a data set
def make_tree(root, n=3, size=(40, 30), jpg=True, seed=0):
    """A data set laid out as the reference's (Water_DS.py:25-41): one folder of n images and palette masks."""
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, 'JPEGImages', 'a'))
    os.makedirs(os.path.join(root, 'Annotations', 'a'))
    with open(os.path.join(root, 'train_imgs.txt'), 'w') as f:
        f.write('a\n')
    W, H = size
    for k in range(n):
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([(xx * 5 + k * 20) % 256, (yy * 7) % 256, (xx + yy) * 2 % 256], -1).astype(np.uint8)
        img = np.clip(img.astype(np.int32) + rng.integers(-20, 20, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'JPEGImages', 'a', f'{k:03d}.jpg' if jpg and k != 1 else f'{k:03d}.png'))
        m = np.zeros((H, W), np.uint8)
        if k != 2:                                   # image 2 has no object: obj_n == 1
            m[H // 3:, :] = 1
            m[:H // 4, W // 2:] = 2
        pm = Image.fromarray(m, 'P')
        pm.putpalette([0, 0, 0, 0, 0, 128, 0, 128, 0] + [100] * (253 * 3))
        pm.save(os.path.join(root, 'Annotations', 'a', f'{k:03d}.png'))
