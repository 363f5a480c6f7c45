"""``Water_Image_Train_DS``: the training dataset of ``video_module/dataset/Water_DS.py:14-83`` with the pixel work on the GPU
(``csrc/train_aug.hip``).

The reference builds every sample from one photograph with PIL in DataLoader workers: ``clip_n`` frames, frames 1.. flipped
(30 %), colour-jittered and warped by a random affine map, every frame cropped and resized to ``output_size``, then
``ToTensor`` and ``ToOnehot``.  Here the split is the one of ``Video_DS(decode='device')``:

* ``Water_Image_Train_DS.__getitem__`` (worker processes) reads the two files and undoes the serial part of their coding
  (JPEG entropy decoding, PNG inflate; anything outside those subsets is decoded by PIL);
* ``TrainClipLoader`` (the training process) finishes the decode on the device, draws the random parameters
  (``draw_clip_params``), builds the small coefficient / index tables Pillow would build (in double precision, exactly as
  Pillow does) and runs ``ClipAugmenter``: three stages, all frames of the clip per launch, on a side stream while the
  previous sample trains.

The kernels restate Pillow's C arithmetic operation by operation, so for given parameters the tensors equal the ones the
reference's transforms produce with Pillow 12.2.0, in every bit (tests/test_train_aug_host.py, tests/test_train_aug_gpu.py).
"""
import ctypes as C
import math
import os
import random
from glob import glob

import numpy as np
import torch
from torch.utils import data

from . import _lib
from ._lib import ptr, stream, check
from .data import load_image_in_PIL

MAX_SIDE = _lib.TRAIN_AUG_MAX_SIDE


# ====================================================================================================== the host's tables
def inverse_affine_matrix(W, H, angle, translate, scale, shear_x):
    """torchvision's ``_get_inverse_affine_matrix`` as ``TF.affine`` calls it for a PIL image: centre (W * 0.5, H * 0.5),
    angle and shear in degrees, shear (shear_x, 0).  Python floats; output pixel -> source pixel."""
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


def resize_tables(n_in, n_out, filt='bicubic'):
    """Pillow's ``precompute_coeffs`` and ``normalize_coeffs_8bpc`` (libImaging/Resample.c) for the bicubic filter (or, with
    ``filt='bilinear'``, the triangle filter of support 1: ``image_seg``), one axis:
    (bounds int32 [n_out, 2] = (first source index, count), coefficients int32 [n_out, ksize]).  Vectorised, but every
    number goes through the same double-precision operations in the same order as in the C loop (the running sum of the
    weights is a sequential ``cumsum``)."""
    scale = fscale = n_in / n_out
    if fscale < 1.0:
        fscale = 1.0
    support = (2.0 if filt == 'bicubic' else 1.0) * fscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / fscale
    center = (np.arange(n_out) + 0.5) * scale
    xmin = np.maximum((center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum((center + support + 0.5).astype(np.int64), n_in) - xmin
    x = np.arange(ksize)[None, :]
    valid = x < xmax[:, None]
    arg = np.abs(((x + xmin[:, None]) - center[:, None] + 0.5) * ss)
    a = -0.5
    if filt == 'bicubic':
        w = np.where(arg < 1.0, ((a + 2.0) * arg - (a + 3.0)) * arg * arg + 1,
                     np.where(arg < 2.0, (((arg - 5) * arg + 8) * arg - 4) * a, 0.0))
    else:
        w = np.where(arg < 1.0, 1.0 - arg, 0.0)
    w = np.where(valid, w, 0.0)
    ww = np.cumsum(w, axis=1)[:, -1:]
    w = np.where(ww != 0.0, w / np.where(ww != 0.0, ww, 1.0), w)
    kk = np.trunc(np.where(w < 0, -0.5, 0.5) + w * float(1 << 22)).astype(np.int32)
    kk[~valid] = 0
    return np.stack([xmin, xmax], 1).astype(np.int32), kk


def nearest_table(a0, a2, n_out, n_in):
    """``ImagingScaleAffine``'s index table (libImaging/Geometry.c): ``o = a2 + a0 * 0.5``, then for every output index
    ``int(o)`` and ``o += a0`` -- an accumulation, kept one (``cumsum`` adds in order).  -1 where the index is outside."""
    steps = np.full(n_out, float(a0))
    steps[0] = a2 + a0 * 0.5
    o = np.cumsum(steps)
    idx = np.where(o < 0.0, -1, np.trunc(o)).astype(np.int64)
    idx[(idx < 0) | (idx >= n_in)] = -1
    return idx.astype(np.int32)


# ====================================================================================================== the random draws
def _crop_params(rng, width, height, scale=(0.8, 1.0), ratio=(3. / 4., 4. / 3.)):
    """``RandomResizedCrop.get_params`` (transforms.py:317-358): ten tries, then the central crop."""
    area = height * width
    for _ in range(10):
        target_area = rng.uniform(*scale) * area
        log_ratio = (math.log(ratio[0]), math.log(ratio[1]))
        aspect_ratio = math.exp(rng.uniform(*log_ratio))
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if 0 < w <= width and 0 < h <= height:
            i = rng.randint(0, height - h)
            j = rng.randint(0, width - w)
            return i, j, h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w


def draw_clip_params(rng, W, H, clip_n, output_size, after_first=None):
    """The random parameters of one sample, drawn from ``rng`` (a ``random.Random``) in the order ``__getitem__`` of the
    reference consumes them (Water_DS.py:61-78): per frame i > 0 the flip (transforms.py:49), the jitter (torchvision
    ``ColorJitter.get_params``: the order of the four operations, then brightness, contrast, saturation, hue), the affine
    map (transforms.py:140-163, translations ``np.round``-ed), and for every frame the crop (:317-358).  ``after_first`` is
    called with frame 0's record right after frame 0's crop is drawn: that is where ``ToOnehot(shuffle=True)`` consumes
    randoms (``random.shuffle(obj_list)``, :413-414), which needs frame 0's resized mask.

    Stream-for-stream parity with the reference's generators is NOT claimed: torchvision draws the jitter from torch's
    generator, not from ``random``, and torchvision is no dependency of this package.  The distributions and the order are
    the reference's; the pixels, for given parameters, are Pillow's.

    -> list of ``clip_n`` dicts: ``flip`` (bool), ``jitter`` (None, or (order, (brightness, contrast, saturation, hue shift
    0..255))), ``affine`` (None, or the inverse matrix, 6 floats), ``crop`` (i, j, h, w) and ``draws`` (the raw values)."""
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError(f'source image {W} x {H}: the affine kernels take sides up to {MAX_SIDE} '
                         "(Pillow's 16.16 nearest path needs every transformed coordinate below 32768)")
    del output_size                                    # (the crop does not depend on it; kept for the reference's signature)
    out = []
    for i in range(clip_n):
        p = {'flip': False, 'jitter': None, 'affine': None, 'draws': {}}
        if i > 0:
            p['flip'] = rng.random() < 0.3
            order = list(range(4))
            rng.shuffle(order)
            b, c, s = rng.uniform(0.9, 1.1), rng.uniform(0.9, 1.1), rng.uniform(0.9, 1.1)
            hue = rng.uniform(-0.03, 0.03)
            p['jitter'] = (tuple(order), (b, c, s, int(hue * 255) % 256))
            angle = rng.uniform(-20, 20)
            max_dx, max_dy = 0.1 * W, 0.1 * H
            tr = (float(np.round(rng.uniform(-max_dx, max_dx))), float(np.round(rng.uniform(-max_dy, max_dy))))
            scale = rng.uniform(0.9, 1.1)
            shear = rng.uniform(-10, 10)
            p['affine'] = inverse_affine_matrix(W, H, angle, tr, scale, shear)
            p['draws'] = {'brightness': b, 'contrast': c, 'saturation': s, 'hue': hue, 'angle': angle, 'translate': tr,
                          'scale': scale, 'shear': shear}
        p['crop'] = _crop_params(rng, W, H)
        out.append(p)
        if i == 0 and after_first is not None:
            after_first(p)
    return out


# ====================================================================================================== the dataset (host part)
def _host_decode(path, want):
    """The serial part of a file's decoding, safe in worker processes: {'jpeg': ...} / {'png': ...} as ``Video_DS`` hands
    them out, or {'u8': ...} from PIL.  ``want``: 'RGB', or 'P' (palette PNG files only go the device way)."""
    import zlib
    with open(path, 'rb') as f:
        data_ = f.read()
    try:
        if want == 'RGB' and data_[:2] == b'\xff\xd8':
            from . import jpeg_device
            coef, qt, info = jpeg_device.entropy_decode(data_)
            return {'jpeg': (torch.from_numpy(coef), torch.from_numpy(qt.astype(np.int16)), torch.from_numpy(info))}
        if data_[:8] == b'\x89PNG\r\n\x1a\n':
            from . import png_decode
            filtered, info, pal = png_decode.inflate(data_)
            if want == 'RGB' or int(info[2]) == 3:
                return {'png': (torch.from_numpy(filtered), torch.from_numpy(info), torch.from_numpy(pal))}
    except (RuntimeError, zlib.error, ValueError):
        pass
    return {'u8': torch.from_numpy(np.array(load_image_in_PIL(path, want), np.uint8))}


class Water_Image_Train_DS(data.Dataset):
    """Water_DS.py:14-52: same constructor, file layout (``root/dataset_file`` lists the folders under ``root/JPEGImages``
    and ``root/Annotations``) and ``__len__``.  ``__getitem__`` does the host part only (see the module docstring) and
    returns ``{'img': ..., 'mask': ..., 'name': path}``; ``TrainClipLoader`` makes the reference's sample of it."""

    def __init__(self, root, output_size, dataset_file='train_imgs.txt', clip_n=3, max_obj_n=11):
        self.root = root
        self.clip_n = clip_n
        self.output_size = output_size
        self.max_obj_n = max_obj_n
        self.img_list = list()
        self.mask_list = list()
        with open(os.path.join(root, dataset_file), 'r') as lines:
            for line in lines:
                dataset_name = line.strip()
                img_dir = os.path.join(root, 'JPEGImages', dataset_name)
                mask_dir = os.path.join(root, 'Annotations', dataset_name)
                img_list = sorted(glob(os.path.join(img_dir, '*.jpg')) + glob(os.path.join(img_dir, '*.png')))
                mask_list = sorted(glob(os.path.join(mask_dir, '*.png')))
                assert len(img_list) == len(mask_list)
                self.img_list += img_list
                self.mask_list += mask_list

    def __len__(self):
        return len(self.img_list)

    def __getitem__(self, idx):
        return {'img': _host_decode(self.img_list[idx], 'RGB'), 'mask': _host_decode(self.mask_list[idx], 'P'),
                'name': self.img_list[idx]}


def _identity(batch):
    return batch[0]


# ====================================================================================================== the device part
def image_to_device(item, device):
    """{'jpeg' | 'png' | 'u8': ...} of an RGB file -> uint8 [H, W, 3] on the device (bit-identical to PIL's decode)."""
    if 'jpeg' in item:
        from . import jpeg_device
        return jpeg_device.to_tensor(*item['jpeg'], device, u8_only=True)
    if 'png' in item:
        from . import png_decode
        return png_decode.to_tensor(*item['png'], device, want_u8=True)[1]
    return item['u8'].to(device, non_blocking=True).contiguous()


def mask_to_device(item, device):
    """{'png' | 'u8': ...} of a palette file -> its indices, uint8 [H, W] on the device."""
    if 'png' in item:
        from . import png_decode
        return png_decode.palette_indices(item['png'][0], item['png'][1], device)
    return item['u8'].to(device, non_blocking=True).contiguous()


class ClipAugmenter:
    """The three stages of ``csrc/train_aug.hip`` for one photograph on the device.  ``params``: the per-frame dicts of
    ``draw_clip_params`` (``flip``, ``jitter``, ``affine``, ``crop``).  Everything runs on the caller's current stream, in
    order.  What ``jitter`` and ``affine`` return are views of per-stream SCRATCH that the next call of the same method on that
    stream overwrites (they feed the next stage); ``resize`` / ``clip`` return fresh tensors."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._scratch = {}

    # ---- descriptor and scratch
    def _buf(self, name, shape, dtype):
        key = (name, torch.cuda.current_stream(self.device).cuda_stream)
        n = int(np.prod(shape))
        b = self._scratch.get(key)
        if b is None or b.numel() < n or b.dtype != dtype:
            b = self._scratch[key] = torch.empty(n, dtype=dtype, device=self.device)
        return b[:n].view(shape)

    def _desc(self, H, W, params):
        T = len(params)
        if not 1 <= T <= _lib.TRAIN_AUG_MAX_T:
            raise ValueError(f'a clip has 1 .. {_lib.TRAIN_AUG_MAX_T} frames, not {T}')
        if H > MAX_SIDE or W > MAX_SIDE:
            raise ValueError(f'source image {W} x {H}: sides up to {MAX_SIDE}')
        d = _lib.TrainAugDesc()
        d.H, d.W, d.T = H, W, T
        for t, p in enumerate(params):
            f = d.frame[t]
            f.flip = int(bool(p.get('flip')))
            if p.get('jitter') is not None:
                order, (b, c, s, shift) = p['jitter']
                f.jitter = 1
                f.order[:] = list(order)
                f.brightness, f.contrast, f.saturation, f.hue_shift = b, c, s, int(shift)
            if p.get('affine') is not None:
                f.affine = 1
                f.m[:] = [float(v) for v in p['affine']]
                f.nearest_tables = int(f.m[1] == 0 and f.m[3] == 0)       # Pillow: ImagingScaleAffine instead of affine_fixed
            f.win_i, f.win_j, f.win_h, f.win_w = (int(v) for v in p['crop'])
        return d

    def _tables(self, arrays):
        """int32 arrays -> one upload; -> the device tensor and each array's device address."""
        flat = np.concatenate([np.ascontiguousarray(a, np.int32).reshape(-1) for a in arrays])
        dev = torch.from_numpy(flat).to(self.device, non_blocking=True)
        base, addr, off = dev.data_ptr(), [], 0
        for a in arrays:
            addr.append(base + 4 * off)
            off += a.size
        return dev, addr

    # ---- the stages
    def jitter(self, src, params):
        """uint8 [H, W, 3] -> uint8 [T, H, W, 3]: frame t jittered (and flipped) where ``params[t]['jitter']`` is set."""
        H, W = src.shape[:2]
        d = self._desc(H, W, params)
        jit = self._buf('jit', (len(params), H, W, 3), torch.uint8)
        lsum = self._buf('lsum', (len(params),), torch.int64)
        d.src, d.jit, d.lsum = src.data_ptr(), jit.data_ptr(), lsum.data_ptr()
        check(_lib.lib().vfn_train_aug_jitter(C.byref(d), stream()), 'vfn_train_aug_jitter')
        return jit

    def affine(self, src, mask, params, jit=None):
        """-> (win_img uint8 [T, H*W*3], win_mask uint8 [T, H*W]): frame t's crop window [h][w][3] / [h][w] of the transformed
        image and mask at the start of row t (``window`` cuts it out)."""
        H, W = src.shape[:2]
        T = len(params)
        d = self._desc(H, W, params)
        win_img = self._buf('win_img', (T, H * W * 3), torch.uint8)
        win_mask = self._buf('win_mask', (T, H * W), torch.uint8)
        d.src, d.mask, d.win_img, d.win_mask = src.data_ptr(), mask.data_ptr(), win_img.data_ptr(), win_mask.data_ptr()
        if jit is not None:
            d.jit = jit.data_ptr()
        keep = None
        if any(d.frame[t].nearest_tables for t in range(T)):
            xt, yt = np.full((T, W), -1, np.int32), np.full((T, H), -1, np.int32)
            for t in range(T):
                if d.frame[t].nearest_tables:
                    m = d.frame[t].m
                    xt[t], yt[t] = nearest_table(m[0], m[2], W, W), nearest_table(m[4], m[5], H, H)
            keep, (d.aff_xtab, d.aff_ytab) = self._tables([xt, yt])
        check(_lib.lib().vfn_train_aug_affine(C.byref(d), stream()), 'vfn_train_aug_affine')
        del keep                                      # (the caching allocator orders its reuse behind this stream's work)
        return win_img, win_mask

    @staticmethod
    def window(buf, t, h, w, channels):
        """Frame t's window out of ``affine``'s buffers: [h, w, 3] of win_img (channels 3), [h, w] of win_mask (channels 1)."""
        v = buf[t, :h * w * channels]
        return v.view(h, w, 3) if channels == 3 else v.view(h, w)

    def resize(self, win_img, win_mask, H, W, params, S, obj_list):
        """The windows -> (frames float32 [T, 3, S, S], masks float32 [T, len(obj_list) + 1, S, S])."""
        T = len(params)
        obj_n = len(obj_list) + 1
        if not 1 <= obj_n <= _lib.TRAIN_AUG_MAX_OBJ:
            raise ValueError(f'obj_n {obj_n} outside 1 .. {_lib.TRAIN_AUG_MAX_OBJ}')
        d = self._desc(H, W, params)
        tabs = [[resize_tables(p['crop'][3], S), resize_tables(p['crop'][2], S)] for p in params]
        ksx, ksy = max(t[0][1].shape[1] for t in tabs), max(t[1][1].shape[1] for t in tabs)
        kx, ky = np.zeros((T, S, ksx), np.int32), np.zeros((T, S, ksy), np.int32)
        for t in range(T):
            kx[t, :, :tabs[t][0][1].shape[1]] = tabs[t][0][1]
            ky[t, :, :tabs[t][1][1].shape[1]] = tabs[t][1][1]
        bx, by = np.stack([t[0][0] for t in tabs]), np.stack([t[1][0] for t in tabs])
        nx = np.stack([nearest_table(p['crop'][3] / S, 0.0, S, p['crop'][3]) for p in params])
        ny = np.stack([nearest_table(p['crop'][2] / S, 0.0, S, p['crop'][2]) for p in params])
        keep, (d.kx_bounds, d.kx, d.ky_bounds, d.ky, d.nx, d.ny) = self._tables([bx, kx, by, ky, nx, ny])
        hpass = self._buf('hpass', (T, H, S, 3), torch.uint8)
        frames = torch.empty(T, 3, S, S, dtype=torch.float32, device=self.device)
        masks = torch.empty(T, obj_n, S, S, dtype=torch.float32, device=self.device)
        d.win_img, d.win_mask, d.hpass = win_img.data_ptr(), win_mask.data_ptr(), hpass.data_ptr()
        d.frames, d.masks = frames.data_ptr(), masks.data_ptr()
        d.S, d.ksize_x, d.ksize_y, d.obj_n = S, ksx, ksy, obj_n
        for k, o in enumerate(obj_list):
            d.obj_list[k] = int(o)
        check(_lib.lib().vfn_train_aug_resize(C.byref(d), stream()), 'vfn_train_aug_resize')
        del keep
        return frames, masks

    def clip(self, src, mask, params, S, obj_list):
        """All stages: uint8 [H, W, 3] and uint8 [H, W] on the device -> (frames, masks) of the clip."""
        H, W = src.shape[:2]
        jit = self.jitter(src, params) if any(p.get('jitter') is not None for p in params) else None
        win_img, win_mask = self.affine(src, mask, params, jit)
        return self.resize(win_img, win_mask, H, W, params, S, obj_list)

    def labels_present(self, mask, crop, S):
        """The labels of ``mask[i:i+h, j:j+w]`` resized to S x S (nearest), as a sorted list without 0: what
        ``ToOnehot`` (transforms.py:405-411) finds in frame 0.  One 256-byte device-to-host copy (synchronises)."""
        H, W = mask.shape
        i, j, h, w = crop
        xt, yt = nearest_table(w / S, 0.0, S, w), nearest_table(h / S, 0.0, S, h)
        xt, yt = np.where(xt >= 0, xt + j, -1), np.where(yt >= 0, yt + i, -1)
        keep, (xa, ya) = self._tables([xt, yt])
        present = torch.empty(256, dtype=torch.uint8, device=self.device)
        check(_lib.lib().vfn_train_aug_label_present(ptr(mask), H, W, xa, ya, S, ptr(present), stream()),
              'vfn_train_aug_label_present')
        del keep
        table = present.cpu().numpy()
        return [int(v) for v in np.nonzero(table)[0] if v > 0]


def sample_on_device(aug, item, rng, clip_n, S, max_obj_n):
    """``Water_Image_Train_DS.__getitem__`` of the reference (Water_DS.py:53-83) from a host item, on ``aug``'s device and the
    current stream: -> (frames [T, 3, S, S], masks [T, obj_n, S, S], obj_n, params)."""
    src = image_to_device(item['img'], aug.device)
    mask = mask_to_device(item['mask'], aug.device)
    H, W = src.shape[:2]
    if tuple(mask.shape) != (H, W):
        raise ValueError(f"{item['name']}: image {W} x {H}, mask {mask.shape[1]} x {mask.shape[0]}")
    obj = []

    def first(p):                                      # ToOnehot(max_obj_n, shuffle=True) on frame 0 (transforms.py:405-415)
        obj[:] = aug.labels_present(mask, p['crop'], S)
        rng.shuffle(obj)
        del obj[max_obj_n - 1:]
    params = draw_clip_params(rng, W, H, clip_n, S, after_first=first)
    frames, masks = aug.clip(src, mask, params, S, obj)
    return frames, masks, len(obj) + 1, params


class TrainClipLoader:
    """What ``data.DataLoader(Water_Image_Train_DS(...), batch_size=1, shuffle=True, num_workers=2)`` is to the reference's
    ``train_model`` (train_video_seg.py:100): iterating it yields ``(frames [1, T, 3, S, S], masks [1, T, obj_n, S, S], obj_n,
    info)`` on the device -- what ``train.train_model`` takes.  A torch ``DataLoader`` runs the dataset's host part in
    ``num_workers`` processes; the device part of sample n + 1 is issued on a side stream (``_lib.independent_stream``)
    before sample n is handed out.  Not all of it runs beside a training step: ``ToOnehot``'s shuffle needs the labels of
    frame 0's resized mask before frame 1's parameters can be drawn, so preparing a sample waits on the host for the side
    stream to finish the device decode and the label table (``ClipAugmenter.labels_present``), and ``train_step`` has ended
    in a host wait of its own by then -- the decode and that read-back run between two steps, with the training stream idle
    (apart from the optimizer's tail); only the three augmentation stages, enqueued after the wait, overlap with the next
    step.  DESIGN.md section 8b gives the measured cost.  Samples with ``obj_n == 1`` are passed through
    (``train_model`` skips them, train_video_seg.py:60-61).  The same ``seed`` gives bit-identical samples, whatever
    ``num_workers`` is; every pass (epoch) continues the seed's sequence."""

    def __init__(self, dataset, device, shuffle=True, num_workers=2, seed=None):
        self.dataset, self.device = dataset, torch.device(device)
        self.shuffle, self.num_workers = shuffle, num_workers
        self.seed = int.from_bytes(os.urandom(4), 'little') if seed is None else int(seed)
        self.epoch = 0
        self.aug = ClipAugmenter(self.device)
        self._side = None
        self._sampler = _EpochSampler(len(dataset), shuffle)
        self._loader = None

    def __len__(self):
        return len(self.dataset)

    def _prepare(self, item, rng, main):
        ds = self.dataset
        with torch.cuda.stream(self._side):
            frames, masks, obj_n, _ = sample_on_device(self.aug, item, rng, ds.clip_n, ds.output_size, ds.max_obj_n)
            ready = torch.cuda.Event()
            ready.record()
        for t in (frames, masks):
            t.record_stream(main)                      # allocated on the side stream, consumed on the training stream
        return frames.unsqueeze(0), masks.unsqueeze(0), obj_n, {'name': item['name']}, ready

    def __iter__(self):
        if self._side is None:
            with torch.cuda.device(self.device):
                self._side = _lib.independent_stream(self.device)
        if self._loader is None:
            # ONE DataLoader for all epochs, its workers kept: starting workers forks the training process, and forking a
            # process that holds a GPU context and the model costs seconds -- per epoch, that dwarfed the epoch itself
            self._loader = data.DataLoader(self.dataset, batch_size=1, sampler=self._sampler, num_workers=self.num_workers,
                                           collate_fn=_identity, persistent_workers=self.num_workers > 0)
        epoch_seed = self.seed * 1000003 + self.epoch
        self.epoch += 1
        self._sampler.seed = epoch_seed
        rng = random.Random(epoch_seed)
        main = torch.cuda.current_stream(self.device)
        nxt = None
        for item in self._loader:
            cur, nxt = nxt, self._prepare(item, rng, main)
            if cur is not None:
                main.wait_event(cur[4])
                yield cur[:4]
        if nxt is not None:
            main.wait_event(nxt[4])
            yield nxt[:4]


class _EpochSampler(data.Sampler):
    """The order of one epoch: a permutation drawn from ``seed`` (set by ``TrainClipLoader`` before every pass)."""

    def __init__(self, n, shuffle):
        self.n, self.shuffle, self.seed = n, shuffle, 0

    def __len__(self):
        return self.n

    def __iter__(self):
        if not self.shuffle:
            return iter(range(self.n))
        g = torch.Generator()
        g.manual_seed(self.seed % (1 << 62))
        return iter(torch.randperm(self.n, generator=g).tolist())
