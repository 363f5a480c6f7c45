"""``WaterDataset_RGB``: the labelled-photograph dataset of ``image_module/dataset_water.py`` with the pixel work on the GPU
(``csrc/train_aug.hip``, entry points ``vfn_imgval_*`` of ``include/vfn_image_val.h``).

The reference builds a sample from one photograph and its palette label with PIL in DataLoader workers.  In mode
``'train_offline'`` -- which ``train_image_seg.py`` uses for the validation loader too -- that is colour changes, an affine map,
a flip, a random crop resized to ``input_size``, ``ToTensor``, ImageNet normalisation, and the label as ``float(index)``;
``'val_offline'`` (written in the reference's ``apply_transforms`` but refused by its constructor) is a plain resize of both:
the deterministic mode for comparing checkpoints.  Here the split is ``train_dataset``'s:

* ``WaterDataset_RGB.__getitem__`` (worker processes) reads the two files and undoes the serial part of their coding;
* ``ImageSampleLoader`` (the process that owns the GPU) finishes the decode on the device, draws the random parameters
  (``draw_sample_params``), builds the small tables Pillow would build and has ``ImageSampleMaker`` launch the kernels into a
  slot of the batch.

For given parameters the tensors equal the ones the reference's transforms produce with Pillow 12.2.0, in every bit
(tests/test_image_val_gpu.py).  The stream of random numbers is NOT the reference's: it draws from the global ``random`` inside
DataLoader workers and is not reproducible itself; here every sample has a generator of its own, seeded from (seed, epoch,
index), so a run does not depend on how the workers are scheduled.
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
from .dataset import device_payload
from .train_dataset import (MAX_SIDE, _host_decode, image_to_device, inverse_affine_matrix, mask_to_device, nearest_table,
                            resize_tables)

MODES = ('train_offline', 'val_offline')
MEAN = (0.485, 0.456, 0.406)
STD = (0.229, 0.224, 0.225)
RANDOM_THRES = 0.8                                     # transforms.py:9
HUE_SHIFT = int(0.1 * 255)                             # transforms.py:28 through torchvision's adjust_hue: 25


# ====================================================================================================== the dataset (host part)
def _by_length_then_name(paths):
    return sorted(paths, key=lambda p: (len(p), p))


class WaterDataset_RGB(data.Dataset):
    """dataset_water.py:18-58, 114-122: ``dataset_path/train_imgs.txt`` names the sub-folders; per sub-folder the labels
    ``Annotations/<sub>/*.png`` and the photographs ``JPEGImages/<sub>/*.jpg``, both sorted by (length of the path, path); a
    photograph without a label of its stem is dropped; the sub-folders follow each other in the file's order.  ``input_size``:
    (S, S), or S.  ``__getitem__`` does the host part only and returns ``{'img': ..., 'label': ..., 'name': path, 'index': i}``;
    ``ImageSampleLoader`` makes the reference's ``(img_norm, label)`` of it."""

    def __init__(self, mode, dataset_path, input_size=None):
        if mode not in MODES:
            raise ValueError(f'mode {mode!r}: one of {MODES}')
        size = (input_size, input_size) if isinstance(input_size, int) else tuple(input_size or ())
        if len(size) != 2 or size[0] != size[1] or not 1 <= size[0] <= _lib.TRAIN_AUG_MAX_OUT:
            raise ValueError(f'input_size {input_size!r}: a square (S, S) with 1 <= S <= {_lib.TRAIN_AUG_MAX_OUT}')
        self.mode, self.input_size = mode, (int(size[0]), int(size[1]))
        self.img_list, self.label_list = [], []
        with open(os.path.join(dataset_path, 'train_imgs.txt')) as f:
            subdirs = [line.strip() for line in f.readlines()]
        for sub in subdirs:
            labels = _by_length_then_name(glob(os.path.join(dataset_path, 'Annotations/', sub, '*.png')))
            self.label_list += labels
            names = [os.path.basename(p)[:-4] for p in labels]
            images = _by_length_then_name(glob(os.path.join(dataset_path, 'JPEGImages/', sub, '*.jpg')))
            self.img_list += [p for p in images if os.path.basename(p)[:-4] in names]

    def __len__(self):
        return len(self.img_list)

    def __getitem__(self, index):
        return {'img': device_payload(self.img_list[index]), 'label': _host_decode(self.label_list[index], 'P'),
                'name': self.img_list[index], 'index': int(index)}


# ====================================================================================================== the random draws
def draw_sample_params(rng, W, H):
    """The random parameters of one ``train_offline`` sample, drawn from ``rng`` (a ``random.Random``) in the order the
    reference consumes the global generator (dataset_water.py:138-140): the three colour operations (transforms.py:12-33: a
    ``random()`` against 0.8 each, and a ``uniform`` for brightness and contrast when taken; hue has no draw of its own), the
    affine map (:35-52: ``random()``, then degrees, the two translations in pixels, scale, shear), the flip (:54), and up to ten
    crop attempts (:101-130: area, aspect ratio, a ``random()`` for swapping w and h, and the two ``randint`` once the box fits),
    else the centred square of side min(W, H).

    -> ``{'brightness': factor | None, 'contrast': factor | None, 'hue': shift 0..255 | None, 'affine': inverse matrix (6
    floats) | None, 'flip': bool, 'crop': (i, j, h, w), 'draws': the raw values}``."""
    if W > MAX_SIDE or H > MAX_SIDE:
        raise ValueError(f'source image {W} x {H}: the affine kernels take sides up to {MAX_SIDE}')
    p = {'brightness': None, 'contrast': None, 'hue': None, 'affine': None, 'flip': False, 'draws': {}}
    if rng.random() < RANDOM_THRES:
        p['brightness'] = rng.uniform(0.1, 1.2)
    if rng.random() < RANDOM_THRES:
        p['contrast'] = rng.uniform(0.2, 1.8)
    if rng.random() < RANDOM_THRES:
        p['hue'] = HUE_SHIFT
    if rng.random() < RANDOM_THRES:
        degrees = rng.uniform(-20, 20)
        translate = (rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2))
        scale = rng.uniform(0.7, 1.3)
        shear = rng.uniform(-20, 20)
        p['affine'] = inverse_affine_matrix(W, H, degrees, translate, scale, shear)
        p['draws'].update(degrees=degrees, translate=translate, scale=scale, shear=shear)
    p['flip'] = rng.random() < 0.5
    area = W * H
    for _ in range(10):
        target_area = rng.uniform(0.08, 1.0) * area
        aspect_ratio = rng.uniform(0.75, 1.33333333)
        w = int(round(math.sqrt(target_area * aspect_ratio)))
        h = int(round(math.sqrt(target_area / aspect_ratio)))
        if rng.random() < 0.5:
            w, h = h, w
        if w <= W and h <= H:
            y = rng.randint(0, H - h)
            x = rng.randint(0, W - w)
            break
    else:
        w = h = min(W, H)
        y, x = (H - w) // 2, (W - w) // 2
    p['crop'] = (y, x, h, w)
    return p


def sample_rng(seed, epoch, index):
    """The generator of one sample: a function of (seed, epoch, index) alone."""
    return random.Random(f'{int(seed)}/{int(epoch)}/{int(index)}')


# ====================================================================================================== the device part
class ImageSampleMaker:
    """The launches of one sample into slot ``b`` of a batch ``x`` f32 [B, 3, S, S], ``y`` f32 [B, 1, S, S], from the decoded
    photograph uint8 [H, W, 3] and its label plane uint8 [H, W] on the device; everything on the caller's current stream.

    ``train_sample``: colour (0, 1 or 2 launches), the window of affine + flip (1), the bicubic resize + normalisation (2), the
    label gather (1).  ``val_sample``: ``vfn_imgseg_resize_norm`` (1 or 2) and the label gather (1)."""

    def __init__(self, device):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('ImageSampleMaker runs on the GPU only (no CPU fallback)')
        self._nearest = {}
        self._mean, self._std = (C.c_float * 3)(*MEAN), (C.c_float * 3)(*STD)

    def _tables(self, arrays):
        """int32 arrays -> one upload; -> the device tensor and each array's device address."""
        flat = np.concatenate([np.ascontiguousarray(a, np.int32).reshape(-1) for a in arrays])
        dev = torch.from_numpy(flat).to(self.device, non_blocking=True)
        base, addr, off = dev.data_ptr(), [], 0
        for a in arrays:
            addr.append(C.c_void_p(base + 4 * off))
            off += a.size
        return dev, addr

    @staticmethod
    def _check(img, label, x, y, b):
        H, W = int(img.shape[0]), int(img.shape[1])
        if img.dtype != torch.uint8 or img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
            raise ValueError('the photograph must be a contiguous uint8 [H, W, 3]')
        if label.dtype != torch.uint8 or tuple(label.shape) != (H, W) or not label.is_contiguous():
            raise ValueError(f'the label must be a contiguous uint8 [{H}, {W}], got {tuple(label.shape)}')
        B, S = int(x.shape[0]), int(x.shape[2])
        if x.dtype != torch.float32 or tuple(x.shape) != (B, 3, S, S) or not x.is_contiguous():
            raise ValueError('x must be a contiguous f32 [B, 3, S, S]')
        if y.dtype != torch.float32 or tuple(y.shape) != (B, 1, S, S) or not y.is_contiguous():
            raise ValueError('y must be a contiguous f32 [B, 1, S, S]')
        if not 0 <= b < B:
            raise ValueError(f'slot {b} outside 0 .. {B - 1}')
        for t in (img, label, x, y):
            _lib.require_gpu(t)
        return H, W, B, S

    def jitter(self, img, p):
        """The colour step -> the changed image (fresh), or ``img`` itself when no operation was drawn."""
        if p.get('brightness') is None and p.get('contrast') is None and p.get('hue') is None:
            return img
        H, W = int(img.shape[0]), int(img.shape[1])
        jit = torch.empty_like(img)
        lsum = torch.empty(1, dtype=torch.int64, device=self.device)
        bri, con, hue = p.get('brightness'), p.get('contrast'), p.get('hue')
        check(_lib.lib().vfn_imgval_jitter(ptr(img), H, W, int(bri is not None), float(bri or 0.0), int(con is not None),
                                           float(con or 0.0), int(hue is not None), int(hue or 0), ptr(jit), ptr(lsum), stream()),
              'vfn_imgval_jitter')
        return jit

    def affine_window(self, img, label, p):
        """-> (win_img uint8 [h, w, 3], win_label uint8 [h, w]): the crop window of the mapped, then flipped, image and label."""
        H, W = int(img.shape[0]), int(img.shape[1])
        i, j, h, w = (int(v) for v in p['crop'])
        if h < 1 or w < 1:
            raise ValueError(f'empty crop window {w} x {h}')
        win_img = torch.empty(h, w, 3, dtype=torch.uint8, device=self.device)
        win_label = torch.empty(h, w, dtype=torch.uint8, device=self.device)
        m = p.get('affine')
        keep, xt, yt, tabs, mm = None, None, None, 0, None
        if m is not None:
            mm = (C.c_double * 6)(*[float(v) for v in m])
            tabs = int(mm[1] == 0 and mm[3] == 0)              # Pillow: ImagingScaleAffine instead of affine_fixed
            if tabs:
                keep, (xt, yt) = self._tables([nearest_table(mm[0], mm[2], W, W), nearest_table(mm[4], mm[5], H, H)])
        check(_lib.lib().vfn_imgval_affine_window(ptr(img), ptr(label), H, W, int(m is not None), mm, tabs, xt, yt,
                                                  int(bool(p.get('flip'))), i, j, h, w, ptr(win_img), ptr(win_label), stream()),
              'vfn_imgval_affine_window')
        del keep                                      # (the caching allocator orders its reuse behind this stream's work)
        return win_img, win_label

    def resize_norm(self, win_img, x, b):
        """``resize((S, S), BICUBIC)`` + ``ToTensor`` + ``Normalize`` of a tight window into slot ``b`` of ``x``."""
        h, w = int(win_img.shape[0]), int(win_img.shape[1])
        B, S = int(x.shape[0]), int(x.shape[2])
        (bx, kx), (by, ky) = resize_tables(w, S), resize_tables(h, S)
        keep, (abx, akx, aby, aky) = self._tables([bx, kx, by, ky])
        hpass = torch.empty(h, S, 3, dtype=torch.uint8, device=self.device)
        check(_lib.lib().vfn_imgval_resize_norm(ptr(win_img), h, w, ptr(hpass), abx, akx, int(kx.shape[1]), aby, aky,
                                                int(ky.shape[1]), ptr(x), B, b, S, self._mean, self._std, stream()),
              'vfn_imgval_resize_norm')
        del keep

    def label_gather(self, plane, y, b, cache=False):
        """Pillow's nearest ``resize((S, S))`` of a tight label plane into slot ``b`` of ``y``, as ``float(index)``."""
        h, w = int(plane.shape[0]), int(plane.shape[1])
        B, S = int(y.shape[0]), int(y.shape[2])
        key = (h, w, S)
        keep = self._nearest.get(key) if cache else None
        if keep is None:
            keep = self._tables([nearest_table(w / S, 0.0, S, w), nearest_table(h / S, 0.0, S, h)])
            if cache:
                if len(self._nearest) >= 64:
                    self._nearest.clear()
                self._nearest[key] = keep
        nx, ny = keep[1]
        check(_lib.lib().vfn_imgval_label_gather(ptr(plane), h, w, nx, ny, ptr(y), B, b, S, stream()), 'vfn_imgval_label_gather')

    def train_sample(self, img, label, p, x, y, b):
        """One ``train_offline`` sample for the parameters ``p`` of ``draw_sample_params``."""
        self._check(img, label, x, y, b)
        win_img, win_label = self.affine_window(self.jitter(img, p), label, p)
        self.resize_norm(win_img, x, b)
        self.label_gather(win_label, y, b)

    def val_sample(self, img, label, x, y, b):
        """One ``val_offline`` sample: ``TF.resize`` of the photograph (bilinear) and of the label (nearest: mode P)."""
        from .image_seg import resize_norm_device
        self._check(img, label, x, y, b)
        resize_norm_device(img, x, b)
        self.label_gather(label, y, b, cache=True)


def _identity(batch):
    return batch[0]


class _Order(data.Sampler):
    def __init__(self, n):
        self.n, self.order = n, list(range(n))

    def __len__(self):
        return self.n

    def __iter__(self):
        return iter(self.order)


class ImageSampleLoader:
    """What ``data.DataLoader(WaterDataset_RGB(...), batch_size, shuffle, num_workers)`` is to the reference
    (train_image_seg.py:68-80): iterating it yields ``(x f32 [b, 3, S, S], y f32 [b, 1, S, S])`` on the device, b = batch_size
    except for a short last batch.  A torch ``DataLoader`` runs the dataset's host part in ``num_workers`` processes, one
    photograph per item (the photographs of a batch differ in size); the decode and the sample kernels are issued here on the
    current stream.  Every pass is an epoch: sample ``index`` of epoch ``e`` draws from ``sample_rng(seed, e, index)``, and a
    shuffled order is a permutation drawn from (seed, e) -- the same ``seed`` gives the same batches bit for bit, whatever
    ``num_workers`` is.  ``params`` holds the parameter dicts of the last pass, in the order the samples were made."""

    def __init__(self, dataset, device, batch_size=1, shuffle=False, num_workers=4, seed=0):
        if batch_size < 1:
            raise ValueError('batch_size must be >= 1')
        self.dataset, self.device = dataset, torch.device(device)
        self.batch_size, self.shuffle, self.num_workers, self.seed = int(batch_size), bool(shuffle), int(num_workers), int(seed)
        self.epoch = 0
        self.maker = ImageSampleMaker(self.device)
        self.params = []
        self._order = _Order(len(dataset))
        self._loader = None

    def __len__(self):
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def _make(self, item, epoch, x, y, b):
        img = image_to_device(item['img'], self.device)
        label = mask_to_device(item['label'], self.device)
        if tuple(label.shape) != tuple(img.shape[:2]):
            raise ValueError(f"{item['name']}: image {img.shape[1]} x {img.shape[0]}, label {label.shape[1]} x {label.shape[0]}")
        if self.dataset.mode == 'val_offline':
            self.params.append(None)
            self.maker.val_sample(img, label, x, y, b)
        else:
            p = draw_sample_params(sample_rng(self.seed, epoch, item['index']), int(img.shape[1]), int(img.shape[0]))
            self.params.append(p)
            self.maker.train_sample(img, label, p, x, y, b)

    def __iter__(self):
        n, S = len(self.dataset), self.dataset.input_size[0]
        epoch = self.epoch
        self.epoch += 1
        self.params = []
        if self._loader is None:                       # one DataLoader for all passes, its workers kept (train_dataset.TrainClipLoader)
            self._loader = data.DataLoader(self.dataset, batch_size=1, sampler=self._order, num_workers=self.num_workers,
                                           collate_fn=_identity, persistent_workers=self.num_workers > 0)
        self._order.order = (random.Random(f'{self.seed}/{epoch}/order').sample(range(n), n) if self.shuffle else list(range(n)))
        with torch.cuda.device(self.device):
            x = y = None
            b = 0
            for k, item in enumerate(self._loader):
                if b == 0:
                    nb = min(self.batch_size, n - k)
                    x = torch.empty(nb, 3, S, S, dtype=torch.float32, device=self.device)
                    y = torch.empty(nb, 1, S, S, dtype=torch.float32, device=self.device)
                self._make(item, epoch, x, y, b)
                b += 1
                if b == x.shape[0]:
                    b = 0
                    yield x, y
