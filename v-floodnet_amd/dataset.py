"""``Video_DS``: the test-time dataset of ``video_module/dataset/Water_DS.py:87-111``.

Same constructor and item contract: ``Video_DS(img_list, first_frame, first_mask)`` with PIL inputs,
``.obj_n``, ``.first_frame`` float[3,H,W] in [0,1], ``.first_mask`` uint8 one-hot [obj_n,H,W],
``ds[i] -> (frame float[3,H,W], name)`` for ``img_list[1:]``.
"""
import os

import numpy as np
import torch
from torch.utils import data

from .data import load_image_in_PIL


def to_tensor(pic):
    """torchvision ``ToTensor``: HWC uint8 -> CHW float32 / 255."""
    arr = np.asarray(pic)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(arr.transpose(2, 0, 1)))
    return t.to(torch.float32).div(255) if t.dtype == torch.uint8 else t


def to_onehot(mask, max_obj_n):
    """``ToOnehot(max_obj_n, shuffle=False)`` (transforms.py:383-421): channel 0 = 1 - sum(objects)."""
    mask = np.asarray(mask)
    new_mask = np.zeros((max_obj_n, *mask.shape), np.uint8)
    obj_list = [i for i in range(1, int(mask.max()) + 1) if (mask == i).any()][:max_obj_n - 1]
    for i, o in enumerate(obj_list):
        new_mask[i + 1] = (mask == o).astype(np.uint8)
    new_mask[0] = 1 - np.sum(new_mask, axis=0)
    return torch.from_numpy(new_mask), obj_list


def device_payload(path):
    """One image file for the device decoders (host only, safe in DataLoader workers): ``{'jpeg': (coef, qt, info)}`` /
    ``{'png': (filtered scanlines, info, palette)}`` / ``{'u8': HWC uint8}`` as ``Video_DS(decode='device')`` hands them out."""
    # Dispatch on the file's magic bytes, not its extension (PIL sniffs content too: a PNG saved as .jpg works in
    # the reference, Water_DS.py:105-109), and hand ANY host-side decode failure to PIL -- the reference's decoder
    # decides whether the file is really bad (it tolerates some truncated / odd files) and raises its own error.
    import zlib
    with open(path, 'rb') as f:
        data_ = f.read()
    try:
        if data_[:2] == b'\xff\xd8':
            from . import jpeg_device
            coef, qt, info = jpeg_device.entropy_decode(data_)
            return {'jpeg': (torch.from_numpy(coef), torch.from_numpy(qt.astype(np.int16)), torch.from_numpy(info))}
        if data_[:8] == b'\x89PNG\r\n\x1a\n':
            from . import png_decode
            filtered, info, pal = png_decode.inflate(data_)
            return {'png': (torch.from_numpy(filtered), torch.from_numpy(info), torch.from_numpy(pal))}
    except (RuntimeError, zlib.error, ValueError):
        pass
    return {'u8': torch.from_numpy(np.array(load_image_in_PIL(path, 'RGB'), np.uint8))}


class Video_DS(data.Dataset):
    """dataset/Water_DS.py:105-139.  Extensions used by ``video_seg.main`` (the defaults are the reference's contract):

    ``raw_u8=True``: ``__getitem__`` hands out the decoded uint8 HWC frame and ``ToTensor`` runs on the GPU
    (``ops.to_tensor_device``, bit-identical), so a frame crosses PCIe as 1 byte per sample.

    ``decode='device'``: baseline JPEG files are only entropy-decoded here (``jpeg_device.entropy_decode``, host C++,
    safe in worker processes); the item is a dict ``{'jpeg': (coef, qt, info)}`` and inverse DCT, chroma upsampling,
    colour conversion and ``ToTensor`` run on the GPU (``jpeg_device.to_tensor``) -- the same tensor, bit for bit.
    8-bit non-interlaced PNG files are only inflated here (``png_decode.inflate``) and come as
    ``{'png': (filtered scanlines, info, palette)}``; the scanline filters are undone on the GPU (``png_decode.to_tensor``).
    Variants outside those subsets (progressive / CMYK JPEG, 16-bit or interlaced PNG ...) are decoded by PIL as before and
    come as ``{'u8': HWC uint8}``; use ``collate_fn=Video_DS.collate`` (batch size 1)."""

    def __init__(self, img_list, first_frame, first_mask, raw_u8=False, decode='pil'):
        if decode not in ('pil', 'device'):
            raise ValueError("decode must be 'pil' or 'device'")
        self.raw_u8 = raw_u8
        self.decode = decode
        self.img_list = img_list[1:]
        self.video_len = len(self.img_list)
        first_mask = np.array(first_mask, np.uint8) > 0
        self.obj_n = int(first_mask.max()) + 1
        mask, _ = to_onehot(first_mask, self.obj_n)
        self.first_mask = mask[:self.obj_n]
        self.first_frame = to_tensor(first_frame)

    def __len__(self):
        return self.video_len

    @staticmethod
    def collate(batch):
        assert len(batch) == 1, 'the inference loop runs with batch size 1 (test_video_seg.py:74)'
        return batch[0]

    def __getitem__(self, idx):
        path = self.img_list[idx]
        img_name = os.path.basename(path)[:-4]
        if self.decode == 'device':
            return device_payload(path), img_name
        img = load_image_in_PIL(path, 'RGB')
        frame = torch.from_numpy(np.array(img, np.uint8)) if self.raw_u8 else to_tensor(img)
        return frame, img_name
