"""First-frame bootstrap plumbing: the reference's ``test_image_seg.py`` contract (BASELINE config C1).

``test_video_seg.py:64-69`` calls ``test_waterseg(model_path, first_frame, name, out_dir, device)`` when the
first-frame mask PNG is missing.  The network behind it (LinkNet + EfficientNet-b4 from the un-vendored
``segmentation_models_pytorch``, a whole pickled module at ``records/link_efficientb4_model.pth``) is *not* part
of the hot path; what is kept here is everything around ``model.predict``:

    norm_imagenet   Resize(416x416, bilinear) -> ToTensor -> Normalize(mean, std)      test_image_seg.py:44-64
    predict_pil     ... -> model.predict -> Resize(back, bilinear) -> round -> postprocessing_pred
                    -> mode-P PNG with the palette                                       test_image_seg.py:95-124
    predict_one     mask + overlay files                                                 test_image_seg.py:67-92
    test_waterseg   file / folder dispatch, output tree                                  test_image_seg.py:127-151

``model`` is any object with ``predict(x: float[1,3,416,416]) -> float[1,1,416,416]`` in [0,1] (the smp API).
``pipeline='host'`` (the default of ``test_waterseg``) is host plumbing (PIL + a handful of torch CPU ops on one 416x416
image), exactly as in the reference.  ``pipeline='device'`` (``ImageSegRunner``; the default of ``python -m
vfloodnet_amd.image_seg``) runs a folder files-to-files on the GPU: loader workers undo the entropy coding, then device
decode -> Pillow's bilinear resize + normalisation into a slot of the model's batch (``vfn_imgseg_resize_norm``) -> one
``model.predict`` per batch -> per image bilinear enlargement + round (``vfn_imgseg_upsample_round``), largest blob, overlay,
and the two PNGs deflated on a side stream (``png_device.PngSink``).  The files hold the pixels ``predict_one`` writes, except
where the enlarged probability is within 2^-13 of 0.5 (include/vfn_hip.h: torch's CPU kernel is not reproducible bit for bit).
"""
import os
from glob import glob
from pathlib import Path

import numpy as np
import torch
from PIL import Image
from torch.nn import functional as F

from .data import add_overlay, color_palette, load_image_in_PIL, postprocessing_pred

MEAN = torch.tensor([0.485, 0.456, 0.406]).view(3, 1, 1)
STD = torch.tensor([0.229, 0.224, 0.225]).view(3, 1, 1)


def norm_imagenet(img_pil, dims):
    """test_image_seg.py:44-64: PIL bilinear resize to ``dims`` (h, w), /255, ImageNet normalisation."""
    img = img_pil.resize((dims[1], dims[0]), Image.BILINEAR)
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(img).transpose(2, 0, 1))).float().div(255)
    return (t - MEAN) / STD


def predict_pil(model, img_pil, model_dims, device):
    """test_image_seg.py:95-124 -> mode-P PIL image of 0/1 labels with the reference palette."""
    img_np = np.array(img_pil)
    x = norm_imagenet(img_pil, model_dims).unsqueeze(0)
    try:
        prediction = model.predict(x.to(device))
    except Exception:                                   # the reference retries on the host tensor
        print('Did not convert input image to cuda.')
        prediction = model.predict(x)
    prediction = torch.as_tensor(prediction).float().cpu()
    # tf.Resize on a tensor = bilinear interpolate, align_corners=False, no antialias (torchvision 0.9.2)
    prediction = F.interpolate(prediction, size=[img_np.shape[0], img_np.shape[1]], mode='bilinear', align_corners=False)
    pred = postprocessing_pred(prediction.squeeze().round().numpy().astype(np.uint8))
    out = Image.fromarray(pred).convert('P')
    out.putpalette(color_palette)
    return out


def predict_one(path, model, mask_outdir, overlay_outdir, device):
    """test_image_seg.py:67-92."""
    img_pil = load_image_in_PIL(path)
    prediction = predict_pil(model, img_pil, model_dims=(416, 416), device=device)
    basename = str(Path(os.path.basename(path)).stem)
    prediction.save(os.path.join(mask_outdir, basename + '.png'))
    bgr = np.ascontiguousarray(np.array(img_pil)[..., ::-1])
    overlay = add_overlay(bgr, np.array(prediction))
    Image.fromarray(np.ascontiguousarray(overlay[..., ::-1])).save(os.path.join(overlay_outdir, basename + '.png'))


# ------------------------------------------------------------------------------------------------ the device pipeline
MODEL_DIMS = (416, 416)
_tables = {}


def resize_tables_device(n_in, n_out, device):
    """Pillow's coefficient tables of ``Image.resize(..., BILINEAR)`` for one axis (built on the host in double in Pillow's
    operation order, ``train_dataset.resize_tables``) on ``device``: (bounds int32 [n_out, 2], coefficients int32
    [n_out, ksize], ksize); None for an axis whose size does not change (Pillow skips that pass)."""
    if n_in == n_out:
        return None
    key = (n_in, n_out, str(device))
    if key not in _tables:
        from .train_dataset import resize_tables
        bounds, kk = resize_tables(n_in, n_out, 'bilinear')
        _tables[key] = (torch.from_numpy(np.ascontiguousarray(bounds)).to(device), torch.from_numpy(np.ascontiguousarray(kk)).to(device),
                        int(kk.shape[1]))
    return _tables[key]


def resize_norm_device(img_u8, x, b):
    """``norm_imagenet`` on the device: uint8 RGB [H,W,3] -> slot ``b`` of ``x`` f32 [B,3,h,w], the same bits."""
    import ctypes as C
    from . import _lib
    H, W, _ = img_u8.shape
    B, _, h, w = x.shape
    assert img_u8.dtype == torch.uint8 and img_u8.is_contiguous() and x.is_contiguous() and x.dtype == torch.float32
    tx, ty = resize_tables_device(W, w, x.device), resize_tables_device(H, h, x.device)
    hpass = torch.empty(H, w, 3, dtype=torch.uint8, device=x.device) if tx is not None else None
    f3 = C.c_float * 3
    p = _lib.ptr
    _lib.check(_lib.lib().vfn_imgseg_resize_norm(
        p(img_u8), H, W, p(hpass), p(tx[0]) if tx else None, p(tx[1]) if tx else None, tx[2] if tx else 0,
        p(ty[0]) if ty else None, p(ty[1]) if ty else None, ty[2] if ty else 0, p(x), B, b, h, w,
        f3(*[float(v) for v in MEAN.view(-1)]), f3(*[float(v) for v in STD.view(-1)]), _lib.stream()), 'vfn_imgseg_resize_norm')


def upsample_round_device(prob, H, W, out=None):
    """``F.interpolate(prob, (H, W), bilinear, align_corners=False).round()`` as uint8 labels [H,W] on the device (prob f32
    [h,w]; the rule: include/vfn_hip.h)."""
    from . import _lib
    h, w = prob.shape
    assert prob.dtype == torch.float32 and prob.is_contiguous()
    if out is None:
        out = torch.empty(H, W, dtype=torch.uint8, device=prob.device)
    _lib.check(_lib.lib().vfn_imgseg_upsample_round(_lib.ptr(prob), h, w, _lib.ptr(out), H, W, _lib.stream()), 'vfn_imgseg_upsample_round')
    return out


class _Files(torch.utils.data.Dataset):
    def __init__(self, paths):
        self.paths = list(paths)

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from .dataset import device_payload
        return device_payload(self.paths[i]), self.paths[i]


def _first(batch):
    return batch[0]


class ImageSegRunner:
    """``predict_one`` for a list of files on the GPU, ``batch`` images per ``model.predict`` (default 1: a batch lowers the
    network's time per image, 3.2 ms -> 0.7 ms at 16, but files to files the tool spends ~57 ms per 1080p photograph elsewhere and
    no batch size measured faster).

    ``model``: any object with the smp ``predict`` API.  ``linknet.LinknetB4`` gets the whole batch [B,3,416,416] through its
    ``predict_batch``, any other ``torch.nn.Module`` through ``predict``; anything else (a stand-in written for one image) is
    called image by image, and a result that
    comes back on the CPU is uploaded.  Files the device decoders refuse (progressive JPEG, 16-bit / interlaced PNG) are
    decoded by PIL in the loader worker and uploaded.  One host synchronisation per batch (the batch before it has left the
    device); the PNGs are deflated on a side stream and framed + written by ``png_workers`` threads.

    ``keep=True`` keeps, per file stem, the label maps before and after ``postprocessing_pred`` on the device (``kept``)."""

    def __init__(self, model, device, batch=1, viz=True, model_dims=MODEL_DIMS, load_workers=4, png_workers=4, keep=False):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('ImageSegRunner runs on the GPU only (no CPU fallback): use pipeline=\'host\' for the reference path')
        if batch < 1:
            raise ValueError('batch must be >= 1')
        self.model, self.device, self.batch, self.viz, self.dims = model, device, int(batch), viz, tuple(model_dims)
        self.load_workers, self.png_workers = load_workers, png_workers
        self.whole_batch = isinstance(model, torch.nn.Module)
        self.kept = {} if keep else None
        self.predict_calls = 0

    def _upload(self, t):
        pinned = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)      # (the caching host allocator hands the block out again
        np.copyto(pinned.numpy(), t.numpy())                               # only after the copy that reads it has run)
        return pinned.to(self.device, non_blocking=True)

    def _decode(self, payload):
        """-> (RGB uint8 [H,W,3], frame f32 [3,H,W] in [0,1] or None without viz), both on the device."""
        from . import jpeg_device, png_decode, ops
        if 'jpeg' in payload:
            coef, qt, info = payload['jpeg']
            if not self.viz:
                return jpeg_device.to_tensor(self._upload(coef), self._upload(qt), info, self.device, u8_only=True), None
            f, u8 = jpeg_device.to_tensor(self._upload(coef), self._upload(qt), info, self.device, want_u8=True)
            return u8, f
        if 'png' in payload:
            filtered, info, pal = payload['png']
            f, u8 = png_decode.to_tensor(self._upload(filtered), info, self._upload(pal), self.device, want_u8=True)
            return u8, f
        u8 = self._upload(payload['u8'].contiguous())
        return u8, (ops.to_tensor_device(u8) if self.viz else None)

    def _predict(self, x):
        self.predict_calls += 1
        if x.shape[0] > 1 and hasattr(self.model, 'predict_batch'):
            prob = self.model.predict_batch(x)               # (LinknetB4: one launch list for the batch)
        elif self.whole_batch or x.shape[0] == 1:
            prob = self.model.predict(x)
        else:
            prob = torch.cat([torch.as_tensor(self.model.predict(x[i:i + 1])) for i in range(x.shape[0])], 0)
        prob = torch.as_tensor(prob)
        if prob.dtype != torch.float32 or prob.device != self.device:
            prob = prob.float().to(self.device)
        return prob.contiguous()

    def run(self, paths, mask_dir, overlay_dir=None):
        from . import ops
        from .data import AsyncWriter
        from .png_device import PngSink
        paths = list(paths)
        if not paths:
            return
        if self.viz and overlay_dir is None:
            raise ValueError('viz needs an overlay directory')
        with torch.cuda.device(self.device), torch.no_grad():
            loader = torch.utils.data.DataLoader(_Files(paths), batch_size=1, shuffle=False, num_workers=self.load_workers,
                                                 prefetch_factor=4 if self.load_workers > 0 else None, collate_fn=_first)
            it = iter(loader)              # (the workers are forked here, before any HIP graph is captured)
            writer = AsyncWriter(self.png_workers)
            sink = PngSink(self.device, writer)
            h, w = self.dims
            prev_done = None
            pending = []                   # (stem, frame, (H, W)) of the slots filled so far
            x = None
            for n, (payload, path) in enumerate(it):
                if not pending:
                    x = torch.empty(self.batch, 3, h, w, device=self.device)      # (a fresh batch: the one before may still be read)
                u8, frame = self._decode(payload)
                resize_norm_device(u8, x, len(pending))
                pending.append((str(Path(os.path.basename(path)).stem), frame, (int(u8.shape[0]), int(u8.shape[1]))))
                if len(pending) < self.batch and n + 1 < len(paths):
                    continue
                prob = self._predict(x[:len(pending)] if len(pending) < self.batch else x)
                for i, (stem, frame, (H, W)) in enumerate(pending):
                    pre = upsample_round_device(prob[i, 0], H, W)
                    post = ops.postprocess_pred_device(pre)
                    if self.kept is not None:
                        self.kept[stem] = (pre, post)
                    sink.save(post, os.path.join(mask_dir, stem + '.png'), color_palette, frame=frame if self.viz else None,
                              overlay_path=os.path.join(overlay_dir, stem + '.png') if self.viz else None)
                pending = []
                done = torch.cuda.Event()
                with torch.cuda.stream(sink.stream):
                    done.record()
                if prev_done is not None:
                    prev_done.synchronize()            # the batch's one host wait: at most two batches are in flight
                prev_done = done
            writer.close()


def test_waterseg(model_path, test_path, test_name, out_path, device, model=None, pipeline='host', batch=1, viz=True, keep=False):
    """test_image_seg.py:127-151.  ``model`` overrides ``torch.load(model_path)`` (the pickled smp module
    needs its package to unpickle; a stand-in with ``.predict`` is enough for the plumbing).  ``pipeline='device'``: the
    folder goes through ``ImageSegRunner`` (``batch`` images per ``model.predict``, ``viz``: overlays, ``keep``: the label maps stay on
    the device, ``ImageSegRunner.kept``) on the GPU ``device``; returns the runner."""
    if pipeline not in ('host', 'device'):
        raise ValueError("pipeline must be 'host' or 'device'")
    if pipeline == 'device' and torch.device(device).type != 'cuda':
        raise RuntimeError("pipeline='device' needs a GPU device: it has no CPU fallback")
    if model is None:
        # the reference unpickles a whole smp module and calls its predict (:133); here the parameters are read by name out of
        # whatever the file holds (the pickled module, if its package is importable, or a state dict) and predict runs on the
        # HIP path (linknet.LinknetB4)
        from .linknet import LinknetB4
        model = LinknetB4.from_checkpoint(model_path, device)
    out_path = os.path.join(out_path, test_name)
    mask_out = os.path.join(out_path, 'mask')
    overlay_out = os.path.join(out_path, 'overlay')
    os.makedirs(mask_out, exist_ok=True)
    os.makedirs(overlay_out, exist_ok=True)
    if os.path.isfile(test_path):
        paths = [test_path]
    elif os.path.isdir(test_path):
        paths = glob(os.path.join(test_path, '*.jpg')) + glob(os.path.join(test_path, '*.png'))
    else:
        print('Error: Unknown path: ', test_path)
        exit(-1)
    if pipeline == 'device':
        runner = ImageSegRunner(model, device, batch=batch, viz=viz, keep=keep)
        runner.run(paths, mask_out, overlay_out)
        return runner
    for path in paths:
        predict_one(path, model, mask_out, overlay_out, device)


test_waterseg.__test__ = False       # not a pytest test despite the reference's name


def get_args(argv=None):
    """test_image_seg.py's flags plus the device pipeline's."""
    import argparse
    parser = argparse.ArgumentParser(description='Water segmentation of single photographs on the MI355X (test_image_seg.py\'s contract).')
    parser.add_argument('--model-path', default='./records/link_efficientb4_model.pth', type=str, metavar='PATH',
                        help='LinkNet checkpoint: the pickled smp module or a state dict.')
    parser.add_argument('--test-path', type=str, metavar='PATH', required=True, help='One .jpg / .png file, or a folder of them.')
    parser.add_argument('--test-name', type=str, required=True, help='Name of the output subfolder.')
    parser.add_argument('--out-path', default=os.path.join('./', 'output', 'segs'), type=str, metavar='PATH',
                        help='Output root: <out-path>/<test-name>/{mask,overlay}/<stem>.png.')
    parser.add_argument('--batch', type=int, default=1,
                        help='Images per model.predict (default 1: files to files the tool is not bound by the network, DESIGN.md 8c).')
    parser.add_argument('--no-viz', dest='viz', action='store_false', default=True, help='Skip the overlay PNGs.')
    parser.add_argument('--gpu', type=int, default=0, help='GPU card id.')
    parser.add_argument('--pipeline', choices=['device', 'host'], default='device',
                        help='device: decode, resizes, post-processing and PNG compression on the GPU; host: the reference\'s PIL path.')
    return parser.parse_args(argv)


if __name__ == '__main__':
    from .video_seg import gct
    args = get_args()
    if not torch.cuda.is_available() or args.gpu < 0:
        raise ValueError('CUDA is required. --gpu must be >= 0.')
    test_waterseg(args.model_path, args.test_path, args.test_name, args.out_path, torch.device('cuda', args.gpu),
                  pipeline=args.pipeline, batch=args.batch, viz=args.viz)
    print(gct(), 'Test image segmentation done.')
