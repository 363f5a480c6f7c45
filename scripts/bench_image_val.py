"""One ``train_offline`` sample of ``WaterDataset_RGB`` (image_module/dataset_water.py:136-153), decoded photograph to
normalised tensor: the device path (``image_dataset.ImageSampleMaker.train_sample``: host tables + HIP launches, HIP events
around the launches of all samples) and the PIL path (the reference's transforms called with the same parameters, host clock),
over the same samples.  Alternating runs in one job; median and range of the time per sample.  The outputs of the two paths are
compared bit for bit before anything is timed.

    python scripts/bench_image_val.py [--n 64] [--runs 3] [--out profiles/image_val_device.txt]
"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image, ImageEnhance

import vfloodnet_amd  # noqa: F401
from vfloodnet_amd.image_dataset import MEAN, STD, ImageSampleMaker, draw_sample_params, sample_rng


def photographs(k, H, W):
    """k distinct synthetic photographs (smooth gradients + texture + noise) with a two-label plane."""
    rng = np.random.default_rng(1)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float32)
    out = []
    for i in range(k):
        base = np.stack([127 + 100 * np.sin(xx / (90 + 7 * i) + i), 127 + 100 * np.cos(yy / (70 + 5 * i)),
                         127 + 60 * np.sin((xx + yy) / 130) + 40 * np.cos(xx / 11)], -1)
        img = np.clip(base + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
        lab = (yy > H * (0.45 + 0.03 * i) + 40 * np.sin(xx / 200)).astype(np.uint8)
        out.append((img, lab))
    return out


def pil_sample(img, lab, p, S):
    """The reference's transforms on PIL images with given parameters (torchvision's PIL back end, call for call)."""
    a, l = Image.fromarray(img, 'RGB'), Image.fromarray(lab, 'P')
    if p['brightness'] is not None:
        a = ImageEnhance.Brightness(a).enhance(p['brightness'])
    if p['contrast'] is not None:
        a = ImageEnhance.Contrast(a).enhance(p['contrast'])
    if p['hue'] is not None:
        h, s, v = a.convert('HSV').split()
        np_h = np.array(h, dtype=np.uint8)
        with np.errstate(over='ignore'):
            np_h += np.uint8(p['hue'])
        a = Image.merge('HSV', (Image.fromarray(np_h, 'L'), s, v)).convert('RGB')
    if p['affine'] is not None:
        m = tuple(float(v) for v in p['affine'])
        a = a.transform(a.size, Image.AFFINE, m, Image.BICUBIC, fillcolor=0)
        l = l.transform(l.size, Image.AFFINE, m, Image.NEAREST, fillcolor=0)
    if p['flip']:
        a, l = a.transpose(Image.FLIP_LEFT_RIGHT), l.transpose(Image.FLIP_LEFT_RIGHT)
    i, j, h, w = p['crop']
    a = a.crop((j, i, j + w, i + h)).resize((S, S), Image.BICUBIC)
    l = l.crop((j, i, j + w, i + h)).resize((S, S), Image.NEAREST)
    t = torch.from_numpy(np.ascontiguousarray(np.asarray(a).transpose(2, 0, 1))).float().div(255)
    x = (t - torch.tensor(MEAN).view(3, 1, 1)) / torch.tensor(STD).view(3, 1, 1)
    return x, torch.from_numpy(np.array(l, np.float32))[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--size', type=int, default=416)
    ap.add_argument('--distinct', type=int, default=8, help='distinct photographs the samples are drawn from')
    ap.add_argument('--repeat', type=int, default=16, help='passes over the samples per timed device run')
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise RuntimeError('this benchmark needs the GPU')
    dev = torch.device('cuda', 0)
    H, W, S, n = args.height, args.width, args.size, args.n
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    photos = photographs(min(args.distinct, n), H, W)
    on_dev = [(torch.from_numpy(i).to(dev), torch.from_numpy(l).to(dev)) for i, l in photos]
    params = [draw_sample_params(sample_rng(0, 0, k), W, H) for k in range(n)]
    maker = ImageSampleMaker(dev)
    x = torch.empty(n, 3, S, S, device=dev)
    y = torch.empty(n, 1, S, S, device=dev)

    def device_run():
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for _ in range(args.repeat):                   # (the 64 samples take ~16 ms: too short a window on its own)
            for k, p in enumerate(params):
                img, lab = on_dev[k % len(on_dev)]
                maker.train_sample(img, lab, p, x, y, k)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / (n * args.repeat), (time.perf_counter() - t0) * 1e3 / (n * args.repeat)

    def pil_run(keep=None):
        t0 = time.perf_counter()
        for k, p in enumerate(params):
            img, lab = photos[k % len(photos)]
            out = pil_sample(img, lab, p, S)
            if keep is not None:
                keep.append(out)
        return (time.perf_counter() - t0) * 1e3 / n

    ref = []
    device_run()                                       # warm-up: code objects, allocator; and the outputs for the comparison
    pil_run(ref)
    gx, gy = x.cpu(), y.cpu()
    same = all(torch.equal(gx[k].view(torch.int32), ref[k][0].view(torch.int32)) and torch.equal(gy[k], ref[k][1]) for k in range(n))
    if not same:
        raise RuntimeError('the device path and the PIL path disagree')
    ev, wall, pil = [], [], []
    for r in range(args.runs):
        e, w_ = device_run()
        ev.append(e)
        wall.append(w_)
        pil.append(pil_run())
        print(f'run {r}: device {e:.3f} ms (events), {w_:.3f} ms (host clock); PIL {pil[-1]:.2f} ms', flush=True)
    taken = {k: sum(p[k] is not None for p in params) for k in ('brightness', 'contrast', 'hue', 'affine')}
    say(f'one train_offline sample of WaterDataset_RGB, decoded {W} x {H} photograph + label -> f32 [3,{S},{S}] + [1,{S},{S}]; {n} samples '
        f'(parameters of seed 0; {taken["brightness"]} / {taken["contrast"]} / {taken["hue"]} / {taken["affine"]} with brightness / contrast / hue / '
        f'affine, {sum(p["flip"] for p in params)} flipped) from {len(photos)} synthetic photographs; outputs of both paths equal in every bit')
    say(f'{args.runs} alternating runs (device: {args.repeat} passes over the samples per run; PIL: one), ms per sample: median [min .. max]')
    for name, v in (('device, HIP events around the launches (host tables included)', ev), ('device, host clock to the last kernel', wall),
                    ('PIL on the host, one process', pil)):
        say(f'  {name:64s} {statistics.median(v):9.3f}  [{min(v):.3f} .. {max(v):.3f}]')
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
