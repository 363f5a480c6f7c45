"""What a training sample costs: ``Water_Image_Train_DS`` + ``TrainClipLoader`` (csrc/train_aug.hip) against the reference's PIL
pipeline, at the reference's training shape (one 1920 x 1080 JPEG -> 6 frames of 400 x 400, 2 objects).

    python scripts/bench_train_aug.py [--out FILE] [--images 12] [--epochs 3]

Parts, each a child process with a time limit of its own; the first failure ends the run:
  device   the device part alone (decode on the device, draws, tables, three stages) per sample: host wall time to a device
           synchronise and device time between events; the host part (read + entropy decode) per item
  train    ``train.train_model`` over the loader against ``train.train_model`` over the same samples as pre-made tensors,
           alternating, three runs each: steps per second and the spread between runs of the same kind
  pil      the reference's transforms with Pillow on this host, 2 worker processes (the reference's DataLoader) and 16
"""
import argparse
import os
import random
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np                                                       # noqa: E402
from PIL import Image, ImageEnhance                                      # noqa: E402

W0, H0, CLIP_N, SIZE = 1920, 1080, 6, 400


def make_dataset(root, n):
    """n photographs-like 1920 x 1080 JPEG files (smooth structure plus mild noise) and palette masks with one object."""
    rng = np.random.default_rng(1)
    os.makedirs(os.path.join(root, 'JPEGImages', 'a'))
    os.makedirs(os.path.join(root, 'Annotations', 'a'))
    with open(os.path.join(root, 'train_imgs.txt'), 'w') as f:
        f.write('a\n')
    yy, xx = np.mgrid[0:H0, 0:W0].astype(np.float32)
    for k in range(n):
        shore = H0 * (0.45 + 0.1 * np.sin(xx[0] / 300.0 + k))
        water = yy > shore[None, :]
        img = np.stack([90 + 60 * np.sin(xx / 97.0 + k) + 40 * np.cos(yy / 61.0), 110 + 50 * np.sin((xx + yy) / 143.0),
                        np.where(water, 170.0, 80.0) + 30 * np.cos(xx / 211.0)], -1)
        img = np.clip(img + rng.normal(0, 6, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'JPEGImages', 'a', f'{k:03d}.jpg'), quality=90)
        pm = Image.fromarray(water.astype(np.uint8), 'P')
        pm.putpalette([0, 0, 0, 0, 0, 128] + [100] * (254 * 3))
        pm.save(os.path.join(root, 'Annotations', 'a', f'{k:03d}.png'))


def pct(xs, q):
    xs = sorted(xs)
    return xs[min(len(xs) - 1, int(q * len(xs)))]


# ------------------------------------------------------------------------------------------------ device part alone
def part_device(root, out):
    import torch
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import train_dataset as D
    dev = torch.device('cuda', 0)
    ds = D.Water_Image_Train_DS(root, SIZE, clip_n=CLIP_N, max_obj_n=3)
    t0 = time.perf_counter()
    items = [ds[i] for i in range(len(ds))]
    host_ms = 1e3 * (time.perf_counter() - t0) / len(ds)
    aug = D.ClipAugmenter(dev)
    rng = random.Random(0)
    wall, devt, stage = [], [], []
    for rep in range(5):
        for it in items:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            frames, masks, obj_n, params = D.sample_on_device(aug, it, rng, CLIP_N, SIZE, 3)
            e1.record()
            torch.cuda.synchronize()
            if rep:                                                      # (the first pass warms every shape up)
                wall.append(1e3 * (time.perf_counter() - t0))
                devt.append(e0.elapsed_time(e1))
    # the three stages alone, on a decoded image (device events around the launches only)
    src, mask = D.image_to_device(items[0]['img'], dev), D.mask_to_device(items[0]['mask'], dev)
    for rep in range(12):
        params = D.draw_clip_params(random.Random(rep), W0, H0, CLIP_N, SIZE)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        torch.cuda.synchronize()
        ev[0].record()
        jit = aug.jitter(src, params)
        ev[1].record()
        wi, wm = aug.affine(src, mask, params, jit)
        ev[2].record()
        aug.resize(wi, wm, H0, W0, params, SIZE, [1])
        ev[3].record()
        torch.cuda.synchronize()
        if rep > 1:
            stage.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)])
    st = np.median(np.array(stage), 0)
    with open(out, 'a') as f:
        f.write(f'device part alone, {len(wall)} samples of {CLIP_N} x {SIZE} x {SIZE} from {W0} x {H0} JPEG, obj_n {obj_n}:\n'
                f'  host wall to synchronise  median {pct(wall, 0.5):.2f} ms  (min {min(wall):.2f}, p90 {pct(wall, 0.9):.2f})\n'
                f'  device time (events)      median {pct(devt, 0.5):.2f} ms  (min {min(devt):.2f}, p90 {pct(devt, 0.9):.2f})  '
                f'[includes the device JPEG / PNG decode and the 256-byte label read-back]\n'
                f'  stages alone (events, median of {len(stage)}): jitter {st[0]:.3f} ms, affine {st[1]:.3f} ms, resize + tensors {st[2]:.3f} ms '
                f'[each includes its table upload]\n'
                f'  host part per item (read + JPEG entropy decode + PNG inflate, one process): {host_ms:.2f} ms\n')


# ------------------------------------------------------------------------------------------------ inside train_model
def part_train(root, out, epochs):
    import torch
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import AFB_URR, train as T, train_dataset as D
    from tools import synth
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    model = AFB_URR(dev, update_bank=False).to(dev)
    model.load_state_dict(synth.make_state_dict(20200212))
    model.train()
    opt = T.AdamW(model.named_parameters(), lr=1e-6)
    ds = D.Water_Image_Train_DS(root, SIZE, clip_n=CLIP_N, max_obj_n=3)
    loader = D.TrainClipLoader(ds, dev, shuffle=True, num_workers=2, seed=1)
    premade = [(f.clone(), m.clone(), n, i) for f, m, n, i in loader]
    n_steps = sum(1 for s in premade if s[2] > 1)
    T.train_model(model, premade, opt)                                   # warm-up: plans, code objects
    T.train_model(model, loader, opt)

    def run(src):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(epochs):
            T.train_model(model, src, opt)
        torch.cuda.synchronize()
        return epochs * n_steps / (time.perf_counter() - t0)
    pre, ld = [], []
    for _ in range(3):
        pre.append(run(premade))
        ld.append(run(loader))
    with open(out, 'a') as f:
        f.write(f'train_model, {epochs * n_steps} steps per run, alternating runs (steps per second; ms per step):\n'
                f'  pre-made tensors : ' + ', '.join(f'{v:.2f} ({1e3 / v:.2f} ms)' for v in pre) + '\n'
                f'  TrainClipLoader  : ' + ', '.join(f'{v:.2f} ({1e3 / v:.2f} ms)' for v in ld) + '\n'
                f'  spread between runs of the same kind: pre-made {100 * (max(pre) - min(pre)) / np.mean(pre):.1f} %, '
                f'loader {100 * (max(ld) - min(ld)) / np.mean(ld):.1f} %; loader / pre-made (means) {np.mean(ld) / np.mean(pre):.3f}\n')


# ------------------------------------------------------------------------------------------------ the reference's PIL pipeline
def pil_sample(args):
    """Water_DS.py:53-83 with Pillow, parameters from draw_clip_params (same distributions as the reference's draws)."""
    img_path, mask_path, seed = args
    from vfloodnet_amd import train_dataset as D
    img0, mask0 = Image.open(img_path).convert('RGB'), Image.open(mask_path).convert('P')
    frames = np.zeros((CLIP_N, 3, SIZE, SIZE), np.float32)
    masks = np.zeros((CLIP_N, 3, SIZE, SIZE), np.float32)
    for t, p in enumerate(D.draw_clip_params(random.Random(seed), W0, H0, CLIP_N, SIZE)):
        img, mask = img0, mask0
        if p['flip']:
            img, mask = img.transpose(Image.FLIP_LEFT_RIGHT), mask.transpose(Image.FLIP_LEFT_RIGHT)
        if p['jitter'] is not None:
            order, (b, c, s, shift) = p['jitter']
            for op in order:
                if op == 0:
                    img = ImageEnhance.Brightness(img).enhance(b)
                elif op == 1:
                    img = ImageEnhance.Contrast(img).enhance(c)
                elif op == 2:
                    img = ImageEnhance.Color(img).enhance(s)
                else:
                    h, s_, v = img.convert('HSV').split()
                    nh = np.array(h, dtype=np.uint8)
                    nh += np.uint8(shift)
                    img = Image.merge('HSV', (Image.fromarray(nh, 'L'), s_, v)).convert('RGB')
        if p['affine'] is not None:
            img = img.transform(img.size, Image.AFFINE, p['affine'], Image.BICUBIC, fillcolor=0)
            mask = mask.transform(mask.size, Image.AFFINE, p['affine'], Image.NEAREST, fillcolor=0)
        i, j, h, w = p['crop']
        img = img.crop((j, i, j + w, i + h)).resize((SIZE, SIZE), Image.BICUBIC)
        mask = np.array(mask.crop((j, i, j + w, i + h)).resize((SIZE, SIZE), Image.NEAREST), np.uint8)
        frames[t] = np.asarray(img).transpose(2, 0, 1).astype(np.float32) / np.float32(255)
        masks[t, 1] = mask == 1
        masks[t, 0] = 1 - masks[t, 1]
    return float(frames.sum())


def part_pil(root, out):
    import multiprocessing as mp
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import train_dataset as D
    ds = D.Water_Image_Train_DS(root, SIZE, clip_n=CLIP_N, max_obj_n=3)
    lines = []
    for workers, n in ((2, 12), (16, 48)):
        jobs = [(ds.img_list[k % len(ds)], ds.mask_list[k % len(ds)], k) for k in range(n)]
        with mp.get_context('fork').Pool(workers) as pool:
            pool.map(pil_sample, jobs[:workers])                         # (workers started, files in the page cache)
            t0 = time.perf_counter()
            pool.map(pil_sample, jobs, chunksize=1)
            dt = time.perf_counter() - t0
        lines.append(f'  {workers:2d} workers: {1e3 * dt / n:.1f} ms per sample ({n} samples in {dt:.1f} s)')
    t0 = time.perf_counter()
    pil_sample((ds.img_list[0], ds.mask_list[0], 0))
    one = 1e3 * (time.perf_counter() - t0)
    with open(out, 'a') as f:
        f.write(f'the reference\'s PIL pipeline on this host (Pillow {Image.__version__ if hasattr(Image, "__version__") else ""}), same shape:\n'
                + '\n'.join(lines) + f'\n  one sample in one process: {one:.0f} ms\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'train_clip_aug.txt'))
    ap.add_argument('--images', type=int, default=12)
    ap.add_argument('--epochs', type=int, default=3)
    ap.add_argument('--part', default=None)
    ap.add_argument('--root', default=None)
    a = ap.parse_args()
    if a.part:
        {'device': lambda: part_device(a.root, a.out), 'train': lambda: part_train(a.root, a.out, a.epochs),
         'pil': lambda: part_pil(a.root, a.out)}[a.part]()
        return 0
    with tempfile.TemporaryDirectory() as tmp:
        root = os.path.join(tmp, 'ds')
        make_dataset(root, a.images)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(f'scripts/bench_train_aug.py --images {a.images} --epochs {a.epochs}\n')
        for part, limit in (('device', 240), ('train', 420), ('pil', 240)):
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), '--part', part, '--root', root, '--out', a.out,
                                 '--epochs', str(a.epochs)], timeout=limit).returncode
            if rc != 0:
                print(f'part {part} failed with status {rc}: stopping', file=sys.stderr)
                return rc
    print(open(a.out).read())
    return 0


if __name__ == '__main__':
    sys.exit(main())
