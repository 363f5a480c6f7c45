"""The image-segmentation tool files to files (``image_seg.test_waterseg``): a folder of synthetic 1920 x 1080 JPEGs through
``pipeline='host'`` (PIL + torch CPU around one ``predict`` per image: the only path before the device pipeline existed) and
through the device pipeline at several batch sizes, LinknetB4 with synthetic weights, overlays on.  Alternating runs, median and
range of images/s; then ``LinknetB4.predict`` alone by HIP events, ms per image at each batch size.

    python scripts/bench_image_seg.py [--n 64] [--runs 3] [--out profiles/image_seg_device.txt]
"""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from PIL import Image

import vfloodnet_amd  # noqa: F401
from vfloodnet_amd import image_seg
from vfloodnet_amd.linknet import LinknetB4
from tools import synth, synth_linknet as S


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=64)
    ap.add_argument('--runs', type=int, default=3)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--batches', type=int, nargs='+', default=[1, 4, 8, 16])
    ap.add_argument('--out', type=str, default=None)
    args = ap.parse_args()
    dev = torch.device('cuda', 0)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    root = tempfile.mkdtemp(prefix='vfn_imgseg_')
    try:
        folder, warm = os.path.join(root, 'in'), os.path.join(root, 'warm')
        os.makedirs(folder)
        os.makedirs(warm)
        for i in range(args.n):
            f0, _ = synth.frame0(100 + i, args.height, args.width)
            Image.fromarray((f0.permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(os.path.join(folder, f'{i:05d}.jpg'), quality=92)
            if i < 2 * max(args.batches):
                shutil.copy(os.path.join(folder, f'{i:05d}.jpg'), warm)
        print('folder written', flush=True)
        model = LinknetB4.from_checkpoint(S.make_state_dict(), dev)
        configs = [('host', dict(pipeline='host'))] + [(f'device, batch {b}', dict(pipeline='device', batch=b)) for b in args.batches]
        for name, kw in configs:                       # tables, encoders, stream probes, one HIP graph per batch size: not timed
            image_seg.test_waterseg('unused', warm, 'warm', os.path.join(root, 'out'), dev, model=model, **kw)
        rates = {name: [] for name, _ in configs}
        for r in range(args.runs):
            for name, kw in configs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                image_seg.test_waterseg('unused', folder, f'run{r}', os.path.join(root, 'out'), dev, model=model, **kw)
                torch.cuda.synchronize()
                rates[name].append(args.n / (time.perf_counter() - t0))
                print(f'run {r} {name}: {rates[name][-1]:.2f} images/s', flush=True)
        say(f'image_seg.test_waterseg, {args.n} JPEGs of {args.width} x {args.height}, files to files with overlays, LinknetB4 (synthetic weights); '
            f'{args.runs} alternating runs, images/s: median [min .. max]')
        for name, _ in configs:
            v = rates[name]
            say(f'  {name:18s} {statistics.median(v):8.2f}  [{min(v):.2f} .. {max(v):.2f}]')
        say('LinknetB4.predict_batch alone at 416 x 416 (one replayed HIP graph per batch size), HIP events, 20 calls: ms per call, ms per image')
        for B in sorted(set([1, 2] + list(args.batches))):
            x = torch.cat([S.frame(3 + i, 416, 416) for i in range(B)], 0).to(dev)
            for _ in range(4):
                model.predict_batch(x)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20):
                model.predict_batch(x)
            e1.record()
            e1.synchronize()
            ms = e0.elapsed_time(e1) / 20
            say(f'  B = {B:2d}  {ms:8.3f}  {ms / B:8.3f}')
    finally:
        shutil.rmtree(root, ignore_errors=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
