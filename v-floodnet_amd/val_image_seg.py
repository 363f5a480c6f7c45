"""Scoring LinkNet checkpoints on a labelled set: the validation half of ``train_image_seg.py`` on the GPU.

The reference answers "how good is this checkpoint" inside its training loop (train_image_seg.py:134-160, 176-197): smp's
``ValidEpoch`` over ``WaterDataset_RGB`` with ``DiceLoss()`` and ``IoU(threshold=0.5)``, and ``score > max_score`` picks the
best epoch.  Here that is a tool of its own:

    seg_scores / dice_loss / iou_score   the five sums of a batch, loss and score in float64 on the device (vfn_seg_scores_f64)
    ValidEpoch(model, device).run(loader)   the mean loss and score over the batches of a loader; one read-back per epoch
    select_best(scores)                  the reference's strict ``score > max_score`` rule, starting from 0

    python -m vfloodnet_amd.val_image_seg --dataset-path D --model-path F [F ...]

The formulas are smp 0.2.0's, stated in include/vfn_image_val.h as the definition; parity with smp itself (its f32 sums) is
not pinned: the package is no dependency.  Everything runs on the GPU; there is no CPU fallback.
"""
import json
import os
from glob import glob

import torch

from . import _lib
from ._lib import ptr, stream, check

LOG_ROWS = 1024                                        # rows of one block of ValidEpoch's device log


def _part(device):
    return torch.empty(_lib.SEG_SCORES_MAX_BLOCKS * 5, dtype=torch.float64, device=device)


def _flat_pair(pr, gt):
    _lib.require_gpu(pr, 'pr')
    _lib.require_gpu(gt, 'gt')
    if pr.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError('pr and gt must be float32')
    if pr.numel() != gt.numel() or pr.numel() < 1 or pr.numel() >= 2 ** 31:
        raise ValueError(f'pr and gt must hold the same number of elements, 1 .. 2^31 - 1: {tuple(pr.shape)}, {tuple(gt.shape)}')
    return pr.contiguous(), gt.contiguous()


def seg_scores(pr, gt, threshold=0.5, log=None, t=0, part=None):
    """``pr`` (probabilities) and ``gt`` (labels), f32 of one shape on the GPU -> ``(sums, row)``: the sums S0 .. S4 of
    include/vfn_image_val.h as f64 [5] and ``[dice_loss, iou_score]`` as f64 [2], both on the device (no synchronisation).
    ``log`` f64 [rows, 2] on the device: the row is ``log[t]``, written in place."""
    pr, gt = _flat_pair(pr, gt)
    dev = pr.device
    if log is None:
        log, t = torch.empty(1, 2, dtype=torch.float64, device=dev), 0
    if log.dtype != torch.float64 or log.dim() != 2 or log.shape[1] != 2 or not log.is_contiguous() or log.device != dev:
        raise ValueError('log must be a contiguous float64 [rows, 2] on the device of pr')
    part = _part(dev) if part is None else part
    sums = torch.empty(5, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().vfn_seg_scores_f64(ptr(pr), ptr(gt), pr.numel(), float(threshold), ptr(part), ptr(sums), ptr(log),
                                            int(log.shape[0]), int(t), stream()), 'vfn_seg_scores_f64')
    return sums, log[t]


def dice_loss(pr, gt):
    """smp ``DiceLoss()`` (eps 1, beta 1, no activation) over the whole tensor, as a float (synchronises)."""
    return float(seg_scores(pr, gt)[1][0])


def iou_score(pr, gt, threshold=0.5):
    """smp ``IoU(threshold)`` (eps 1e-7) over the whole tensor, as a float (synchronises)."""
    return float(seg_scores(pr, gt, threshold)[1][1])


def select_best(scores):
    """train_image_seg.py:162, 193-194: the index whose score is the first to exceed every score before it and 0 -- a tie keeps
    the earlier one, and scores that are all 0 select none (None)."""
    best, max_score = None, 0
    for k, score in enumerate(scores):
        if score > max_score:
            best, max_score = k, score
    return best


class ValidEpoch:
    """smp's ``ValidEpoch(model, loss=DiceLoss(), metrics=[IoU(threshold=0.5)])`` (train_image_seg.py:154-160).  ``model``: any
    object ``image_seg.ImageSegRunner`` accepts -- a ``linknet.LinknetB4`` gets whole batches through ``predict_batch``, another
    ``torch.nn.Module`` through ``predict``, anything else image by image.  ``run(loader)`` takes ``(x, y)`` device batches
    (``image_dataset.ImageSampleLoader``) and returns ``{'dice_loss': float, 'iou_score': float}``, each the mean over the
    batches in double (smp's ``AverageValueMeter``: a running sum divided by the count).  Loss and score of batch t are formed
    on the device into row t of a log that is read back once, at the end of the epoch: no host synchronisation per batch.
    ``log`` keeps that read-back, f64 [batches, 2]."""

    def __init__(self, model, device, threshold=0.5):
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError('ValidEpoch runs on the GPU only (no CPU fallback)')
        self.model, self.device, self.threshold = model, device, float(threshold)
        self.whole_batch = isinstance(model, torch.nn.Module)
        self.log = None

    def _predict(self, x):
        if x.shape[0] > 1 and hasattr(self.model, 'predict_batch'):
            prob = self.model.predict_batch(x)
        elif self.whole_batch or x.shape[0] == 1:
            prob = self.model.predict(x)
        else:
            prob = torch.cat([torch.as_tensor(self.model.predict(x[i:i + 1])) for i in range(x.shape[0])], 0)
        prob = torch.as_tensor(prob)
        if prob.dtype != torch.float32 or prob.device != self.device:
            prob = prob.float().to(self.device)
        return prob.contiguous()

    def run(self, loader):
        blocks, t = [], 0
        with torch.cuda.device(self.device), torch.no_grad():
            part = _part(self.device)
            for x, y in loader:
                if t % LOG_ROWS == 0:
                    blocks.append(torch.empty(LOG_ROWS, 2, dtype=torch.float64, device=self.device))
                seg_scores(self._predict(x), y, self.threshold, log=blocks[-1], t=t % LOG_ROWS, part=part)
                t += 1
            if t == 0:
                raise ValueError('the loader produced no batch')
            self.log = torch.cat(blocks)[:t].cpu().numpy()           # the epoch's one read-back
        sums = [0.0, 0.0]
        for row in self.log:
            sums[0] += float(row[0])
            sums[1] += float(row[1])
        return {'dice_loss': sums[0] / t, 'iou_score': sums[1] / t}


def load_checkpoint(path, device):
    """A file of train_image_seg.py -> ``LinknetB4`` on ``device``: the pickled module (``torch.save(model)``, :196), a state
    dict, or the resume checkpoint whose ``'weights'`` entry is the state dict (:179-190)."""
    from .linknet import LinknetB4
    try:
        obj = torch.load(path, map_location='cpu', weights_only=True)
    except Exception:
        return LinknetB4.from_checkpoint(path, device)
    if isinstance(obj, dict) and 'weights' in obj and 'encoder._conv_stem.weight' not in obj:
        obj = obj['weights']
    return LinknetB4.from_checkpoint(obj, device)


def model_paths(args):
    """``--model-path``: files, or folders whose ``*.pth`` are taken sorted by (length, name)."""
    out = []
    for p in args:
        if os.path.isdir(p):
            out += sorted(glob(os.path.join(p, '*.pth')), key=lambda q: (len(q), q))
        else:
            out.append(p)
    if not out:
        raise ValueError('no checkpoint found')
    return out


def get_args(argv=None):
    import argparse
    parser = argparse.ArgumentParser(description='Score LinkNet checkpoints on a labelled set on the MI355X '
                                                 '(the validation epoch of train_image_seg.py).')
    parser.add_argument('--dataset-path', type=str, metavar='PATH', required=True,
                        help='Dataset root: train_imgs.txt, JPEGImages/<sub>/*.jpg, Annotations/<sub>/*.png.')
    parser.add_argument('--model-path', type=str, metavar='PATH', nargs='+', required=True,
                        help='Checkpoint files (pickled module, state dict or resume checkpoint), or folders of .pth files.')
    parser.add_argument('--input-shape', default=416, type=int, help='Input size of the model, a multiple of 32.')
    parser.add_argument('--batch-size', default=1, type=int, help='Samples per batch (the reference validates with 1).')
    parser.add_argument('--mode', choices=['train_offline', 'val_offline'], default='train_offline',
                        help='train_offline: augmented samples, as the reference validates; val_offline: a plain resize, the same '
                             'for every seed.')
    parser.add_argument('--seed', default=0, type=int, help='Seed of the augmentation draws.')
    parser.add_argument('--num-workers', default=4, type=int, help='Loader processes for the host part of the decoding.')
    parser.add_argument('--gpu', default=0, type=int, help='GPU card id.')
    parser.add_argument('--json', type=str, metavar='PATH', default=None, help='Write every score at full precision.')
    return parser.parse_args(argv)


def main(argv=None):
    from .image_dataset import ImageSampleLoader, WaterDataset_RGB
    args = get_args(argv)
    if not torch.cuda.is_available() or args.gpu < 0:
        raise ValueError('CUDA is required. --gpu must be >= 0.')
    if args.input_shape < 32 or args.input_shape % 32:
        raise ValueError('--input-shape must be a multiple of 32 (the image is subsampled 5 times)')
    device = torch.device('cuda', args.gpu)
    paths = model_paths(args.model_path)
    dataset = WaterDataset_RGB(args.mode, args.dataset_path, (args.input_shape, args.input_shape))
    if len(dataset) == 0:
        raise ValueError(f'{args.dataset_path}: no labelled photograph found')
    results = []
    loader = ImageSampleLoader(dataset, device, batch_size=args.batch_size, shuffle=False, num_workers=args.num_workers,
                               seed=args.seed)
    for path in paths:
        loader.epoch = 0                               # every checkpoint sees epoch 0 of the seed: the same samples
        logs = ValidEpoch(load_checkpoint(path, device), device).run(loader)
        print(path)
        print('dice_loss - {:.4}, iou_score - {:.4}'.format(logs['dice_loss'], logs['iou_score']))          # smp's log line
        results.append({'model_path': path, 'dice_loss': logs['dice_loss'], 'iou_score': logs['iou_score']})
    best = select_best([r['iou_score'] for r in results])
    if best is None:
        print('No checkpoint scores above 0.')
    else:
        print('Best by iou_score: {} ({!r})'.format(results[best]['model_path'], results[best]['iou_score']))
    if args.json:
        with open(args.json, 'w') as f:
            json.dump({'dataset_path': args.dataset_path, 'mode': args.mode, 'input_shape': args.input_shape,
                       'batch_size': args.batch_size, 'seed': args.seed, 'samples': len(dataset), 'results': results,
                       'best': None if best is None else results[best]['model_path']}, f, indent=1)
    return results, best


if __name__ == '__main__':
    main()
