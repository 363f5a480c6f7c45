"""Times of the LinkNet decoder fine-tuning step (vfloodnet_amd/linknet_train.py) on one otherwise idle MI355X, HIP events
around warmed-up windows:

* ms per ``DecoderTrainer.step`` at 416 x 416, batch 4, beside ``predict_batch`` of the same batch (the inference path, which the
  training code does not touch: its figure in this tree is the parent commit's), and the ratio of the two;
* bytes/s of the four BatchNorm kernels on the 86528 x 32 and 10816 x 128 layers (the bytes each must move, computed from the
  shape), beside a plain float4 copy (``Tensor.copy_``) of the same number of bytes measured in the same run.  The tensors of one
  timed launch are rotated through a ring larger than the 256 MB last-level cache, so the rates are memory rates.

    python scripts/bench_image_train.py [--out profiles/image_train_step.txt]

``--mode encoder`` measures the step that trains the encoder as well (``ModelTrainer``, frozen BatchNorm statistics) against the
decoder-only step and ``predict_batch`` in the same job, the three alternating window by window, and the depthwise data- and
weight-gradient kernels on the two largest layers (block 2: 144 -> 160 channels, 208 x 208 -> 104 x 104; block 10: 336 -> 352
channels, 52 x 52 -> 26 x 26; 3 x 3, stride 2, batch 4) beside a copy of the same bytes (a copy of one input-sized tensor,
scaled to the kernel's byte count):

    python scripts/bench_image_train.py --mode encoder [--out profiles/image_train_encoder_step.txt]

``--mode encoder-bn`` measures the step that trains the encoder in train mode (``FullTrainer``: batch-statistics BatchNorm and
drop-connect) against the ``'statistics'`` step, the decoder-only step and ``predict_batch`` in the same job, the four alternating
window by window, and the kernels of include/vfn_encoder_bn_train.h on the expand convolution's output of block 2 (173056 x 160)
and block 10 (10816 x 352) beside a copy of the same bytes:

    python scripts/bench_image_train.py --mode encoder-bn [--out profiles/image_train_encoder_bn_step.txt]
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RING_BYTES = 640 * 1024 * 1024


def timed(fn, iters, warmup):
    """Mean milliseconds per call of fn(i) over ``iters`` calls between two events, after ``warmup`` calls."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def bench_step(dev, lines, steps, warmup):
    from tools import synth_linknet
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import DecoderTrainer
    sd = synth_linknet.make_state_dict()
    x = torch.cat([synth_linknet.frame(50 + i, 416, 416) for i in range(4)]).to(dev)
    y = (torch.rand(4, 1, 416, 416, generator=torch.Generator().manual_seed(1)) > 0.5).float().to(dev)
    model = LinknetB4.from_checkpoint(sd, dev)
    t_pred = timed(lambda i: model.predict_batch(x), steps, max(warmup, 4))          # (the third call captures the graph)
    trainer = DecoderTrainer(model, init_lr=1e-4)
    t_step = timed(lambda i: trainer.step(x, y), steps, warmup)
    spread = [timed(lambda i: trainer.step(x, y), steps, 0) for _ in range(3)]
    lines.append(f'step 416x416 batch 4: {t_step:.3f} ms per step (three more windows of {steps}: ' + ', '.join(f'{v:.3f}' for v in spread) + ')')
    lines.append(f'predict_batch 416x416 batch 4 (inference path, unchanged from the parent commit): {t_pred:.3f} ms per call')
    lines.append(f'ratio step / predict_batch: {t_step / t_pred:.2f}')


def bench_bn(dev, lines, iters, warmup):
    from vfloodnet_amd import _lib as L
    lib = L.lib()
    for M, C in ((86528, 32), (10816, 128)):
        n = M * C
        ring = max(2, RING_BYTES // (3 * n * 4))
        xs = [torch.randn(M, C, device=dev) for _ in range(ring)]
        gs = [1e-4 * torch.randn(M, C, device=dev) for _ in range(ring)]
        outs = [torch.empty(M, C, device=dev) for _ in range(ring)]
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        v = {k: torch.zeros(C, device=dev) for k in ('scale', 'shift', 'mean', 'rstd', 'dgamma', 'dbeta', 'rm', 'rv')}
        part = torch.empty(L.LNT_MAX_BLOCKS * 2 * C, dtype=torch.float64, device=dev)
        p, s = L.ptr, L.stream()

        def stats(i):
            L.check(lib.vfn_lnt_bn_stats_f32(p(xs[i % ring]), M, C, C, p(gamma), p(beta), 1e-5, 0.1, p(part), p(v['scale']), p(v['shift']),
                                             p(v['mean']), p(v['rstd']), p(v['rm']), p(v['rv']), s), 'stats')

        def apply(i):
            L.check(lib.vfn_lnt_bn_apply_f32(p(xs[i % ring]), p(v['scale']), p(v['shift']), p(outs[i % ring]), M, C, C, C, 1, s), 'apply')

        def bwd_reduce(i):
            L.check(lib.vfn_lnt_bn_bwd_reduce_f32(p(gs[i % ring]), p(xs[i % ring]), p(v['scale']), p(v['shift']), p(v['mean']), p(v['rstd']), M, C,
                                                  C, C, 1, p(part), p(v['dgamma']), p(v['dbeta']), s), 'bwd_reduce')

        def bwd_apply(i):
            L.check(lib.vfn_lnt_bn_bwd_apply_f32(p(gs[i % ring]), p(xs[i % ring]), p(v['scale']), p(v['shift']), p(v['mean']), p(v['rstd']),
                                                 p(v['dgamma']), p(v['dbeta']), p(outs[i % ring]), M, C, C, C, C, 1, s), 'bwd_apply')

        stats(0)
        lines.append(f'BatchNorm kernels on {M} x {C} (ring of {ring} tensor sets):')
        for name, fn, floats in (('stats (2 launches)', stats, n), ('apply', apply, 2 * n), ('bwd_reduce (2 launches)', bwd_reduce, 2 * n),
                                 ('bwd_apply', bwd_apply, 3 * n)):
            nbytes = floats * 4
            ms = timed(fn, iters, warmup)
            # a copy that moves the same bytes: floats / 2 read and floats / 2 written, slices of the ring's tensors
            half = floats // 2
            src = [torch.cat([xs[i], gs[i]]).view(-1)[:half] for i in range(ring)] if half > n else [t.view(-1)[:half] for t in xs]
            dst = [torch.empty(half, device=dev) for _ in range(ring)]
            ms_copy = timed(lambda i: dst[i % ring].copy_(src[i % ring]), iters, warmup)
            lines.append(f'  {name:24s} {nbytes / 1e6:7.2f} MB  {ms * 1e3:8.1f} us  {nbytes / ms / 1e6:8.1f} GB/s   '
                         f'copy of the same bytes {ms_copy * 1e3:8.1f} us  {nbytes / ms_copy / 1e6:8.1f} GB/s   kernel / copy {ms / ms_copy:.2f}')
            del src, dst


def bench_encoder_step(dev, lines, steps, warmup):
    from tools import synth_linknet
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import DecoderTrainer, ModelTrainer
    sd = synth_linknet.make_state_dict()
    x = torch.cat([synth_linknet.frame(50 + i, 416, 416) for i in range(4)]).to(dev)
    y = (torch.rand(4, 1, 416, 416, generator=torch.Generator().manual_seed(1)) > 0.5).float().to(dev)
    m_full, m_dec, m_pred = (LinknetB4.from_checkpoint(sd, dev) for _ in range(3))
    full, dec = ModelTrainer(m_full, init_lr=1e-4), DecoderTrainer(m_dec, init_lr=1e-4)
    sides = (('whole model (encoder on its running statistics)', lambda i: full.step(x, y)), ('decoder and head only', lambda i: dec.step(x, y)),
             ('predict_batch', lambda i: m_pred.predict_batch(x)))
    for _, fn in sides:
        timed(fn, 1, max(warmup, 4))
    rounds = [[timed(fn, steps, 0) for _, fn in sides] for _ in range(4)]                 # the sides alternate window by window
    best = [min(r[k] for r in rounds) for k in range(3)]
    for k, (name, _) in enumerate(sides):
        lines.append(f'416x416 batch 4, {name}: {best[k]:.3f} ms (four alternating windows of {steps}: ' + ', '.join(f'{r[k]:.3f}' for r in rounds) + ')')
    lines.append(f'ratio whole-model step / decoder-only step: {best[0] / best[1]:.2f};  whole-model step / predict_batch: {best[0] / best[2]:.2f}')
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        full._pack()
        full._pack_encoder()
    b.record()
    b.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    full.step(x, y)
    torch.cuda.synchronize()
    lines.append(f'peak device memory of one whole-model step above what is resident before it: {(torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20:.0f} MiB')
    lines.append(f'of which packing the filters from the parameters (torch operations on parameter-sized tensors): {a.elapsed_time(b) / steps:.3f} ms')


def bench_full_step(dev, lines, steps, warmup):
    from tools import synth_linknet
    from vfloodnet_amd.linknet import LinknetB4
    from vfloodnet_amd.linknet_train import DecoderTrainer, FullTrainer, ModelTrainer
    sd = synth_linknet.make_state_dict()
    x = torch.cat([synth_linknet.frame(50 + i, 416, 416) for i in range(4)]).to(dev)
    y = (torch.rand(4, 1, 416, 416, generator=torch.Generator().manual_seed(1)) > 0.5).float().to(dev)
    m_train, m_stat, m_dec, m_pred = (LinknetB4.from_checkpoint(sd, dev) for _ in range(4))
    train, stat, dec = FullTrainer(m_train, init_lr=1e-4), ModelTrainer(m_stat, init_lr=1e-4), DecoderTrainer(m_dec, init_lr=1e-4)
    sides = (('whole model, encoder in train mode (batch statistics, drop-connect drawn per step)', lambda i: train.step(x, y)),
             ('whole model, encoder on its running statistics', lambda i: stat.step(x, y)), ('decoder and head only', lambda i: dec.step(x, y)),
             ('predict_batch', lambda i: m_pred.predict_batch(x)))
    for _, fn in sides:
        timed(fn, 1, max(warmup, 4))
    rounds = [[timed(fn, steps, 0) for _, fn in sides] for _ in range(4)]                 # the sides alternate window by window
    best = [min(r[k] for r in rounds) for k in range(len(sides))]
    for k, (name, _) in enumerate(sides):
        lines.append(f'416x416 batch 4, {name}: {best[k]:.3f} ms (four alternating windows of {steps}: ' + ', '.join(f'{r[k]:.3f}' for r in rounds) + ')')
    lines.append(f"ratio train-mode step / 'statistics' step: {best[0] / best[1]:.2f};  / decoder-only step: {best[0] / best[2]:.2f};  "
                 f'/ predict_batch: {best[0] / best[3]:.2f}')
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    train.step(x, y)
    torch.cuda.synchronize()
    lines.append(f'peak device memory of one train-mode step above what is resident before it: {(torch.cuda.max_memory_allocated(dev) - base) / 2 ** 20:.0f} MiB')


def bench_bn_train(dev, lines, iters, warmup):
    from vfloodnet_amd import _lib as L
    lib = L.lib()
    B = 4
    for name, M, C in (('block 2', 173056, 160), ('block 10', 10816, 352)):
        n = M * C
        ring = max(2, RING_BYTES // (3 * n * 4))
        zs = [torch.randn(M, C, device=dev) for _ in range(ring)]
        gs = [1e-4 * torch.randn(M, C, device=dev) for _ in range(ring)]
        ys = [torch.empty(M, C, device=dev) for _ in range(ring)]
        v = {k: torch.randn(C, device=dev) for k in ('gamma', 'beta', 'rstd', 'nshift', 'fold', 'dbeta', 'dgamma', 'rm', 'rv')}
        keep = torch.tensor([1.25, 0.0, 1.25, 1.25], device=dev)
        part = torch.empty(L.ET_MAX_BLOCKS * 2 * C, dtype=torch.float64, device=dev)
        sg, sga = torch.empty(B, C, device=dev), torch.empty(B, C, device=dev)
        p, s = L.ptr, L.stream()

        def stats(i):
            L.check(lib.vfn_et_bn_stats_f32(p(zs[i % ring]), M, C, C, p(v['gamma']), 1e-3, 0.01, p(part), p(v['rstd']), p(v['nshift']), p(v['fold']),
                                            p(v['rm']), p(v['rv']), C, s), 'stats')

        def norm(i):                                              # as the trainer runs it: xhat in place of z, y beside it
            L.check(lib.vfn_et_bn_norm_f32(p(zs[i % ring]), p(v['rstd']), p(v['nshift']), p(v['gamma']), p(v['beta']), p(keep), None, p(zs[i % ring]),
                                           p(ys[i % ring]), B, M // B, C, C, C, C, C, 1, s), 'norm')

        def center(i):                                            # in place, no scale: the expand and depthwise BatchNorms
            L.check(lib.vfn_et_bn_center_f32(p(gs[i % ring]), p(zs[i % ring]), None, p(v['dbeta']), p(v['dgamma']), p(gs[i % ring]), B, M // B, C, C, C,
                                             C, s), 'center')

        def center_keep(i):                                       # out of place under the drop-connect scale: the project BatchNorm
            L.check(lib.vfn_et_bn_center_f32(p(gs[i % ring]), p(zs[i % ring]), p(keep), p(v['dbeta']), p(v['dgamma']), p(ys[i % ring]), B, M // B, C, C,
                                             C, C, s), 'center')

        def sums(i):
            L.check(lib.vfn_et_bn_sums_f32(p(sg), p(sga), p(keep), p(v['dbeta']), p(v['dgamma']), B, C, s), 'sums')

        lines.append(f'train-mode BatchNorm kernels on the expand output of {name}: {M} x {C} (ring of {ring} tensor sets):')
        for kname, fn, floats in (('stats (2 launches)', stats, n), ('norm (xhat in place, y)', norm, 3 * n), ('center in place', center, 3 * n),
                                  ('center under keep', center_keep, 3 * n)):
            nbytes = floats * 4
            ms = timed(fn, iters, warmup)
            half = min(floats // 2, n)
            ms_copy = timed(lambda i: ys[i % ring].view(-1)[:half].copy_(gs[i % ring].view(-1)[:half]), iters, warmup) * (floats / 2) / half
            lines.append(f'  {kname:28s} {nbytes / 1e6:7.2f} MB  {ms * 1e3:8.1f} us  {nbytes / ms / 1e6:8.1f} GB/s   '
                         f'copy of the same bytes {ms_copy * 1e3:8.1f} us  {nbytes / ms_copy / 1e6:8.1f} GB/s   kernel / copy {ms / ms_copy:.2f}')
        lines.append(f'  sums under keep ([{B}][{C}], parameter-sized): {timed(sums, iters, warmup) * 1e3:.1f} us')
        del zs, gs, ys


def bench_depthwise(dev, lines, iters, warmup):
    from vfloodnet_amd import _lib as L
    lib = L.lib()
    for name, N, H, C, k, s_ in (('block 2', 4, 208, 160, 3, 2), ('block 10', 4, 52, 352, 3, 2)):
        Ho = H // s_
        Mi, Mo = N * H * H, N * Ho * Ho
        ring = max(2, RING_BYTES // ((2 * Mi + Mo) * C * 4))
        ys = [torch.randn(Mi, C, device=dev) for _ in range(ring)]
        gs = [1e-4 * torch.randn(Mo, C, device=dev) for _ in range(ring)]
        gxs = [torch.empty(Mi, C, device=dev) for _ in range(ring)]
        w, dw = torch.randn(k * k, C, device=dev), torch.empty(k * k, C, device=dev)
        part = torch.empty(L.ET_MAX_BLOCKS * k * k * C, dtype=torch.float64, device=dev)
        p, st = L.ptr, L.stream()

        def dgrad(i):
            L.check(lib.vfn_et_dw_dgrad_f32(p(gs[i % ring]), p(w), p(ys[i % ring]), p(gxs[i % ring]), N, H, H, C, C, C, C, k, s_, 0, Ho, Ho, 1, st), 'dgrad')

        def wgrad(i):
            L.check(lib.vfn_et_dw_wgrad_f32(p(gs[i % ring]), p(ys[i % ring]), p(part), p(dw), N, H, H, C, C, C, k, s_, 0, Ho, Ho, 1, st), 'wgrad')

        lines.append(f'depthwise kernels of {name}: {N} x {H} x {H} x {C} -> {Ho} x {Ho}, {k} x {k} / stride {s_}, swish on the input (ring of {ring} tensor sets):')
        for kname, fn, floats in (('data gradient', dgrad, (Mo + 2 * Mi) * C), ('weight gradient (2 launches)', wgrad, (Mo + Mi) * C)):
            nbytes = floats * 4
            ms = timed(fn, iters, warmup)
            half = min(floats // 2, Mi * C)
            ms_copy = timed(lambda i: gxs[i % ring].view(-1)[:half].copy_(ys[i % ring].view(-1)[:half]), iters, warmup) * (floats / 2) / half
            lines.append(f'  {kname:28s} {nbytes / 1e6:7.2f} MB  {ms * 1e3:8.1f} us  {nbytes / ms / 1e6:8.1f} GB/s   '
                         f'copy of the same bytes {ms_copy * 1e3:8.1f} us  {nbytes / ms_copy / 1e6:8.1f} GB/s   kernel / copy {ms / ms_copy:.2f}')
        del ys, gs, gxs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('decoder', 'encoder', 'encoder-bn'), default='decoder')
    ap.add_argument('--out', default=None)
    ap.add_argument('--steps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--iters', type=int, default=200)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_image_train.py measures on the GPU only')
    dev = torch.device('cuda', 0)
    lines = [f'{torch.cuda.get_device_name(0)}; HIP events; step windows of {args.steps} after {args.warmup} warm-up steps; '
             f'kernel windows of {args.iters} launches after 20']
    with torch.cuda.device(dev):
        if args.mode == 'encoder-bn':
            bench_full_step(dev, lines, args.steps, args.warmup)
            bench_bn_train(dev, lines, min(args.iters, 100), 20)
        elif args.mode == 'encoder':
            bench_encoder_step(dev, lines, args.steps, args.warmup)
            bench_depthwise(dev, lines, min(args.iters, 100), 20)
        else:
            bench_step(dev, lines, args.steps, args.warmup)
            bench_bn(dev, lines, args.iters, 20)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text)


if __name__ == '__main__':
    main()
