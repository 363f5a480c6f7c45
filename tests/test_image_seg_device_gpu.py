"""The device image-segmentation pipeline on the GPU: the two resize kernels against their NumPy restatements byte for byte
(tests/imgseg_ref.py; the restatements are pinned to Pillow and torch in tests/test_image_seg_device_host.py), LinkNet at batch
B (``predict_batch``) against the float64 oracle and against its own batch-1 path, and ``test_waterseg(pipeline='device')``
end to end against the reference's files (tests/golden/image_seg_c1.npz, written by the reference's ``predict_pil`` around ``tools/standin.StandIn``).

LinkNet tolerances are those of tests/test_linknet.py (logits within 2e-3 of float64, probabilities within 5e-4, labels equal
away from |logit| < 5e-3); a batched logit and its batch-1 twin are each within 2e-3 of the same float64 value and are held
to 2e-3 of each other."""
import ctypes as C
import os
import struct
import zlib

import numpy as np
import pytest
import torch
from PIL import Image

import imgseg_ref as R

pytestmark = pytest.mark.gpu


# =============================================================================================== (a) resize + normalise
def _resize_norm(image_seg, a, x, b, gpu):
    image_seg.resize_norm_device(torch.from_numpy(a).to(gpu), x, b)


@pytest.mark.parametrize('src,dst', R.RESIZE_CASES)
def test_resize_norm_kernel_equals_restatement(gpu, src, dst):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    a = R.photo(src[0] * 1000 + src[1], *src)
    x = torch.full((1, 3) + dst, float('nan'), device=gpu)
    _resize_norm(image_seg, a, x, 0, gpu)
    want = R.np_norm(R.np_resize_bilinear(a, *dst))
    assert np.array_equal(x[0].cpu().numpy().view(np.uint32), want.view(np.uint32))


def test_resize_norm_slots_of_a_batch(gpu):
    """Three differently sized photographs into the three slots of one batch, out of order: each slot holds its own image
    and a write leaves the other slots alone."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    dst = (32, 64)
    imgs = [R.photo(10 + i, *hw) for i, hw in enumerate([(95, 131), (20, 24), (40, 64)])]
    x = torch.full((3, 3) + dst, float('nan'), device=gpu)
    for b in (2, 0):
        _resize_norm(image_seg, imgs[b], x, b, gpu)
    assert torch.isnan(x[1]).all()
    _resize_norm(image_seg, imgs[1], x, 1, gpu)
    for b in range(3):
        want = R.np_norm(R.np_resize_bilinear(imgs[b], *dst))
        assert np.array_equal(x[b].cpu().numpy().view(np.uint32), want.view(np.uint32)), b


def test_resize_norm_equals_norm_imagenet_on_the_golden_frame(gpu):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    g = np.load(R.GOLD)
    a = g['small_frame_u8']
    x = torch.empty(1, 3, 416, 416, device=gpu)
    _resize_norm(image_seg, a, x, 0, gpu)
    want = image_seg.norm_imagenet(Image.fromarray(a), (416, 416))
    assert torch.equal(x[0].cpu(), want) and np.array_equal(x[0].cpu().numpy()[:, ::16, ::16], g['small_norm'])


def test_new_entry_points_refuse_bad_arguments(gpu):
    """VFN_ERR_ARG and no launch: the outputs keep their sentinels."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib
    from vfloodnet_amd._lib import ptr, stream
    L = _lib.lib()
    src = torch.zeros(8, 8, 3, dtype=torch.uint8, device=gpu)
    x = torch.full((2, 3, 8, 8), 7.0, device=gpu)
    f3 = C.c_float * 3
    m, s0, s1 = f3(0.5, 0.5, 0.5), f3(0.25, 0.0, 0.25), f3(0.25, 0.25, 0.25)
    rn = lambda *a: L.vfn_imgseg_resize_norm(*a, stream())
    assert rn(ptr(src), 8, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 2, 8, 8, m, s1) == 1         # slot outside the batch
    assert rn(ptr(src), 8, 8, None, None, None, 0, None, None, 0, ptr(x), 2, -1, 8, 8, m, s1) == 1
    assert rn(None, 8, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 8, m, s1) == 1
    assert rn(ptr(src), 8, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 8, m, s0) == 1          # std 0
    assert rn(ptr(src), 8, 16, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 8, m, s1) == 1         # a pass without tables
    assert rn(ptr(src), 16, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 8, m, s1) == 1
    assert rn(ptr(src), 8, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 4097, m, s1) == 1
    assert rn(ptr(src), 8193, 8, None, None, None, 0, None, None, 0, ptr(x), 2, 0, 8, 8, m, s1) == 1
    lab = torch.full((8, 8), 9, dtype=torch.uint8, device=gpu)
    p = torch.zeros(4, 4, device=gpu)
    assert L.vfn_imgseg_upsample_round(None, 4, 4, ptr(lab), 8, 8, stream()) == 1
    assert L.vfn_imgseg_upsample_round(ptr(p), 0, 4, ptr(lab), 8, 8, stream()) == 1
    assert L.vfn_imgseg_upsample_round(ptr(p), 4, 4, ptr(lab), 8, 8193, stream()) == 1
    g = torch.full((2, 8), 3.0, device=gpu)
    assert L.vfn_ln_colsum_batch_f32(ptr(x), 2, 4, 6, 8, ptr(g), 1, stream()) == 1                         # C % 4
    assert L.vfn_ln_colsum_batch_f32(ptr(x), 2, 4, 8, 8, ptr(g), 0, stream()) == 1
    assert L.vfn_ln_se_gate_batch_f32(ptr(g), 1, 1.0, ptr(p), ptr(p), ptr(p), ptr(p), ptr(g), 2, 8, 257, 8, stream()) == 1
    assert L.vfn_ln_se_gate_batch_f32(ptr(g), 1, 1.0, ptr(p), ptr(p), ptr(p), ptr(p), ptr(g), 2, 8, 2, 4100, stream()) == 1
    assert L.vfn_ln_scale_rows_f32(ptr(x), ptr(g), 2, 4, 8, 6, stream()) == 1                              # ld < C
    assert L.vfn_ln_scale_rows_f32(ptr(x), None, 2, 4, 8, 8, stream()) == 1
    torch.cuda.synchronize()
    assert (x == 7.0).all() and (lab == 9).all() and (g == 3.0).all()


# =============================================================================================== (b) enlargement + round
@pytest.mark.parametrize('hw,HW', [((32, 32), (37, 61)), ((64, 96), (120, 214)), ((48, 40), (30, 33))])
def test_upsample_round_kernel_equals_restatement(gpu, hw, HW):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    p = R.smooth_map(hw[0], *hw)
    got = image_seg.upsample_round_device(torch.from_numpy(p).to(gpu), *HW).cpu().numpy()
    assert np.array_equal(got, R.np_upsample_round(p, *HW))


def test_upsample_round_kernel_on_the_standin_map(gpu):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    p, H, W = R.standin_prob('small')
    got = image_seg.upsample_round_device(torch.from_numpy(p).to(gpu), H, W).cpu().numpy()
    assert np.array_equal(got, R.np_upsample_round(p, H, W))
    half = torch.full((4, 4), 0.5, device=gpu)
    assert not image_seg.upsample_round_device(half, 9, 7).any()                 # halves to even


# =============================================================================================== (c) LinkNet at batch B
@pytest.fixture(scope='module')
def linknet(gpu):
    from tools import synth_linknet as S
    from vfloodnet_amd.linknet import LinknetB4
    sd = S.make_state_dict()
    return sd, {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}, LinknetB4.from_checkpoint(sd, gpu)


def _batch(H, W):
    from tools import synth_linknet as S
    return torch.cat([S.frame(seed, H, W) for seed in (3, 4, 11)], 0)


def _check_against_oracle(z, z_ref, what):
    err = (z - z_ref).abs().max().item()
    dp = (torch.sigmoid(z) - torch.sigmoid(z_ref)).abs().max().item()
    print(f'{what}: max |dlogit| {err:.2e}, max |dprob| {dp:.2e}')
    assert err < 2e-3 and dp < 5e-4
    sure = z_ref.abs() > 5e-3
    assert torch.equal((z > 0)[sure], (z_ref > 0)[sure])


@pytest.mark.parametrize('H,W', [(32, 32), (64, 96)])
def test_linknet_batch_vs_oracle_and_batch_one(gpu, linknet, H, W):
    from oracle import linknet_ref as LR
    from vfloodnet_amd import engine as E
    sd, sd64, model = linknet
    x = _batch(H, W)
    assert not torch.equal(x[0], x[1]) and not torch.equal(x[1], x[2])
    with torch.no_grad():
        z_ref = torch.cat([LR.logits(sd64, x[i:i + 1].double()) for i in range(3)], 0)
    xg = x.to(gpu)
    model._graphs.clear()
    model._graph_runs.clear()
    single = torch.cat([model.predict(xg[i:i + 1], logits=True) for i in range(3)], 0).cpu().double()
    calls = []
    for n in range(4):                                                # third call: capture + first replay; fourth: replay
        z = model.predict_batch(xg, logits=True)
        assert z.shape == (3, 1, H, W)
        calls.append(z.cpu().double())
        for i in range(3):
            _check_against_oracle(calls[-1][i], z_ref[i], f'linknet B=3 {H}x{W} call {n} image {i}')
        d1 = (calls[-1] - single).abs().max().item()
        print(f'linknet B=3 {H}x{W} call {n}: max |batched - batch-1 logit| {d1:.2e}')
        assert d1 < 2e-3
    if E._GRAPHS:
        assert (3, H, W, True) in model._graphs                    # a graph per (B, H, W, logits)
        assert torch.equal(calls[0], calls[2]) and torch.equal(calls[0], calls[3])
    p = model.predict_batch(xg).cpu().double()
    assert (p - torch.sigmoid(z_ref)).abs().max() < 5e-4
    # predict itself keeps its contract: a batch is the single-image results bit for bit
    assert torch.equal(model.predict(xg, logits=True).cpu().double(), single)
    # a permuted batch permutes the result: nothing leaks between images
    zp = model.predict_batch(xg[[2, 0, 1]].contiguous(), logits=True).cpu().double()
    assert torch.equal(zp, calls[0][[2, 0, 1]])


def test_linknet_batch_gates_are_per_image(gpu, linknet):
    _, _, model = linknet
    xg = _batch(64, 96).to(gpu)
    P = model._packed or model._pack()
    gates = []
    with torch.no_grad():
        model._predict_eager(P, xg, True, gates=gates)
    assert len(gates) == 32
    for k, g in enumerate(gates):
        g = g.cpu()
        assert g.shape[0] == 3 and ((g >= 0) & (g <= 1)).all()
        assert not torch.equal(g[0], g[1]) and not torch.equal(g[1], g[2]) and not torch.equal(g[0], g[2]), k


def test_linknet_launch_list_does_not_depend_on_the_batch(gpu, linknet, monkeypatch):
    """Every launcher call of the eager list, counted by name through a wrapper around the loaded library: the same for B = 2
    and B = 3, and one list, not B of them."""
    from collections import Counter
    from vfloodnet_amd import _lib
    _, _, model = linknet
    P = model._packed or model._pack()
    real = _lib.lib()
    counts = Counter()

    class Counting:
        def __getattr__(self, name):
            fn = getattr(real, name)
            if not name.startswith('vfn_'):
                return fn

            def call(*a):
                counts[name] += 1
                return fn(*a)
            return call
    monkeypatch.setattr(_lib, 'lib', lambda: Counting())
    per_batch = {}
    for B in (1, 2, 3):
        counts.clear()
        with torch.no_grad():
            model._predict_eager(P, _batch(64, 96)[:B].to(gpu), True)
        per_batch[B] = dict(counts)
    torch.cuda.synchronize()
    launchers = {k: v for k, v in per_batch[3].items() if 'cfg' not in k}
    assert launchers == {k: v for k, v in per_batch[2].items() if 'cfg' not in k}
    assert launchers['vfn_ln_scale_rows_f32'] == launchers['vfn_ln_colsum_batch_f32'] == launchers['vfn_ln_se_gate_batch_f32'] == 32
    assert 'vfn_ln_scale_cols_f32' not in launchers and per_batch[1]['vfn_ln_scale_cols_f32'] == 32
    assert sum(launchers.values()) <= sum(v for k, v in per_batch[1].items() if 'cfg' not in k)


# =============================================================================================== end to end
def _golden_frame(name):
    from tools import synth
    g = np.load(R.GOLD)
    seed, H, W = [int(x) for x in g[f'{name}_seed_hw']]
    frames, _ = synth.clip(seed, 1, H, W)
    return (frames[0] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()


def _write(u8, path):
    if str(path).endswith('.jpg'):
        Image.fromarray(u8).save(str(path), quality=92)
    else:
        Image.fromarray(u8).save(str(path))


def _host_maps(path):
    """What predict_pil computes for the file on the host: (the photograph's bytes, the stand-in's probability map, the label
    map before postprocessing_pred)."""
    from vfloodnet_amd import image_seg
    from tools.standin import StandIn
    img = image_seg.load_image_in_PIL(str(path))
    u8 = np.array(img)
    prob = StandIn().predict(image_seg.norm_imagenet(img, (416, 416)).unsqueeze(0))
    pre = torch.nn.functional.interpolate(prob, size=list(u8.shape[:2]), mode='bilinear', align_corners=False)
    return u8, prob[0, 0].numpy(), pre.squeeze().round().numpy().astype(np.uint8)


def _check_outputs(out_dir, name, stem, src_path, runner, golden=None):
    """Everything the issue asks of one image's files; returns (mask, overlay) as arrays."""
    from vfloodnet_amd.data import add_overlay, postprocessing_pred
    g = np.load(R.GOLD)
    mask_img = Image.open(os.path.join(out_dir, name, 'mask', stem + '.png'))
    ov_img = Image.open(os.path.join(out_dir, name, 'overlay', stem + '.png'))
    u8, prob, host_pre = _host_maps(src_path)
    H, W = u8.shape[:2]
    assert mask_img.mode == 'P' and mask_img.size == (W, H) and ov_img.mode == 'RGB' and ov_img.size == (W, H)
    assert mask_img.getpalette()[:768] == [int(v) for v in g['c1_palette']]
    mask, ov = np.array(mask_img), np.array(ov_img)
    band = R.in_band(prob, H, W)
    pre_dev, post_dev = (t.cpu().numpy() for t in runner.kept[stem])
    flipped = pre_dev != host_pre
    print(f'{stem}: {int(flipped.sum())} pre-CCL labels differ from the host, {int(band.sum())} of {band.size} pixels in the band')
    assert not (flipped & ~band).any()
    assert np.array_equal(pre_dev, R.np_upsample_round(prob, H, W))
    assert np.array_equal(mask, post_dev) and np.array_equal(mask, postprocessing_pred(pre_dev))
    bgr = np.ascontiguousarray(u8[..., ::-1])
    assert np.array_equal(ov, add_overlay(bgr, mask)[..., ::-1])
    if golden is not None:
        want = np.unpackbits(g[f'{golden}_labels'], axis=-1)[:, :W]
        assert not ((mask != want) & ~band).any()
        if not flipped.any():
            assert np.array_equal(mask, want) and zlib.crc32(ov.tobytes()) == int(g[f'{golden}_overlay_crc'])
            if golden == 'small':
                assert np.array_equal(ov, g['small_overlay'])
    return mask, ov


@pytest.mark.parametrize('name,ext', [('c1', 'png'), ('small', 'png'), ('c1', 'jpg'), ('small', 'jpg')])
def test_device_pipeline_single_file_matches_reference(gpu, tmp_path, name, ext):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    from tools.standin import StandIn
    src = tmp_path / f'{name}.{ext}'
    _write(_golden_frame(name), src)
    runner = image_seg.test_waterseg('unused.pth', str(src), name, str(tmp_path / 'out'), gpu, model=StandIn(), pipeline='device',
                                     keep=True)
    assert runner.predict_calls == 1
    _check_outputs(str(tmp_path / 'out'), name, name, src, runner, golden=name if ext == 'png' else None)


def test_device_pipeline_folder_of_two_sizes_in_one_batch(gpu, tmp_path):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    from tools.standin import StandIn
    folder = tmp_path / 'in'
    folder.mkdir()
    for name in ('c1', 'small'):
        _write(_golden_frame(name), folder / f'{name}.png')
    runner = image_seg.test_waterseg('unused.pth', str(folder), 'both', str(tmp_path / 'out'), gpu, model=StandIn(), pipeline='device',
                                     batch=2, keep=True)
    assert runner.predict_calls == 1                       # both photographs, of different sizes, in one batch
    for name in ('c1', 'small'):
        _check_outputs(str(tmp_path / 'out'), 'both', name, folder / f'{name}.png', runner, golden=name)


def _adam7_png(u8):
    """An interlaced (Adam7) 8-bit RGB PNG of uint8 [H, W, 3], filter type 0 on every scanline (Pillow reads interlaced files
    and writes none)."""
    H, W, _ = u8.shape
    raw = b''
    for xs, ys, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = u8[ys::dy, xs::dx]
        if sub.shape[0] and sub.shape[1]:
            raw += b''.join(b'\x00' + np.ascontiguousarray(row).tobytes() for row in sub)
    chunk = lambda tag, body: struct.pack('>I', len(body)) + tag + body + struct.pack('>I', zlib.crc32(tag + body) & 0xffffffff)
    return (b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', struct.pack('>IIBBBBB', W, H, 8, 2, 0, 0, 1)) + chunk(b'IDAT', zlib.compress(raw))
            + chunk(b'IEND', b''))


def test_device_pipeline_short_last_batch_and_pil_fallback(gpu, tmp_path):
    """Five photographs of five sizes, batch 4 (a short last batch), one of them an interlaced PNG the device decoder refuses
    (decoded by PIL in the loader, uploaded): five masks and five overlays, each equal to the image's own single run."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg, png_decode
    from tools.standin import StandIn
    folder = tmp_path / 'in'
    folder.mkdir()
    sizes = [(60, 80), (75, 101), (48, 130), (96, 64), (57, 91)]
    files = []
    for i, hw in enumerate(sizes):
        a = R.photo(40 + i, *hw)
        a[..., 2] = np.clip(a[..., 2].astype(np.int32) + np.linspace(-90, 90, hw[1]).astype(np.int32)[None, :], 0, 255)
        path = folder / (f'img{i}.jpg' if i in (1, 3) else f'img{i}.png')
        if i == 2:
            path.write_bytes(_adam7_png(a))
            assert np.array_equal(np.array(Image.open(str(path)).convert('RGB')), a)
            with pytest.raises(RuntimeError):
                png_decode.inflate(path.read_bytes())
        else:
            _write(a, path)
        files.append(path)
    runner = image_seg.test_waterseg('unused.pth', str(folder), 'five', str(tmp_path / 'out'), gpu, model=StandIn(), pipeline='device',
                                     batch=4, keep=True)
    assert runner.predict_calls == 2
    out = tmp_path / 'out' / 'five'
    assert sorted(os.listdir(out / 'mask')) == sorted(os.listdir(out / 'overlay')) == sorted(f'img{i}.png' for i in range(5))
    for i, path in enumerate(files):
        mask, ov = _check_outputs(str(tmp_path / 'out'), 'five', f'img{i}', path, runner)
        one = image_seg.ImageSegRunner(StandIn(), gpu, batch=1, load_workers=0, keep=True)
        (tmp_path / f'm{i}').mkdir()
        (tmp_path / f'o{i}').mkdir()
        one.run([str(path)], str(tmp_path / f'm{i}'), str(tmp_path / f'o{i}'))
        assert np.array_equal(np.array(Image.open(str(tmp_path / f'm{i}' / f'img{i}.png'))), mask)
        assert np.array_equal(np.array(Image.open(str(tmp_path / f'o{i}' / f'img{i}.png'))), ov)


def test_device_pipeline_with_the_hip_model_batches_predict(gpu, tmp_path, linknet):
    """LinknetB4 behind the runner: three photographs, batch 2 -> two predict calls on batches of 2 and 1, and the masks are
    the ones the host pipeline writes with the same model, up to pixels whose enlarged probability is near 0.5 (the batched
    and the batch-1 network differ in their last bits, the two enlargements inside the band)."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    _, _, model = linknet
    folder = tmp_path / 'in'
    folder.mkdir()
    from tools import synth
    for i, hw in enumerate([(120, 214), (96, 160), (150, 110)]):
        f0, _ = synth.frame0(20 + i, *hw)
        _write((f0.permute(1, 2, 0).numpy() * 255).astype(np.uint8), folder / f'p{i}.{"jpg" if i == 1 else "png"}')
    seen = []
    real, real_b = model.predict, model.predict_batch
    model.predict = lambda x, *a, **k: (seen.append(tuple(x.shape)), real(x, *a, **k))[1]
    model.predict_batch = lambda x, *a, **k: (seen.append(tuple(x.shape)), real_b(x, *a, **k))[1]
    try:
        image_seg.test_waterseg('unused.pth', str(folder), 'dev', str(tmp_path / 'out'), gpu, model=model, pipeline='device', batch=2)
    finally:
        del model.predict, model.predict_batch
    assert seen.count((2, 3, 416, 416)) == 1 and set(seen) == {(1, 3, 416, 416), (2, 3, 416, 416)}
    image_seg.test_waterseg('unused.pth', str(folder), 'host', str(tmp_path / 'out'), gpu, model=model)
    for i in range(3):
        d = np.array(Image.open(str(tmp_path / 'out' / 'dev' / 'mask' / f'p{i}.png')))
        h = np.array(Image.open(str(tmp_path / 'out' / 'host' / 'mask' / f'p{i}.png')))
        assert d.shape == h.shape and set(np.unique(d)) <= {0, 1} and (d != h).mean() < 2e-3
        assert (tmp_path / 'out' / 'dev' / 'overlay' / f'p{i}.png').exists()
