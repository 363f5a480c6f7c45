"""The training-clip kernels (``csrc/train_aug.hip``) against the NumPy restatement of Pillow's arithmetic (tests/aug_ref.py
``np_*``, pinned to Pillow 12.2.0 by tests/test_train_aug_host.py): every stage alone and the whole clip, EQUAL IN EVERY
BYTE; then the loader, the training entry point and the argument checks of the raw ABI."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest
import torch

import aug_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def aug(gpu):
    from vfloodnet_amd import train_dataset as D
    return D.ClipAugmenter(gpu)


@pytest.fixture(scope='module')
def noise():
    rng = np.random.default_rng(20200212)
    return rng.integers(0, 256, (93, 67, 3), dtype=np.uint8), rng.integers(0, 3, (93, 67), dtype=np.uint8)


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def np_jitter(a, p):
    if p.get('flip'):
        a = R.np_hflip(a)
    order, (b, c, s, shift) = p['jitter']
    for op in order:
        a = (R.np_brightness, R.np_contrast, R.np_saturation, R.np_hue)[op](a, (b, c, s, shift)[op])
    return a


def pil_jitter(a, p):
    if p.get('flip'):
        a = R.pil_hflip(a)
    order, (b, c, s, shift) = p['jitter']

    def hue(x, sh):
        hsv = R.pil_rgb2hsv(x)
        hsv[..., 0] = (hsv[..., 0].astype(np.int32) + sh) & 255
        return R.pil_hsv2rgb(hsv)
    for op in order:
        a = (R.pil_brightness, R.pil_contrast, R.pil_saturation, hue)[op](a, (b, c, s, shift)[op])
    return a


# ------------------------------------------------------------------------------------------------ stage A
def jitter_cases():
    prng = random.Random(1)
    orders = [(0, 1, 2, 3), (3, 2, 1, 0), (1, 0, 3, 2), (2, 3, 0, 1), (1, 2, 3, 0), (3, 1, 0, 2), (0, 2, 1, 3), (2, 0, 3, 1)]
    cases = [{'flip': k % 3 == 1, 'jitter': (o, (prng.uniform(0.9, 1.1), prng.uniform(0.9, 1.1), prng.uniform(0.9, 1.1), prng.choice([0, 3, 7, 249, 252])))}
             for k, o in enumerate(orders)]
    cases.append({'flip': False, 'jitter': ((0, 1, 2, 3), (0.9, 0.9, 0.9, 0))})
    cases.append({'flip': True, 'jitter': ((0, 1, 2, 3), (1.1, 1.1, 1.1, 255))})
    cases.append({'flip': False, 'jitter': ((2, 1, 0, 3), (1.0, 1.0, 1.0, 0))})          # factor 1 copies; the hue round trip still runs
    cases.append({'flip': False, 'jitter': ((1, 0, 2, 3), (1.5, 0.0, 2.0, 128))})         # outside the reference's range: both clamps
    return cases


def test_jitter_equals_numpy_and_pillow(aug, gpu, noise):
    cases = jitter_cases()
    for c in cases:
        c['crop'] = (0, 0, 1, 1)
    half = np.zeros((8, 8, 3), np.uint8)                  # the mean of L sits on 100.5
    half[:, :4], half[:, 4:] = 100, 101
    for img in (noise[0], half):
        got = aug.jitter(dev(img, gpu), cases).cpu().numpy()
        for t, c in enumerate(cases):
            ref = np_jitter(img, c)
            assert np.array_equal(got[t], ref), (t, c)
            assert np.array_equal(ref, pil_jitter(img, c)), (t, c)


def test_jitter_of_a_frame_larger_than_one_pass_of_the_grid(aug, gpu):
    """1024 blocks of 256 threads cover 262144 pixels: 600 x 500 makes the grid-stride loop take a second turn."""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (500, 600, 3), dtype=np.uint8)
    cases = [{'flip': True, 'jitter': ((2, 0, 1, 3), (1.07, 0.93, 1.02, 251)), 'crop': (0, 0, 1, 1)}]
    assert np.array_equal(aug.jitter(dev(img, gpu), cases).cpu().numpy()[0], np_jitter(img, cases[0]))


def test_hue_on_all_colours(aug, gpu):
    g = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    a = np.stack([(g >> 16) & 255, (g >> 8) & 255, g & 255], -1).astype(np.uint8)
    # both conversions over all 2^24 triples once (a holds every triple in index order), then the shift is a table look-up
    hsv = np.concatenate([R.np_rgb2hsv(a[lo:lo + 256]) for lo in range(0, 4096, 256)])
    back = np.concatenate([R.np_hsv2rgb(a[lo:lo + 256]) for lo in range(0, 4096, 256)]).reshape(-1, 3)
    cases = [{'flip': False, 'jitter': ((3, 0, 1, 2), (1.0, 1.0, 1.0, shift)), 'crop': (0, 0, 1, 1)} for shift in (249, 6)]
    got = aug.jitter(dev(a, gpu), cases).cpu().numpy()
    for t, shift in enumerate((249, 6)):
        h = (hsv[..., 0].astype(np.uint32) + shift) & 255
        ref = back[(h << 16) | (hsv[..., 1].astype(np.uint32) << 8) | hsv[..., 2]]
        assert np.array_equal(got[t], ref), shift
    small = a[::61, ::67]
    assert np.array_equal(R.np_hue(small, 249), np.ascontiguousarray(got[0][::61, ::67]))


# ------------------------------------------------------------------------------------------------ stage B
def affine_cases(W, H):
    prng = random.Random(7)

    def draw():
        return R.inverse_affine_matrix(W, H, prng.uniform(-20, 20), (float(np.round(prng.uniform(-0.1 * W, 0.1 * W))),
                                                                    float(np.round(prng.uniform(-0.1 * H, 0.1 * H)))),
                                       prng.uniform(0.9, 1.1), prng.uniform(-10, 10))
    wins = [(0, 0, 20, 25), (0, W - 25, 20, 25), (H - 20, 0, 20, 25), (H - 20, W - 25, 20, 25), (0, 0, H, W), (30, 20, 1, 1),
            (11, 3, 70, 64)]
    cases = [{'flip': k % 2 == 1, 'affine': draw(), 'crop': w} for k, w in enumerate(wins)]
    # fill pushed into the window: a large shift, a strong rotation, a zoom out
    cases.append({'flip': False, 'affine': R.inverse_affine_matrix(W, H, 0.0, (30.0, 40.0), 1.0, 5.0), 'crop': (0, 0, H, W)})
    cases.append({'flip': True, 'affine': R.inverse_affine_matrix(W, H, 45.0, (0.0, 0.0), 1.0, 0.0), 'crop': (0, 0, H, W)})
    cases.append({'flip': False, 'affine': R.inverse_affine_matrix(W, H, -20.0, (-6.0, 9.0), 0.5, -10.0), 'crop': (0, 0, H, W)})
    # m1 == m3 == 0: Pillow's nearest filter takes the scaling path (index tables)
    cases.append({'flip': False, 'affine': R.inverse_affine_matrix(W, H, 0.0, (5.0, -7.0), 1.0, 0.0), 'crop': (0, 0, H, W)})
    cases.append({'flip': True, 'affine': R.inverse_affine_matrix(W, H, 0.0, (-3.0, 4.0), 1.07, 0.0), 'crop': (2, 1, 80, 60)})
    cases.append({'flip': True, 'affine': None, 'crop': (5, 6, 50, 40)})              # no transform: the window is copied
    return cases


def test_affine_window_equals_the_cropped_full_transform(aug, gpu, noise):
    from vfloodnet_amd import train_dataset as D
    img, mask = noise
    H, W = mask.shape
    cases = affine_cases(W, H)
    assert len(cases) <= 16
    wi, wm = aug.affine(dev(img, gpu), dev(mask, gpu), cases)
    torch.cuda.synchronize()
    fills = 0
    for t, c in enumerate(cases):
        a, m = (R.np_hflip(img), R.np_hflip(mask)) if c['flip'] else (img, mask)
        if c['affine'] is not None:
            a, m = R.np_affine_bicubic(a, c['affine']), R.np_affine_nearest(m, c['affine'])
        i, j, h, w = c['crop']
        got_i, got_m = D.ClipAugmenter.window(wi, t, h, w, 3).cpu().numpy(), D.ClipAugmenter.window(wm, t, h, w, 1).cpu().numpy()
        assert np.array_equal(got_i, a[i:i + h, j:j + w]), (t, c)
        assert np.array_equal(got_m, m[i:i + h, j:j + w]), (t, c)
        fills += int((a[i:i + h, j:j + w].max(-1) == 0).sum() > 20)
        if t in (0, 7, 10):                               # Pillow itself, where it is cheap
            src = (R.pil_hflip(img), R.pil_hflip(mask)) if c['flip'] else (img, mask)
            assert np.array_equal(got_i, R.pil_affine(src[0], c['affine'], 'bicubic')[i:i + h, j:j + w])
            assert np.array_equal(got_m, R.pil_affine(src[1], c['affine'], 'nearest')[i:i + h, j:j + w])
    assert fills >= 5


# ------------------------------------------------------------------------------------------------ stage C
def crops_131x173():
    H, W = 173, 131
    fixed = [(0, 0, H, W), (0, 0, 9, 11), (0, 20, 30, 111), (40, 0, 133, 50), (173 - 12, 131 - 15, 12, 15), (10, 131 - 101, 150, 101),
             (173 - 100, 3, 100, 40), (5, 7, 16, 16), (3, 2, 40, 100), (1, 1, 171, 129), (7, 9, 100, 100), (0, 0, 40, 40)]
    prng = random.Random(11)
    out = list(fixed)
    while len(out) < 24:
        h, w = prng.randint(5, H), prng.randint(5, W)
        out.append((prng.randint(0, H - h), prng.randint(0, W - w), h, w))
    return out


@pytest.mark.parametrize('S', [16, 40, 100, 400])
def test_crop_resize_tensor_and_onehot(aug, gpu, S):
    """Stage C alone: the windows are uploaded as they are (what stage B's copy branch would leave)."""
    rng = np.random.default_rng(5)
    H, W = 173, 131
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mask = rng.integers(0, 5, (H, W), dtype=np.uint8)      # labels 0 .. 4; the object list names 3, 1 and the absent 9
    crops = crops_131x173()[{16: 0, 40: 6, 100: 12, 400: 18}[S]:][:6] + [(5, 7, 16, 16), (7, 9, 100, 100), (0, 0, 40, 40)]
    params = [{'crop': c} for c in crops]
    T = len(params)
    wi, wm = np.zeros((T, H * W * 3), np.uint8), np.zeros((T, H * W), np.uint8)
    for t, (i, j, h, w) in enumerate(crops):
        wi[t, :h * w * 3] = img[i:i + h, j:j + w].reshape(-1)
        wm[t, :h * w] = mask[i:i + h, j:j + w].reshape(-1)
    obj = [3, 1, 9]
    frames, masks = aug.resize(dev(wi, gpu), dev(wm, gpu), H, W, params, S, obj)
    assert frames.shape == (T, 3, S, S) and masks.shape == (T, 4, S, S) and frames.dtype == masks.dtype == torch.float32
    frames, masks = frames.cpu().numpy(), masks.cpu().numpy()
    for t, (i, j, h, w) in enumerate(crops):
        u8 = R.np_crop_resize_bicubic(img, i, j, h, w, S)
        lab = R.np_crop_resize_nearest(mask, i, j, h, w, S)
        assert np.array_equal(frames[t], R.np_to_tensor(u8)), (t, crops[t])
        assert np.array_equal(frames[t], u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
        assert np.array_equal(masks[t], R.np_onehot(lab, obj)), (t, crops[t])
        assert np.array_equal(masks[t].sum(0), np.ones((S, S), np.float32))
        assert np.array_equal(masks[t, 1], (lab == 3).astype(np.float32)) and np.array_equal(masks[t, 2], (lab == 1).astype(np.float32))
        assert not masks[t, 3].any()                                                     # label 9 is nowhere
        assert np.array_equal(masks[t, 0], np.isin(lab, [0, 2, 4]).astype(np.float32))   # labels outside the list: channel 0
        if t < 2:
            assert np.array_equal(u8, R.pil_crop_resize(img, i, j, h, w, S, 'bicubic'))
            assert np.array_equal(lab, R.pil_crop_resize(mask, i, j, h, w, S, 'nearest'))


def test_labels_present(aug, gpu):
    mask = np.zeros((60, 80), np.uint8)
    mask[10:30, 5:20], mask[40:, 60:], mask[0, 0], mask[59, 79] = 4, 200, 7, 255
    m = dev(mask, gpu)
    for crop, S in (((0, 0, 60, 80), 16), ((0, 0, 60, 80), 100), ((5, 0, 30, 40), 20), ((35, 50, 25, 30), 16), ((0, 30, 9, 9), 16)):
        i, j, h, w = crop
        lab = R.np_crop_resize_nearest(mask, i, j, h, w, S)
        assert aug.labels_present(m, crop, S) == [int(v) for v in np.unique(lab) if v > 0], (crop, S)


# ------------------------------------------------------------------------------------------------ the whole clip
def clip_params(W, H, seed):
    from vfloodnet_amd import train_dataset as D
    return D.draw_clip_params(random.Random(seed), W, H, 3, 0)


@pytest.mark.parametrize('shape,S,seed', [((93, 67), 16, 3), ((270, 480), 400, 4)])
def test_whole_clip_equals_the_composed_pipeline(aug, gpu, shape, S, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([(xx * 3 + yy) % 256, (yy * 2 + 40) % 256, (xx + 2 * yy) % 256], -1)
    img = np.clip(img + rng.integers(-40, 40, img.shape), 0, 255).astype(np.uint8)
    mask = ((yy > H // 2).astype(np.uint8) + 2 * ((xx > 2 * W // 3) & (yy < H // 3)).astype(np.uint8))
    params = clip_params(W, H, seed)
    params[1]['flip'], params[2]['flip'] = True, False
    assert params[0]['jitter'] is None and params[1]['affine'] is not None
    frames, masks = aug.clip(dev(img, gpu), dev(mask, gpu), params, S, [2, 1])
    f_ref, m_ref, _ = R.np_clip(img, mask, params, S, [2, 1])
    assert np.array_equal(frames.cpu().numpy(), f_ref)
    assert np.array_equal(masks.cpu().numpy(), m_ref)
    if S == 16:
        f_pil, m_pil, _ = R.pil_clip(img, mask, params, S, [2, 1])
        assert np.array_equal(f_ref, f_pil) and np.array_equal(m_ref, m_pil)


# ------------------------------------------------------------------------------------------------ loader and entry point
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = str(tmp_path_factory.mktemp('train_ds'))
    R.make_tree(root, n=3, size=(120, 90))
    return root


def collect(loader):
    return [(f.clone(), m.clone(), n, info) for f, m, n, info in loader]


def test_loader_samples(gpu, tree):
    from vfloodnet_amd import train_dataset as D
    ds = D.Water_Image_Train_DS(tree, 48, clip_n=3, max_obj_n=3)
    a = collect(D.TrainClipLoader(ds, gpu, shuffle=True, num_workers=0, seed=11))
    b = collect(D.TrainClipLoader(ds, gpu, shuffle=True, num_workers=0, seed=11))
    c = collect(D.TrainClipLoader(ds, gpu, shuffle=True, num_workers=2, seed=11))
    torch.cuda.synchronize()
    assert len(a) == len(b) == len(c) == 3 and sorted(s[3]['name'] for s in a) == sorted(ds.img_list)
    for (f, m, n, info), sb, sc in zip(a, b, c):
        assert f.shape == (1, 3, 3, 48, 48) and m.shape == (1, 3, n, 48, 48) and f.dtype == m.dtype == torch.float32
        assert f.device == m.device == gpu and isinstance(n, int)
        assert n == (1 if info['name'].endswith('002.jpg') else 3)       # image 2 has no object: passed through for train_model to skip
        assert torch.equal(m.sum(2), torch.ones_like(m[:, :, 0]))
        for other in (sb, sc):
            assert other[3] == info and other[2] == n and torch.equal(other[0], f) and torch.equal(other[1], m)
    d = collect(D.TrainClipLoader(ds, gpu, shuffle=True, num_workers=0, seed=12))
    assert any(not torch.equal(x[0], y[0]) for x, y in zip(a, d) if x[3] == y[3]) or [x[3] for x in a] != [y[3] for y in d]


def test_sample_equals_pillow_decode_and_the_composed_pipeline(gpu, tree):
    """A whole item: the device decode (JPEG and PNG) and the clip against PIL's decode and ``np_*`` with the same draws."""
    from PIL import Image
    from vfloodnet_amd import train_dataset as D
    ds = D.Water_Image_Train_DS(tree, 32, clip_n=3, max_obj_n=3)
    aug = D.ClipAugmenter(gpu)
    for idx in (0, 1):
        frames, masks, obj_n, params = D.sample_on_device(aug, ds[idx], random.Random(idx), 3, 32, 3)
        img = np.array(Image.open(ds.img_list[idx]).convert('RGB'))
        mask = np.array(Image.open(ds.mask_list[idx]).convert('P'))
        rng = random.Random(idx)                                       # the same draws, the shuffle included
        obj = []

        def first(p):
            i, j, h, w = p['crop']
            lab = R.np_crop_resize_nearest(mask, i, j, h, w, 32)
            obj[:] = [int(v) for v in np.unique(lab) if v > 0]
            rng.shuffle(obj)
        ref_params = D.draw_clip_params(rng, 120, 90, 3, 32, after_first=first)
        assert ref_params == params and obj_n == len(obj) + 1 and obj_n >= 2
        f_ref, m_ref, _ = R.np_clip(img, mask, params, 32, obj)
        assert np.array_equal(frames.cpu().numpy(), f_ref) and np.array_equal(masks.cpu().numpy(), m_ref)


def test_train_video_seg_main(gpu, tree, tmp_path, monkeypatch):
    from tools import synth
    from vfloodnet_amd import AFB_URR
    from vfloodnet_amd import train_video_seg as TV
    monkeypatch.chdir(tmp_path)                                                           # --log writes under ./logs, as the reference
    two = str(tmp_path / 'two')
    R.make_tree(two, n=2, size=(120, 90), seed=1)
    ckpt = str(tmp_path / 'start.pth')
    torch.save({'model': synth.make_state_dict(20200212), 'seed': 1}, ckpt)
    common = ['--dataset', two, '--log', '--size', '96', '--clip-n', '3']
    out = TV.main(common + ['--resume', ckpt, '--new', '--seed', '5', '--total-epochs', '1'])
    assert out['epochs'] == 1 and math.isfinite(out['loss']) and out['loss'] > 0
    assert out['model_path'].startswith('logs/level0_') and out['model_path'].endswith('/model')
    for name in ('final.pth', 'best.pth'):
        assert os.path.isfile(os.path.join(out['model_path'], name))
    assert any(n.startswith('epoch_000_loss_') for n in os.listdir(out['model_path']))
    final = os.path.join(out['model_path'], 'final.pth')
    ck = torch.load(final, map_location='cpu')
    assert set(ck) == {'epoch', 'model', 'optimizer', 'loss', 'seed'} and ck['epoch'] == 0 and ck['seed'] == 5
    assert ck['loss'] == out['loss'] and ck['optimizer']['param_groups'][0]['initial_lr'] == 1e-5
    model = AFB_URR(gpu, update_bank=True)
    model.load_state_dict(ck['model'], strict=True)
    start = synth.make_state_dict(20200212)
    assert any(not torch.equal(ck['model'][k], start[k]) for k in start)                  # the step moved the weights
    # resumed without --new (train_video_seg.py:119-124): epoch, optimizer state, best loss and seed come from the checkpoint
    resumed = str(tmp_path / 'epoch0.pth')
    os.replace(final, resumed)
    out2 = TV.main(common + ['--resume', resumed, '--scheduler-step', '1', '--total-epochs', '2'])
    assert out2['epochs'] == 1 and math.isfinite(out2['loss'])
    ck2 = torch.load(os.path.join(out2['model_path'], 'final.pth'), map_location='cpu')
    assert ck2['epoch'] == 1 and ck2['seed'] == 5
    g = ck2['optimizer']['param_groups'][0]
    assert g['initial_lr'] == 1e-5 and g['lr'] == 0.5e-5                                  # StepLR(step 1, gamma 0.5) entered epoch 1
    assert int(ck2['optimizer']['state'][0]['step']) == 2 * int(ck['optimizer']['state'][0]['step'])
    with pytest.raises(ValueError):
        TV.main(['--dataset', two])


# ------------------------------------------------------------------------------------------------ the raw ABI
def test_bad_arguments_launch_nothing(gpu):
    from vfloodnet_amd import _lib
    L = _lib.lib()
    H, W, T, S = 20, 30, 2, 8
    z = lambda *shape, dt=torch.uint8: torch.full(shape, 77, dtype=dt, device=gpu)
    src, mask = z(H, W, 3), z(H, W)
    outs = {'jit': z(T, H, W, 3), 'lsum': z(T, dt=torch.int64), 'win_img': z(T, H * W * 3), 'win_mask': z(T, H * W), 'hpass': z(T, H, S, 3),
            'frames': z(T, 3, S, S, dt=torch.float32), 'masks': z(T, 3, S, S, dt=torch.float32), 'present': z(256)}
    tabs = torch.zeros(4096, dtype=torch.int32, device=gpu)

    def good():
        d = _lib.TrainAugDesc()
        d.src, d.mask = src.data_ptr(), mask.data_ptr()
        for k in ('jit', 'lsum', 'win_img', 'win_mask', 'hpass', 'frames', 'masks'):
            setattr(d, k, outs[k].data_ptr())
        for k in ('kx_bounds', 'kx', 'ky_bounds', 'ky', 'nx', 'ny', 'aff_xtab', 'aff_ytab'):
            setattr(d, k, tabs.data_ptr())
        d.H, d.W, d.T, d.S, d.ksize_x, d.ksize_y, d.obj_n = H, W, T, S, 5, 5, 3
        d.obj_list[0], d.obj_list[1] = 1, 2
        for t in range(T):
            f = d.frame[t]
            f.jitter = f.affine = 1
            f.order[:] = [0, 1, 2, 3]
            f.brightness = f.contrast = f.saturation = 1.0
            f.m[:] = [1.0, 0.1, 0.0, -0.1, 1.0, 0.0]
            f.win_i, f.win_j, f.win_h, f.win_w = 2, 3, 10, 12
        return d
    stages = (L.vfn_train_aug_jitter, L.vfn_train_aug_affine, L.vfn_train_aug_resize)

    def bad(change, which=stages):
        for fn in which:
            d = good()
            change(d)
            assert fn(C.byref(d), None) == 1, (fn.__name__, change)                      # VFN_ERR_ARG

    def set_(**kw):
        def change(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return change

    def frame_(t, **kw):
        def change(d):
            for k, v in kw.items():
                setattr(d.frame[t], k, v)
        return change
    for fn in stages:
        assert fn(None, None) == 1
    bad(set_(src=None), stages[:2])
    bad(set_(mask=None), stages[1:2])
    bad(set_(jit=None), stages[:2])
    bad(set_(lsum=None), stages[:1])
    bad(set_(win_img=None), stages[1:])
    bad(set_(win_mask=None), stages[1:])
    for k in ('hpass', 'kx_bounds', 'kx', 'ky_bounds', 'ky', 'nx', 'ny', 'frames', 'masks'):
        bad(set_(**{k: None}), stages[2:])
    bad(set_(H=8193))
    bad(set_(W=8193))
    bad(set_(H=0))
    bad(set_(T=0))
    bad(set_(T=17))
    bad(set_(S=0), stages[2:])
    bad(set_(S=4097), stages[2:])
    bad(set_(obj_n=0), stages[2:])
    bad(set_(obj_n=12), stages[2:])
    bad(set_(ksize_x=0), stages[2:])
    bad(frame_(1, win_i=11))                                                              # rows 11 .. 20 of 20
    bad(frame_(0, win_j=19))
    bad(frame_(1, win_i=-1))
    bad(frame_(0, win_h=0))
    bad(frame_(0, win_w=31))
    bad(frame_(1, hue_shift=256), stages[:1])

    def twice(d):
        d.frame[0].order[:] = [0, 1, 1, 3]
    bad(twice, stages[:1])

    def tables_missing(d):
        d.frame[0].nearest_tables, d.aff_xtab = 1, None
    bad(tables_missing, stages[1:2])

    def far(d):
        d.frame[0].m[:] = [1.0, 0.1, 40000.0, -0.1, 1.0, 0.0]                             # beyond the 16.16 range
    bad(far, stages[1:2])
    p = outs['present']
    t4 = tabs.data_ptr()
    for args in ((None, H, W, t4, t4, S, p.data_ptr()), (mask.data_ptr(), H, W, None, t4, S, p.data_ptr()),
                 (mask.data_ptr(), H, W, t4, t4, S, None), (mask.data_ptr(), 8193, W, t4, t4, S, p.data_ptr()),
                 (mask.data_ptr(), H, W, t4, t4, 0, p.data_ptr()), (mask.data_ptr(), H, W, t4, t4, 4097, p.data_ptr())):
        assert L.vfn_train_aug_label_present(*args, None) == 1
    torch.cuda.synchronize()
    for k, v in outs.items():
        assert bool((v == 77).all()), k                                                   # nothing was launched, nothing was cleared
    # and the descriptor the checks start from is a good one
    for fn in stages:
        assert fn(C.byref(good()), None) == 0
    assert L.vfn_train_aug_label_present(mask.data_ptr(), H, W, t4, t4, S, p.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert not bool((outs['present'] == 77).all()) and not bool((outs['frames'] == 77).all())
