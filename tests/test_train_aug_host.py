"""The arithmetic of the training augmentation on the CPU: the NumPy restatement the GPU tests compare against
(tests/aug_ref.py ``np_*``) equals Pillow (``pil_*``) byte for byte -- this pins ``np_*`` to the installed Pillow (12.2.0) --
and the host half of ``vfloodnet_amd.train_dataset`` (tables, random draws, the dataset's file listing, the CLI parser)."""
import math
import os
import random

import numpy as np
import pytest
from PIL import Image

import aug_ref as R
from aug_ref import make_tree


@pytest.fixture(scope='module')
def noise():
    rng = np.random.default_rng(20200212)
    return rng.integers(0, 256, (93, 67, 3), dtype=np.uint8), rng.integers(0, 3, (93, 67), dtype=np.uint8)


def reference_draw(prng, W, H):
    return R.inverse_affine_matrix(W, H, prng.uniform(-20, 20), (float(np.round(prng.uniform(-0.1 * W, 0.1 * W))),
                                                                float(np.round(prng.uniform(-0.1 * H, 0.1 * H)))),
                                   prng.uniform(0.9, 1.1), prng.uniform(-10, 10))


def test_affine_equals_pillow(noise):
    img, mask = noise
    H, W = mask.shape
    prng = random.Random(7)
    mats = [reference_draw(prng, W, H) for _ in range(100)]
    mats.append(R.inverse_affine_matrix(W, H, 0.0, (5.0, -7.0), 1.0, 0.0))          # pure integer translation
    mats.append(R.inverse_affine_matrix(W, H, 0.0, (-3.0, 4.0), 1.07, 0.0))         # m1 == m3 == 0: Pillow's scaling path
    assert mats[100][1] == 0 and mats[100][3] == 0 and mats[100][0] == 1.0
    for m in mats:
        assert np.array_equal(R.np_affine_bicubic(img, m), R.pil_affine(img, m, 'bicubic')), m
        assert np.array_equal(R.np_affine_nearest(mask, m), R.pil_affine(mask, m, 'nearest')), m


def crops_131x173():
    """(i, j, h, w) of a 173-row, 131-column image: narrower and wider than every S, touching each border."""
    H, W = 173, 131
    fixed = [(0, 0, H, W), (0, 0, 9, 11), (0, 20, 30, 111), (40, 0, 133, 50), (173 - 12, 131 - 15, 12, 15), (10, 131 - 101, 150, 101),
             (173 - 100, 3, 100, 40), (5, 7, 16, 16), (3, 2, 40, 100), (1, 1, 171, 129)]
    prng = random.Random(11)
    out = list(fixed)
    while len(out) < 44:
        h, w = prng.randint(5, H), prng.randint(5, W)
        out.append((prng.randint(0, H - h), prng.randint(0, W - w), h, w))
    return out


def test_crop_resize_equals_pillow():
    from vfloodnet_amd import train_dataset as D
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (173, 131, 3), dtype=np.uint8)
    mask = rng.integers(0, 4, (173, 131), dtype=np.uint8)
    crops = crops_131x173()
    assert len(crops) >= 40
    sizes = (16, 40, 100, 400)
    assert any(c[3] < 16 for c in crops) and any(c[3] > 100 for c in crops) and any(c[2] < 16 for c in crops)
    assert any(c[0] == 0 for c in crops) and any(c[1] == 0 for c in crops)
    assert any(c[0] + c[2] == 173 for c in crops) and any(c[1] + c[3] == 131 for c in crops)
    for n, (i, j, h, w) in enumerate(crops):
        S = sizes[n % 4]
        ref = R.pil_crop_resize(img, i, j, h, w, S, 'bicubic')
        assert np.array_equal(R.np_crop_resize_bicubic(img, i, j, h, w, S), ref), (i, j, h, w, S)
        ref_m = R.pil_crop_resize(mask, i, j, h, w, S, 'nearest')
        assert np.array_equal(R.np_crop_resize_nearest(mask, i, j, h, w, S), ref_m), (i, j, h, w, S)
        # the tables the package uploads, applied in NumPy (both passes always: a pass over equal sizes is the identity)
        c = img[i:i + h, j:j + w]
        bx, kx = D.resize_tables(w, S)
        by, ky = D.resize_tables(h, S)
        got = R.np_resize_pass(R.np_resize_pass(c, bx, kx, axis=1), by, ky, axis=0)
        assert np.array_equal(got, ref), (i, j, h, w, S)
        xt, yt = D.nearest_table(w / S, 0.0, S, w), D.nearest_table(h / S, 0.0, S, h)
        assert xt.min() >= 0 and yt.min() >= 0
        assert np.array_equal(mask[i:i + h, j:j + w][yt[:, None], xt[None, :]], ref_m), (i, j, h, w, S)


def test_resize_tables_equal_the_sequential_form():
    from vfloodnet_amd import train_dataset as D
    for n_in, n_out in ((131, 16), (16, 16), (9, 400), (1080, 400), (400, 399), (5, 7), (1920, 400)):
        b, k = D.resize_tables(n_in, n_out)
        b2, k2 = R.np_resize_coeffs(n_in, n_out)
        assert np.array_equal(b, b2) and np.array_equal(k, k2), (n_in, n_out)
    for a0, a2, n_out, n_in in ((131 / 16, 0.0, 16, 131), (0.9345794392523364, -2.48, 67, 67), (1.0, 5.0, 67, 67), (0.3, 0.0, 400, 120)):
        assert np.array_equal(D.nearest_table(a0, a2, n_out, n_in), R.nearest_scale_table(a0, a2, n_out, n_in))


def half_mean_image():
    """Uniform image whose mean of L sits exactly on x.5: half the pixels L = 100, half L = 101."""
    a = np.zeros((8, 8, 3), np.uint8)
    a[:, :4], a[:, 4:] = 100, 101
    assert R.np_L(a).sum() * 2 == (100 + 101) * 64
    return a


@pytest.mark.parametrize('factor', [0.9, 1.0, 1.1])
def test_blends_equal_pillow(noise, factor):
    for a in (noise[0], half_mean_image()):
        assert np.array_equal(R.np_brightness(a, factor), R.pil_brightness(a, factor))
        assert np.array_equal(R.np_contrast(a, factor), R.pil_contrast(a, factor))
        assert np.array_equal(R.np_saturation(a, factor), R.pil_saturation(a, factor))
        assert np.array_equal(R.np_hflip(a), R.pil_hflip(a))
    assert R.np_contrast_mean(half_mean_image()) == 101


def test_hsv_equals_pillow_on_all_colours():
    g = np.arange(1 << 24, dtype=np.uint32).reshape(4096, 4096)
    a = np.stack([(g >> 16) & 255, (g >> 8) & 255, g & 255], -1).astype(np.uint8)
    hsv = R.pil_rgb2hsv(a)
    rgb = R.pil_hsv2rgb(a)
    for lo in range(0, 4096, 256):                                   # (in slabs: the restatement holds float64 temporaries)
        assert np.array_equal(R.np_rgb2hsv(a[lo:lo + 256]), hsv[lo:lo + 256])
        assert np.array_equal(R.np_hsv2rgb(a[lo:lo + 256]), rgb[lo:lo + 256])
    small = a[::64, ::64]
    assert np.array_equal(R.np_hue(small, R.hue_shift(-0.0275)), R.pil_hue(small, -0.0275))
    assert np.array_equal(R.np_hue(small, 0), R.pil_hue(small, 0.0))
    assert R.hue_shift(-0.0275) == 249 and R.hue_shift(0.03) == 7


def test_composed_pipeline_equals_pillow(noise):
    from vfloodnet_amd import train_dataset as D
    img, mask = noise
    params = D.draw_clip_params(random.Random(3), 67, 93, 4, 16)
    f_np, m_np, l_np = R.np_clip(img, mask, params, 16, [2, 1])
    f_pil, m_pil, l_pil = R.pil_clip(img, mask, params, 16, [2, 1])
    assert np.array_equal(f_np, f_pil) and np.array_equal(m_np, m_pil) and np.array_equal(l_np, l_pil)


# ------------------------------------------------------------------------------------------------ the package's host half
def test_inverse_matrix():
    """``inverse_affine_matrix`` against matrices worked out by hand (output pixel -> source pixel about the centre c:
    src = c + A^-1 (dst - c - t) with A = scale * R(angle) * Shear) and against the forward matrix inverted by NumPy."""
    from vfloodnet_amd import train_dataset as D
    m = D.inverse_affine_matrix(10, 10, 90.0, (0, 0), 1.0, 0.0)     # a quarter turn about the centre
    assert np.allclose(m, [0, 1, 0, -1, 0, 10], atol=1e-12)
    m = D.inverse_affine_matrix(8, 6, 0.0, (3, -2), 2.0, 0.0)       # scale 2, shift (3, -2): src = c + (dst - c - t) / 2
    assert np.allclose(m, [0.5, 0, 4 - 0.5 * (4 + 3), 0, 0.5, 3 - 0.5 * (3 - 2)], atol=1e-12)
    m = D.inverse_affine_matrix(8, 6, 0.0, (0, 0), 1.0, 45.0)       # shear only: A = [[1, -tan 45], [0, 1]], A^-1 = [[1, 1], [0, 1]]
    assert np.allclose(m, [1, 1, -3, 0, 1, 0], atol=1e-12)
    prng = random.Random(1)
    for case in [(20.0, (0, 0), 1.0, 10.0)] + [(prng.uniform(-20, 20), (prng.randint(-9, 9), prng.randint(-9, 9)), prng.uniform(0.9, 1.1),
                                               prng.uniform(-10, 10)) for _ in range(20)]:
        angle, (tx, ty), scale, shear = case
        W, H = 67, 93
        r, s = math.radians(angle), math.radians(shear)
        # torchvision's forward map: T(c) T(t) [scale * Rot(r) * [[1, -tan s], [0, 1]]] T(-c)
        A = scale * np.array([[math.cos(r), -math.sin(r)], [math.sin(r), math.cos(r)]]) @ np.array([[1, -math.tan(s)], [0, 1]])
        F = np.eye(3)
        F[:2, :2] = A
        c, t = np.array([W * 0.5, H * 0.5]), np.array([tx, ty])
        F[:2, 2] = c + t - A @ c
        assert np.allclose(np.array(D.inverse_affine_matrix(W, H, *case)).reshape(2, 3), np.linalg.inv(F)[:2], atol=1e-9), case
        assert D.inverse_affine_matrix(W, H, *case) == R.inverse_affine_matrix(W, H, *case)      # the helper's copy, used by np_* / pil_*


def test_draw_clip_params():
    from vfloodnet_amd import train_dataset as D
    W, H = 500, 400
    fallback = (0, (W - int(round(H * 4. / 3.))) // 2, H, int(round(H * 4. / 3.))) if W / H > 4. / 3. else (0, 0, H, W)
    tried = 0
    for seed in range(20):
        ps = D.draw_clip_params(random.Random(seed), W, H, 6, 400)
        assert len(ps) == 6
        assert ps[0]['flip'] is False and ps[0]['jitter'] is None and ps[0]['affine'] is None
        for p in ps:
            i, j, h, w = p['crop']
            assert 0 <= i and 0 <= j and 0 < h and 0 < w and i + h <= H and j + w <= W
            if p['crop'] != fallback:                                    # one of the ten tries: scale (0.8, 1), ratio (3/4, 4/3)
                tried += 1
                assert 0.8 * W * H * 0.98 <= h * w <= W * H and 0.74 <= w / h <= 1.35
        for p in ps[1:]:
            order, (b, c, s, shift) = p['jitter']
            assert sorted(order) == [0, 1, 2, 3] and all(0.9 <= v <= 1.1 for v in (b, c, s))
            d = p['draws']
            assert -0.03 <= d['hue'] <= 0.03 and shift == int(d['hue'] * 255) % 256 and (shift <= 7 or shift >= 249)
            assert -20 <= d['angle'] <= 20 and 0.9 <= d['scale'] <= 1.1 and -10 <= d['shear'] <= 10
            assert abs(d['translate'][0]) <= 0.1 * W and abs(d['translate'][1]) <= 0.1 * H
            assert d['translate'][0] == round(d['translate'][0]) and d['translate'][1] == round(d['translate'][1])
            assert p['affine'] == R.inverse_affine_matrix(W, H, d['angle'], d['translate'], d['scale'], d['shear'])
    assert tried > 60
    # a 16:9 source admits no crop of 80 % of its area inside the ratio range: always the central 4:3 crop
    assert all(p['crop'] == (0, 80, 360, 480) for p in D.draw_clip_params(random.Random(1), 640, 360, 6, 400))
    assert any(p['flip'] for s in range(20) for p in D.draw_clip_params(random.Random(s), W, H, 6, 400))
    a, b = D.draw_clip_params(random.Random(5), W, H, 6, 400), D.draw_clip_params(random.Random(5), W, H, 6, 400)
    assert a == b and a != D.draw_clip_params(random.Random(6), W, H, 6, 400)
    # the hook runs once, after frame 0's crop and before frame 1's draws: randoms it consumes shift what follows
    seen = []
    rng = random.Random(5)
    c = D.draw_clip_params(rng, W, H, 6, 400, after_first=lambda p: (seen.append(dict(p)), [rng.random() for _ in range(3)]))
    assert len(seen) == 1 and seen[0]['crop'] == a[0]['crop'] and c[0] == a[0] and c[1:] != a[1:]
    with pytest.raises(ValueError):
        D.draw_clip_params(random.Random(0), 8193, 100, 3, 400)


def test_crop_falls_back_to_the_centre_for_an_extreme_aspect_ratio():
    from vfloodnet_amd import train_dataset as D
    # 1000 x 10: no crop of >= 80 % of the area has an aspect ratio <= 4/3 that fits -> height 10, width round(10 * 4/3)
    for seed in range(5):
        p = D.draw_clip_params(random.Random(seed), 1000, 10, 2, 400)
        assert [q['crop'] for q in p] == [(0, (1000 - 13) // 2, 10, 13)] * 2
    p = D.draw_clip_params(random.Random(0), 10, 1000, 1, 400)
    assert p[0]['crop'] == ((1000 - 13) // 2, 0, int(round(10 / 0.75)), 10)


def test_dataset_lists_the_reference_layout(tmp_path):
    from vfloodnet_amd import train_dataset as D
    root = str(tmp_path / 'ds')
    make_tree(root)
    ds = D.Water_Image_Train_DS(root, 400, clip_n=6, max_obj_n=3)
    assert len(ds) == 3 and (ds.clip_n, ds.output_size, ds.max_obj_n) == (6, 400, 3)
    assert [os.path.basename(p) for p in ds.img_list] == ['000.jpg', '001.png', '002.jpg']
    assert [os.path.basename(p) for p in ds.mask_list] == ['000.png', '001.png', '002.png']
    assert D.Water_Image_Train_DS(root, 400).clip_n == 3 and D.Water_Image_Train_DS(root, 400).max_obj_n == 11
    os.remove(ds.mask_list[2])
    with pytest.raises(AssertionError):
        D.Water_Image_Train_DS(root, 400)


def test_dataset_items_carry_the_files_content(tmp_path):
    """The host part, without a GPU: JPEG -> coefficients, PNG -> inflated scanlines, a palette mask -> its scanlines."""
    from vfloodnet_amd import train_dataset as D
    root = str(tmp_path / 'ds')
    make_tree(root)
    ds = D.Water_Image_Train_DS(root, 400)
    it = ds[0]
    assert set(it) == {'img', 'mask', 'name'} and it['name'] == ds.img_list[0]
    assert 'jpeg' in it['img'] and 'png' in ds[1]['img']
    filtered, info, _ = it['mask']['png']
    W, H, ctype, bpp = (int(v) for v in info)
    assert (W, H, ctype, bpp) == (40, 30, 3, 1)
    rgb = ds.mask_list[0][:-4] + '_rgb.png'                           # not a palette file: PIL converts, as the reference does
    Image.fromarray(np.zeros((30, 40, 3), np.uint8)).save(rgb)
    u8 = D._host_decode(rgb, 'P')['u8'].numpy()
    assert u8.shape == (30, 40) and np.array_equal(u8, np.array(Image.open(rgb).convert('P')))


def test_cli_defaults_are_the_reference_s():
    from vfloodnet_amd import train_video_seg as TV
    a = TV.get_parser().parse_args(['--dataset', 'x'])
    assert (a.gpu, a.dataset, a.seed, a.log, a.level, a.lr, a.lu, a.resume, a.new) == (0, 'x', -1, False, 0, 1e-5, 0.5, None, False)
    assert (a.scheduler_step, a.total_epochs, a.budget, a.obj_n, a.clip_n, a.size) == (25, 100, 300000, 3, 6, 400)
    with pytest.raises(SystemExit):
        TV.get_parser().parse_args([])
    assert math.isclose(TV.get_parser().parse_args(['--dataset', 'x', '--lr', '2e-5']).lr, 2e-5)
