"""The image model's validation on the device (include/vfn_image_val.h): the sample kernels of ``WaterDataset_RGB`` against
Pillow called the way torchvision's PIL back end calls it (tests/aug_ref.py ``pil_*``), EQUAL IN EVERY BYTE AND BIT; the scoring
kernel against NumPy float64; the argument checks of the raw ABI; then ``ValidEpoch`` over a small dataset and the command line.

Tolerances of the scoring kernel: S3 and S4 are sums of small integers and must be equal.  Every term of S0 .. S2 is exact in
double (an f32 x f32 product has 48 significant bits) and non-negative, and at most 2^22 of them are added, so any order of the
additions stays within n * 2^-53 ~ 5e-10 of the exact sum, relative: 1e-9 for the sums, the loss and the score."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import aug_ref as R

pytestmark = pytest.mark.gpu

f32 = np.float32
MEAN = np.array([0.485, 0.456, 0.406], f32).reshape(3, 1, 1)
STD = np.array([0.229, 0.224, 0.225], f32).reshape(3, 1, 1)
ERR_ARG = 1


def dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@pytest.fixture(scope='module')
def maker(gpu):
    from vfloodnet_amd.image_dataset import ImageSampleMaker
    return ImageSampleMaker(gpu)


@pytest.fixture(scope='module')
def photos():
    """(image uint8 [H, W, 3], label uint8 [H, W]): a 93 x 67 noise photograph with a three-label plane, and an even 64 x 48."""
    rng = np.random.default_rng(20200212)
    out = []
    for W, H in ((93, 67), (64, 48)):
        out.append((rng.integers(0, 256, (H, W, 3), dtype=np.uint8), rng.integers(0, 3, (H, W), dtype=np.uint8)))
    return out


# ================================================================================================ the sample kernels
def pil_normalise(a):
    """``ToTensor`` and ``Normalize``: f32 throughout, a subtraction and a division."""
    t = np.ascontiguousarray(a.transpose(2, 0, 1)).astype(f32) / f32(255)
    return (t - MEAN) / STD


def pil_sample(img, lab, p, S):
    """One ``train_offline`` sample through Pillow: colour in the fixed order, affine, flip, crop + resize, normalisation."""
    a, l = img, lab
    if p.get('brightness') is not None:
        a = R.pil_brightness(a, p['brightness'])
    if p.get('contrast') is not None:
        a = R.pil_contrast(a, p['contrast'])
    if p.get('hue') is not None:
        assert p['hue'] == int(0.1 * 255)
        a = R.pil_hue(a, 0.1)
    if p.get('affine') is not None:
        a, l = R.pil_affine(a, p['affine'], 'bicubic'), R.pil_affine(l, p['affine'], 'nearest')
    if p.get('flip'):
        a, l = R.pil_hflip(a), R.pil_hflip(l)
    i, j, h, w = p['crop']
    a, l = R.pil_crop_resize(a, i, j, h, w, S, 'bicubic'), R.pil_crop_resize(l, i, j, h, w, S, 'nearest')
    return pil_normalise(a), l.astype(f32)[None]


def sample_cases(W, H):
    """(name, parameters, S) for a W x H photograph."""
    whole = (0, 0, H, W)
    aff = R.inverse_affine_matrix(W, H, 13.0, (0.15, -0.07), 1.12, -9.0)
    aff2 = R.inverse_affine_matrix(W, H, -19.0, (3.3, -2.7), 0.74, 17.0)
    scale_only = R.inverse_affine_matrix(W, H, 0.0, (0.2, -0.2), 0.8, 0.0)       # m1 == m3 == 0: the table path
    assert scale_only[1] == 0 and scale_only[3] == 0
    cases = []

    def add(name, S=32, **p):
        p.setdefault('crop', whole)
        cases.append((name, p, S))
    # ---- colour: none, each operation alone, both clamps of brightness and contrast, all three
    add('no colour')
    add('brightness alone', brightness=0.7)
    add('contrast alone', contrast=1.3)
    add('hue alone', hue=25)
    add('brightness 0.1', brightness=0.1)
    add('brightness 1.2', brightness=1.2)
    add('contrast 0.2', contrast=0.2)
    add('contrast 1.8', contrast=1.8)
    add('all colour', brightness=0.93, contrast=1.41, hue=25)
    # ---- geometry
    add('affine', affine=aff)
    add('affine + flip', affine=aff, flip=True)
    add('flip alone', flip=True)
    add('tables + flip', affine=scale_only, flip=True)
    add('tables', affine=scale_only)
    add('everything', brightness=1.1, contrast=0.6, hue=25, affine=aff2, flip=True, crop=(5, 7, 40, 31))
    # ---- windows
    for flip in (False, True):
        add(f'1 x 1 window, flip {flip}', affine=aff, flip=flip, crop=(H // 2, W // 3, 1, 1))
        add(f'right edge, flip {flip}', affine=aff2, flip=flip, crop=(3, W - 20, 30, 20))
        add(f'bottom edge, flip {flip}', affine=aff2, flip=flip, crop=(H - 17, 4, 17, 41))
        add(f'corner, no affine, flip {flip}', flip=flip, crop=(H - 9, W - 11, 9, 11))
    # ---- S = 5 and 32, the window smaller (enlargement) and larger (reduction) than S on each axis independently
    for S, small, large in ((5, 3, 44), (32, 20, 45)):
        add(f'S {S}: rows enlarged, columns reduced', S=S, affine=aff, flip=True, crop=(2, 6, small, large))
        add(f'S {S}: rows reduced, columns enlarged', S=S, affine=aff, crop=(1, 9, large, small))
        add(f'S {S}: both enlarged', S=S, contrast=1.2, crop=(8, 8, small, small))
        add(f'S {S}: both reduced', S=S, flip=True, crop=(0, 0, large, large))
        add(f'S {S}: window of S x S', S=S, affine=aff, crop=(4, 4, S, S))
    return cases


def test_train_offline_sample_equals_pillow(maker, gpu, photos):
    for img, lab in photos:
        H, W = lab.shape
        dimg, dlab = dev(img, gpu), dev(lab, gpu)
        for name, p, S in sample_cases(W, H):
            x = torch.full((3, 3, S, S), -77.0, device=gpu)
            y = torch.full((3, 1, S, S), -77.0, device=gpu)
            maker.train_sample(dimg, dlab, p, x, y, 1)
            rx, ry = pil_sample(img, lab, p, S)
            gx, gy = x.cpu().numpy(), y.cpu().numpy()
            where = f'{W} x {H}: {name}'
            assert np.array_equal(gx[1].view(np.int32), rx.view(np.int32)), where
            assert np.array_equal(gy[1], ry), where
            assert (gx[[0, 2]] == -77.0).all() and (gy[[0, 2]] == -77.0).all(), where          # the other slots are not touched


def test_jitter_larger_than_one_pass_of_the_grid(maker, gpu):
    """1024 blocks of 256 threads cover 262144 pixels: 600 x 500 makes the grid-stride loops take a second turn."""
    img = np.random.default_rng(3).integers(0, 256, (500, 600, 3), dtype=np.uint8)
    p = {'brightness': 1.07, 'contrast': 0.93, 'hue': 25}
    want = R.pil_hue(R.pil_contrast(R.pil_brightness(img, 1.07), 0.93), 0.1)
    assert np.array_equal(maker.jitter(dev(img, gpu), p).cpu().numpy(), want)


def test_val_offline_sample_equals_pillow(maker, gpu, photos):
    """The label against ``Image.resize((S, S))`` of the mode-P plane, enlarged, reduced and mixed; the image against
    ``resize((S, S), BILINEAR)`` + normalisation."""
    for img, lab in photos:
        H, W = lab.shape
        for S in (5, 32, 80, 128, H):
            x = torch.full((2, 3, S, S), -77.0, device=gpu)
            y = torch.full((2, 1, S, S), -77.0, device=gpu)
            maker.val_sample(dev(img, gpu), dev(lab, gpu), x, y, 1)
            ry = np.array(Image.fromarray(lab, 'P').resize((S, S))).astype(f32)
            rx = pil_normalise(np.array(Image.fromarray(img, 'RGB').resize((S, S), Image.BILINEAR)))
            assert np.array_equal(y.cpu().numpy()[1, 0], ry), (W, H, S)
            assert np.array_equal(x.cpu().numpy()[1].view(np.int32), rx.view(np.int32)), (W, H, S)
            assert (y[0] == -77.0).all() and (x[0] == -77.0).all()


# ================================================================================================ the scoring kernel
def np_scores(pr, gt, threshold=0.5):
    """The definitions of include/vfn_image_val.h in float64 on the same f32 inputs -> (S0 .. S4, [dice_loss, iou_score])."""
    p, g = pr.astype(np.float64).ravel(), gt.astype(np.float64).ravel()
    b = (pr.ravel() > f32(threshold)).astype(np.float64)
    S = np.array([(g * p).sum(), p.sum(), g.sum(), (g * b).sum(), b.sum()])
    return S, np.array([1.0 - (2.0 * S[0] + 1.0) / (S[1] + S[2] + 1.0), (S[3] + 1e-7) / (S[2] + S[4] - S[3] + 1e-7)])


def close(a, b, rel=1e-9):
    return abs(a - b) <= rel * max(abs(a), abs(b))


SCORE_SIZES = [1, 63, 64, 65, 255, 256, 257, 2049, 3 * 2048 + 1, 4 * 32 * 32, 2 * 1024 * 1024 + 3]


@pytest.fixture(scope='module')
def score_inputs():
    """One set of inputs per size, computed once with its float64 reference: probabilities in [0, 1] that hold exact 0.5 (not
    counted) and nextafter(0.5, 1) (counted), labels 0, 1 and 2."""
    rng = np.random.default_rng(7)
    out = {}
    for n in SCORE_SIZES:
        pr = rng.random(n, dtype=f32)
        gt = rng.integers(0, 3, n).astype(f32)
        pr[::5] = f32(0.5)
        pr[1::7] = np.nextafter(f32(0.5), f32(1))
        out[n] = (pr, gt) + np_scores(pr, gt)
    return out


@pytest.mark.parametrize('n', SCORE_SIZES)
def test_seg_scores_against_float64(gpu, score_inputs, n):
    from vfloodnet_amd.val_image_seg import seg_scores
    pr, gt, S_ref, row_ref = score_inputs[n]
    log = torch.full((3, 2), -5.0, dtype=torch.float64, device=gpu)
    sums, row = seg_scores(dev(pr, gpu), dev(gt, gpu), log=log, t=1)
    S, got = sums.cpu().numpy(), log.cpu().numpy()
    print(f'n {n}: S {S.tolist()} ref {S_ref.tolist()} row {got[1].tolist()} ref {row_ref.tolist()}')
    assert S[3] == S_ref[3] and S[4] == S_ref[4]
    assert all(close(S[k], S_ref[k]) for k in range(3))
    assert close(got[1, 0], row_ref[0]) and close(got[1, 1], row_ref[1])
    assert (got[[0, 2]] == -5.0).all() and torch.equal(row, log[1])
    sums2, row2 = seg_scores(dev(pr, gpu), dev(gt, gpu))                        # a second run: the same bits
    assert np.array_equal(sums2.cpu().numpy().view(np.int64), S.view(np.int64))
    assert np.array_equal(row2.cpu().numpy().view(np.int64), got[1].view(np.int64))


def test_seg_scores_threshold_is_strict_and_zero_inputs(gpu):
    from vfloodnet_amd.val_image_seg import dice_loss, iou_score, seg_scores
    above = np.nextafter(f32(0.5), f32(1))
    pr = np.array([0.5, above, 0.5, above, 0.25], f32)
    gt = np.array([1, 1, 0, 2, 1], f32)
    S = seg_scores(dev(pr, gpu), dev(gt, gpu))[0].cpu().numpy()
    assert S[4] == 2.0 and S[3] == 3.0 and S[2] == 5.0                          # 0.5 is not counted, the next float is
    assert np.array_equal(S, np_scores(pr, gt)[0])
    # all-zero inputs: loss = 1 - (0 + 1) / (0 + 0 + 1) = 0, score = 1e-7 / 1e-7 = 1
    z = torch.zeros(2, 1, 32, 32, device=gpu)
    sums, row = seg_scores(z, z)
    assert (sums == 0).all() and row.cpu().tolist() == [0.0, 1.0]
    assert dice_loss(z, z) == 0.0 and iou_score(z, z) == 1.0
    # another threshold
    assert seg_scores(dev(pr, gpu), dev(gt, gpu), threshold=0.2)[0].cpu().numpy()[4] == 5.0


# ================================================================================================ argument checks of the raw ABI
def test_raw_abi_argument_checks(gpu):
    """Null pointers, a window outside the image, sizes out of range: VFN_ERR_ARG, and nothing written."""
    from vfloodnet_amd import _lib
    L, p, st = _lib.lib(), _lib.ptr, _lib.stream
    H, W, S, B = 20, 24, 8, 2
    big = _lib.TRAIN_AUG_MAX_SIDE + 1
    img = torch.zeros(H, W, 3, dtype=torch.uint8, device=gpu)
    lab = torch.zeros(H, W, dtype=torch.uint8, device=gpu)
    out8 = torch.full((H, W, 3), 200, dtype=torch.uint8, device=gpu)
    out8b = torch.full((H, W), 200, dtype=torch.uint8, device=gpu)
    lsum = torch.zeros(1, dtype=torch.int64, device=gpu)
    x = torch.full((B, 3, S, S), -77.0, device=gpu)
    y = torch.full((B, 1, S, S), -77.0, device=gpu)
    tab = torch.zeros(4096, dtype=torch.int32, device=gpu)
    f3 = (C.c_float * 3)(0.5, 0.5, 0.5)
    m = (C.c_double * 6)(1.0, 0.1, 0.0, 0.1, 1.0, 0.0)
    far = (C.c_double * 6)(1.0, 0.1, 40000.0, 0.1, 1.0, 0.0)                    # a corner at 40000: past 16.16 fixed point
    nan = (C.c_double * 6)(1.0, float('nan'), 0.0, 0.1, 1.0, 0.0)

    def jitter(src=img, h=H, w=W, bri=1, fb=0.9, con=1, fc=1.1, hue=1, shift=25, jit=out8, ls=lsum):
        return L.vfn_imgval_jitter(p(src), h, w, bri, fb, con, fc, hue, shift, p(jit), p(ls), st())
    assert jitter(src=None) == ERR_ARG and jitter(jit=None) == ERR_ARG and jitter(ls=None) == ERR_ARG
    assert jitter(h=0) == ERR_ARG and jitter(w=big) == ERR_ARG and jitter(shift=256) == ERR_ARG and jitter(shift=-1) == ERR_ARG
    assert jitter(fb=float('inf')) == ERR_ARG and jitter(fc=float('nan')) == ERR_ARG
    assert jitter(bri=0, con=0, hue=0) == 0                                     # nothing to do: nothing launched

    def window(a=img, l=lab, h=H, w=W, on=1, mm=m, tabs=0, xt=tab, yt=tab, win=(2, 3, 5, 6), oi=out8, ol=out8b):
        return L.vfn_imgval_affine_window(p(a), p(l), h, w, on, mm, tabs, p(xt), p(yt), 1, *win, p(oi), p(ol), st())
    assert window(a=None) == ERR_ARG and window(l=None) == ERR_ARG and window(oi=None) == ERR_ARG and window(ol=None) == ERR_ARG
    assert window(mm=None) == ERR_ARG and window(mm=nan) == ERR_ARG and window(mm=far) == ERR_ARG
    assert window(tabs=1, mm=(C.c_double * 6)(1.0, 0.0, 0.0, 0.0, 1.0, 0.0), xt=None) == ERR_ARG
    assert window(h=0) == ERR_ARG and window(w=big) == ERR_ARG
    for win in ((-1, 3, 5, 6), (2, -1, 5, 6), (2, 3, 0, 6), (2, 3, 5, 0), (H - 4, 3, 5, 6), (2, W - 5, 5, 6), (0, 0, H + 1, W)):
        assert window(win=win) == ERR_ARG, win

    def resize(a=out8, h=H, w=W, hp=out8, bx=tab, kx=tab, ksx=5, by=tab, ky=tab, ksy=5, xx=x, nb=B, b=0, s=S, mean=f3, std=f3):
        return L.vfn_imgval_resize_norm(p(a), h, w, p(hp), p(bx), p(kx), ksx, p(by), p(ky), ksy, p(xx), nb, b, s, mean, std, st())
    for k in ('a', 'hp', 'bx', 'kx', 'by', 'ky', 'xx', 'mean', 'std'):
        assert resize(**{k: None}) == ERR_ARG, k
    assert resize(h=0) == ERR_ARG and resize(w=big) == ERR_ARG and resize(s=0) == ERR_ARG
    assert resize(s=_lib.TRAIN_AUG_MAX_OUT + 1) == ERR_ARG and resize(b=B) == ERR_ARG and resize(b=-1) == ERR_ARG and resize(nb=0) == ERR_ARG
    assert resize(ksx=0) == ERR_ARG and resize(ksy=0) == ERR_ARG
    assert resize(std=(C.c_float * 3)(0.5, 0.0, 0.5)) == ERR_ARG

    def gather(a=lab, h=H, w=W, nx=tab, ny=tab, yy=y, nb=B, b=0, s=S):
        return L.vfn_imgval_label_gather(p(a), h, w, p(nx), p(ny), p(yy), nb, b, s, st())
    for k in ('a', 'nx', 'ny', 'yy'):
        assert gather(**{k: None}) == ERR_ARG, k
    assert gather(h=big) == ERR_ARG and gather(w=0) == ERR_ARG and gather(s=0) == ERR_ARG and gather(b=B) == ERR_ARG

    pr = torch.rand(100, device=gpu)
    part = torch.full((_lib.SEG_SCORES_MAX_BLOCKS * 5,), -5.0, dtype=torch.float64, device=gpu)
    sums = torch.full((5,), -5.0, dtype=torch.float64, device=gpu)
    log = torch.full((2, 2), -5.0, dtype=torch.float64, device=gpu)

    def scores(a=pr, g=pr, n=100, thr=0.5, pt=part, sm=sums, lg=log, rows=2, t=0):
        return L.vfn_seg_scores_f64(p(a), p(g), n, thr, p(pt), p(sm), p(lg), rows, t, st())
    assert scores(a=None) == ERR_ARG and scores(g=None) == ERR_ARG and scores(pt=None) == ERR_ARG and scores(lg=None) == ERR_ARG
    assert scores(n=0) == ERR_ARG and scores(n=-3) == ERR_ARG and scores(thr=float('nan')) == ERR_ARG
    assert scores(t=2) == ERR_ARG and scores(t=-1) == ERR_ARG and scores(rows=0) == ERR_ARG

    torch.cuda.synchronize()
    assert (out8 == 200).all() and (out8b == 200).all() and (x == -77.0).all() and (y == -77.0).all()
    assert (part == -5.0).all() and (sums == -5.0).all() and (log == -5.0).all() and int(lsum) == 0
    assert scores(sm=None) == 0                                                  # the sums are optional
    torch.cuda.synchronize()
    assert (log[0] != -5.0).all() and (log[1] == -5.0).all()


# ================================================================================================ end to end
@pytest.fixture(scope='module')
def dataset_dir(tmp_path_factory):
    """Five JPEG / PNG pairs of two sizes under one sub-folder."""
    root = str(tmp_path_factory.mktemp('water'))
    os.makedirs(os.path.join(root, 'JPEGImages', 'a'))
    os.makedirs(os.path.join(root, 'Annotations', 'a'))
    with open(os.path.join(root, 'train_imgs.txt'), 'w') as f:
        f.write('a\n')
    rng = np.random.default_rng(11)
    for k in range(5):
        W, H = ((80, 60), (72, 96))[k % 2]
        yy, xx = np.mgrid[0:H, 0:W]
        img = np.stack([(xx * 3 + k * 40) % 256, (yy * 4) % 256, (xx + yy) * 2 % 256], -1)
        img = np.clip(img + rng.integers(-25, 25, img.shape), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, 'JPEGImages', 'a', f'{k}.jpg'), quality=92)
        lab = np.zeros((H, W), np.uint8)
        lab[H // 3 + k:, :] = 1
        if k == 3:
            lab[:6, :9] = 2
        pm = Image.fromarray(lab, 'P')
        pm.putpalette([0, 0, 0, 0, 0, 128, 0, 128, 0] + [100] * (253 * 3))
        pm.save(os.path.join(root, 'Annotations', 'a', f'{k}.png'))
    return root


@pytest.fixture(scope='module')
def linknet(gpu):
    from tools import synth_linknet
    from vfloodnet_amd.linknet import LinknetB4
    sd = synth_linknet.make_state_dict()
    return sd, LinknetB4.from_checkpoint(sd, gpu)


class Recorder:
    """The model behind ``ValidEpoch`` with every (input, output) kept."""

    def __init__(self, model):
        self.model, self.seen = model, []

    def predict(self, x):
        out = self.model.predict(x)
        self.seen.append((x.clone(), out.clone()))
        return out

    def predict_batch(self, x):
        out = self.model.predict_batch(x)
        self.seen.append((x.clone(), out.clone()))
        return out


def recorded(loader, kept):
    for x, y in loader:
        kept.append((x.clone(), y.clone()))
        yield x, y


def run_epoch(dataset_dir, gpu, model, mode, batch_size, seed):
    """-> (ValidEpoch's result, its log, the float64 evaluation of the definitions over what the loader and the model produced)."""
    from vfloodnet_amd.image_dataset import ImageSampleLoader, WaterDataset_RGB
    from vfloodnet_amd.val_image_seg import ValidEpoch
    ds = WaterDataset_RGB(mode, dataset_dir, (64, 64))
    assert len(ds) == 5
    loader = ImageSampleLoader(ds, gpu, batch_size=batch_size, shuffle=False, num_workers=0, seed=seed)
    rec, batches = Recorder(model), []
    epoch = ValidEpoch(rec, gpu)
    got = epoch.run(recorded(loader, batches))
    assert len(batches) == len(rec.seen) == len(loader) == -(-5 // batch_size)
    assert [int(x.shape[0]) for x, _ in batches] == [batch_size] * (5 // batch_size) + ([5 % batch_size] if 5 % batch_size else [])
    rows = []
    for (x, y), (xs, prob) in zip(batches, rec.seen):
        assert torch.equal(x, xs) and prob.shape == y.shape == (x.shape[0], 1, 64, 64)
        rows.append(np_scores(prob.cpu().numpy(), y.cpu().numpy())[1])
    rows = np.array(rows)
    return got, epoch.log, {'dice_loss': float(rows[:, 0].sum() / len(rows)), 'iou_score': float(rows[:, 1].sum() / len(rows))}


@pytest.mark.parametrize('batch_size', [1, 2])
@pytest.mark.parametrize('mode', ['train_offline', 'val_offline'])
def test_valid_epoch_equals_float64_definitions(gpu, dataset_dir, linknet, mode, batch_size):
    model = linknet[1]
    got, log, want = run_epoch(dataset_dir, gpu, model, mode, batch_size, seed=0)
    print(f'{mode} batch {batch_size}: got {got} want {want}')
    for k in ('dice_loss', 'iou_score'):
        assert abs(got[k] - want[k]) <= 1e-9, k
    assert 0.0 < got['dice_loss'] < 1.0 and 0.0 <= got['iou_score'] <= 1.0
    again = run_epoch(dataset_dir, gpu, model, mode, batch_size, seed=0)
    assert np.array_equal(again[1].view(np.int64), log.view(np.int64)) and again[0] == got     # the same seed: the same bits
    other = run_epoch(dataset_dir, gpu, model, mode, batch_size, seed=1)
    if mode == 'train_offline':
        assert not np.array_equal(other[1], log)                                 # other draws, other samples
    else:
        assert np.array_equal(other[1].view(np.int64), log.view(np.int64))       # val_offline draws nothing


def test_command_line_names_the_better_checkpoint(gpu, dataset_dir, linknet, tmp_path, capsys):
    from vfloodnet_amd import val_image_seg
    from vfloodnet_amd.image_dataset import ImageSampleLoader, WaterDataset_RGB
    from vfloodnet_amd.linknet import LinknetB4
    sd = linknet[0]
    flat = {k: v.clone() for k, v in sd.items()}
    flat['segmentation_head.0.weight'] = torch.zeros_like(flat['segmentation_head.0.weight'])   # a constant output: cannot tie
    paths = [str(tmp_path / 'flat.pth'), str(tmp_path / 'full.pth')]
    torch.save(flat, paths[0])
    torch.save({'epoch': 3, 'weights': sd}, paths[1])                            # the reference's resume checkpoint layout
    want = []
    for state in (flat, sd):
        model = LinknetB4.from_checkpoint(state, gpu)
        loader = ImageSampleLoader(WaterDataset_RGB('train_offline', dataset_dir, (64, 64)), gpu, num_workers=0, seed=5)
        rows = np.array([np_scores(model.predict(x).cpu().numpy(), y.cpu().numpy())[1] for x, y in loader])
        assert len(rows) == 5
        want.append((float(rows[:, 0].sum() / 5), float(rows[:, 1].sum() / 5)))
    assert want[0][1] != want[1][1]
    better = paths[0] if want[0][1] > want[1][1] else paths[1]
    out_json = str(tmp_path / 'scores.json')
    val_image_seg.main(['--dataset-path', dataset_dir, '--model-path', paths[0], paths[1], '--input-shape', '64', '--seed', '5',
                        '--num-workers', '0', '--json', out_json])
    printed = capsys.readouterr().out
    with open(out_json) as f:
        report = json.load(f)
    assert [r['model_path'] for r in report['results']] == paths
    for r, (loss, iou) in zip(report['results'], want):
        assert abs(r['dice_loss'] - loss) <= 1e-9 and abs(r['iou_score'] - iou) <= 1e-9
        assert 'dice_loss - {:.4}, iou_score - {:.4}'.format(r['dice_loss'], r['iou_score']) in printed
    assert report['best'] == better and report['mode'] == 'train_offline' and report['batch_size'] == 1 and report['samples'] == 5
    assert 'Best by iou_score: ' + better in printed
