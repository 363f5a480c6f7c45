"""The water-level kernels (``csrc/waterlevel.hip``) against a restatement in numpy (integers and float64), the meter end to
end against the reference's loop restated with scipy's filter, and ``video_seg.main --waterlevel`` against ``est_waterlevel``
run over the mask PNGs it wrote."""
import argparse
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------ the restatement
def warp_coords(minv, H, W):
    """Scaled source coordinates (float64, before rounding) of every destination pixel: include/vfn_hip.h."""
    m = np.asarray(minv, np.float64).reshape(9)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    X0 = m[0] * x + m[1] * y + m[2]
    Y0 = m[3] * x + m[4] * y + m[5]
    Wd = m[6] * x + m[7] * y + m[8]
    with np.errstate(divide='ignore'):
        s = np.where(Wd != 0, 32.0 / Wd, 0.0)
    return np.clip(X0 * s, INT_MIN, INT_MAX), np.clip(Y0 * s, INT_MIN, INT_MAX)


def near_ties(minv, H, W, eps=1e-6):
    """Destination pixels whose scaled coordinate lies within ``eps`` of a rounding tie (n + 1/2)."""
    fx, fy = warp_coords(minv, H, W)
    return (np.abs(fx - np.floor(fx) - 0.5) < eps) | (np.abs(fy - np.floor(fy) - 0.5) < eps)


def warp_ref(img, homo):
    """uint8 [H,W] or [H,W,C] -> the same shape: OpenCV's fixed-point bilinear remap stated in integers."""
    a = img[:, :, None] if img.ndim == 2 else img
    H, W, _ = a.shape
    fx, fy = warp_coords(np.linalg.inv(np.asarray(homo, np.float64)), H, W)
    X, Y = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)          # rint: half to even
    sx, ax, sy, ay = X >> 5, (X & 31)[..., None], Y >> 5, (Y & 31)[..., None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok[..., None], a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), 0)
    acc = ((32 - ay) * ((32 - ax) * tap(sy, sx) + ax * tap(sy, sx + 1)) + ay * ((32 - ax) * tap(sy + 1, sx) + ax * tap(sy + 1, sx + 1)) + 512) >> 10
    return acc.astype(np.uint8).reshape(img.shape)


def warp_frame_ref(frame, homo):
    """float32 [3,H,W] -> float32 [3,H,W]: bytes by truncation of x * 255 (f32 product), warped, / 255 in f32."""
    u8 = (frame * np.float32(255)).astype(np.uint8).transpose(1, 2, 0)
    return np.ascontiguousarray(warp_ref(u8, homo).transpose(2, 0, 1)).astype(np.float32) / np.float32(255)


def scan_ref(label, kps, water=1):
    out = []
    for kx, ky in kps:
        d = -1
        for row in range(ky + 1, label.shape[0]):
            if label[row, kx] == water:
                d = row - ky
                break
        out.append(d)
    return out


def draw_ref(ov, boxes, offsets):
    """The project's drawing rule (include/vfn_hip.h) on a copy of the RGB overlay."""
    out = ov.copy()
    H, W, _ = out.shape
    for x, y, w, h in boxes:
        for py in range(max(y, 0), min(y + h, H - 1) + 1):
            for px in range(max(x, 0), min(x + w, W - 1) + 1):
                if min(px - x, x + w - px, py - y, y + h - py) < 2:
                    out[py, px] = (0, 200, 0)
    for (x, y, w, h), d in zip(boxes, offsets):
        if d > 1:
            kx, ky = int(x + w / 2), int(y + h)
            for py in range(max(ky, 0), min(ky + d, H - 1) + 1):
                for px in (kx, kx + 1):
                    if 0 <= px < W:
                        out[py, px] = (200, 0, 0)
    return out


def rotation(deg, cx, cy, p0, p1):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    return np.array([[c, -s, cx - c * cx + s * cy], [s, c, cy - s * cx - c * cy], [p0, p1, 1.0]], np.float64)


KEYSTONE = np.array([[1.02, 0.05, -3.0], [0.01, 0.98, 2.0], [1e-4, 2e-4, 1.0]], np.float64)
MATRICES = {
    'identity': np.eye(3),
    'shift': np.array([[1, 0, 5], [0, 1, -3], [0, 0, 1]], np.float64),
    'half': np.array([[1, 0, 0.5], [0, 1, 0], [0, 0, 1]], np.float64),
    'keystone': KEYSTONE,
    'rotation': rotation(7.0, 20.0, 15.0, 1.1e-4, -0.9e-4),
}
SIZES = [(37, 53), (64, 96)]


def image(H, W, C, seed):
    rng = np.random.RandomState(seed)
    if C == 3:
        return rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    coarse = rng.randint(0, 2, ((H + 7) // 8, (W + 7) // 8)).astype(np.uint8)      # random 0/1 blobs
    return np.ascontiguousarray(np.kron(coarse, np.ones((8, 8), np.uint8))[:H, :W])


# ------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize('name', sorted(MATRICES))
@pytest.mark.parametrize('C', [1, 3])
@pytest.mark.parametrize('H,W', SIZES)
def test_warp_equals_the_integer_restatement(gpu, H, W, C, name):
    from vfloodnet_amd import ops
    homo = MATRICES[name]
    img = image(H, W, C, 100 * H + C)
    ties = near_ties(np.linalg.inv(homo), H, W)
    assert ties.sum() == 0, 'the test matrices are chosen to have no coordinate near a rounding tie'
    got = ops.warp_perspective_u8(torch.from_numpy(img).to(gpu), homo).cpu().numpy()
    want = warp_ref(img, homo)
    keep = ~ties
    assert ties.mean() <= 1e-3 and np.array_equal(got[keep], want[keep])
    if name == 'identity':
        assert np.array_equal(got, img)
    elif name == 'shift':                         # destination (x, y) = source (x - 5, y + 3), 0 outside
        exp = np.zeros_like(img)
        exp[:H - 3, 5:] = img[3:, :W - 5]
        assert np.array_equal(got, exp)
    elif name == 'half':                          # the rounded mean of source columns x - 1 and x
        a = img.astype(np.int64)
        left = np.zeros_like(a)
        left[:, 1:] = a[:, :-1]
        assert np.array_equal(got, ((left + a + 1) >> 1).astype(np.uint8))
    else:                                         # part of the output lies outside the source
        fx, fy = warp_coords(np.linalg.inv(homo), H, W)
        outside = (fx < -32) | (fy < -32) | (fx > 32 * W) | (fy > 32 * H)
        assert 0 < outside.sum() < H * W and not got[outside].any()


def test_warp_of_the_float_frame(gpu):
    from vfloodnet_amd import ops
    H, W = 37, 53
    frame = torch.from_numpy(image(H, W, 3, 5)).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    for name in ('shift', 'keystone'):
        got = ops.warp_perspective_u8(frame.to(gpu), MATRICES[name]).cpu().numpy()
        want = warp_frame_ref(frame.numpy(), MATRICES[name])
        assert got.dtype == np.float32 and np.array_equal(got, want)
    with pytest.raises(ValueError):
        ops.warp_perspective_u8(frame.to(gpu), np.zeros((3, 3)))
    with pytest.raises(ValueError):
        ops.warp_perspective_u8(torch.zeros(4, 4, 2, dtype=torch.uint8, device=gpu), np.eye(3))


# ------------------------------------------------------------------------------------------------ scan
def test_scan_five_references_in_one_launch(gpu):
    from vfloodnet_amd import ops
    H, W = 40, 64
    lab = np.zeros((H, W), np.uint8)
    kps = [(3, 10), (9, 10), (20, 5), (30, H - 1), (40, 7)]
    lab[12:, 3] = 1                               # water two rows below the key point
    lab[11:, 9] = 1                               # directly below: offset 1
    lab[0:6, 20] = 1                              # water only above / at the key point: nothing below
    lab[:, 30] = 1                                # key point on the last row
    lab[10:20, 40] = 2                            # label 2 above label 1: only 1 counts
    lab[20:, 40] = 1
    log = torch.full((3, 5), -7, dtype=torch.int32, device=gpu)
    ops.waterline_scan(torch.from_numpy(lab).to(gpu), np.array(kps, np.int32), log, 1)
    got = log.cpu().numpy()
    assert got[1].tolist() == scan_ref(lab, kps) == [2, 1, -1, -1, 13]
    assert (got[[0, 2]] == -7).all()              # only row t is written
    log2 = torch.zeros((1, 5), dtype=torch.int32, device=gpu)
    ops.waterline_scan(torch.from_numpy(lab).to(gpu), kps, log2, 0, water_label=2)
    assert log2.cpu().numpy()[0].tolist() == scan_ref(lab, kps, 2) == [-1, -1, -1, -1, 3]


def test_scan_beyond_one_stride_of_the_wave(gpu):
    from vfloodnet_amd import ops
    H, W = 300, 17
    lab = np.zeros((H, W), np.uint8)
    lab[257:, 5] = 1
    lab[299, 6] = 1
    kps = [(5, 2), (6, 0), (7, 0), (5, 256), (5, 192)]
    log = torch.zeros((1, 5), dtype=torch.int32, device=gpu)
    ops.waterline_scan(torch.from_numpy(lab).to(gpu), kps, log, 0)
    assert log.cpu().numpy()[0].tolist() == scan_ref(lab, kps) == [255, 299, -1, 1, 65]


@pytest.mark.parametrize('kp', [(64, 3), (-1, 3), (3, 40), (3, -1)])
def test_scan_rejects_a_key_point_outside_the_image(gpu, kp):
    from vfloodnet_amd import ops, _lib
    import ctypes as C
    lab = torch.zeros(40, 64, dtype=torch.uint8, device=gpu)
    log = torch.zeros((1, 2), dtype=torch.int32, device=gpu)
    with pytest.raises(ValueError):
        ops.waterline_scan(lab, [(1, 1), kp], log, 0)
    raw = (C.c_int * 4)(1, 1, kp[0], kp[1])       # the C entry point refuses too (VFN_ERR_ARG = 1), and launches nothing
    assert _lib.lib().vfn_waterline_scan(_lib.ptr(lab), 40, 64, raw, 2, 1, _lib.ptr(log), 1, 0, _lib.stream()) == 1
    with pytest.raises(ValueError):
        ops.waterline_scan(lab, [(1, 1), (2, 2)], log, 1)          # row outside the log


# ------------------------------------------------------------------------------------------------ draw
def test_draw_equals_the_rule(gpu):
    from vfloodnet_amd import ops
    H, W = 48, 64
    ov = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = [(10, 5, 8, 10), (50, 30, 13, 17), (30, 4, 7, 9), (20, 20, 6, 5), (40, 2, 3, 1)]    # the second touches two image edges
    offsets = [20, 9, -1, 1, 60]                   # no line for -1 and 1; the last line runs off the image
    log = torch.tensor([[0] * 5, offsets], dtype=torch.int32, device=gpu)
    dev = torch.from_numpy(ov).to(gpu)
    out = ops.waterlevel_draw(dev, np.array(boxes, np.int32), log, 1)
    assert out.data_ptr() == dev.data_ptr()
    want = draw_ref(ov, boxes, offsets)
    assert np.array_equal(dev.cpu().numpy(), want)
    assert (want[47, 63] == (0, 200, 0)).all() and (want[15:36, 14] == (200, 0, 0)).all() and (want[16:40, 33] == ov[16:40, 33]).all()


# ------------------------------------------------------------------------------------------------ meter end to end
T_CLIP, H_CLIP, W_CLIP = 12, 48, 64
BOXES = [(10, 5, 8, 10), (40, 8, 7, 9)]
NAMES = [f'2021-09-01-12-00-{2 * t:02d}' for t in range(T_CLIP)]


def synthetic_clip():
    rng = np.random.RandomState(11)
    frames = (rng.randint(0, 256, (T_CLIP, 3, H_CLIP, W_CLIP)).astype(np.float32) / np.float32(255))
    labels = np.zeros((T_CLIP, H_CLIP, W_CLIP), np.uint8)
    for t in range(T_CLIP):
        if t not in (0, 6):                        # frames without any water: the previous estimate is kept
            labels[t, 40 - 2 * t:, :] = 1          # the water line rises by two rows a frame
    return frames, labels


def reference_loop(labels, boxes, homo):
    """reference_tracking.py:157-217 on label maps (warped by the restatement), scipy's filter, nanmean."""
    import copy
    from scipy.ndimage import gaussian_filter1d
    levels = [[0 for _ in boxes]]
    offsets = []
    for lab in labels:
        if homo is not None:
            lab = warp_ref(lab, homo)
        est = copy.deepcopy(levels[-1])
        offsets.append(scan_ref(lab, [(int(x + w / 2), int(y + h)) for x, y, w, h in boxes]))
        for r, d in enumerate(offsets[-1]):
            if d > 0:
                est[r] = np.nan if d == 1 else d
        levels.append(est)
    px = np.array(levels[1:], np.float64)
    for r in range(len(boxes)):
        px[:, r] = gaussian_filter1d(px[:, r], sigma=2, mode='nearest')
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        return offsets, px, np.nanmean(px, axis=1)


@pytest.fixture(scope='module', params=['plain', 'calibrated'])
def metered(request, gpu, tmp_path_factory):
    from vfloodnet_amd import waterlevel
    homo = KEYSTONE if request.param == 'calibrated' else None
    if homo is not None:
        assert near_ties(np.linalg.inv(homo), H_CLIP, W_CLIP).sum() == 0
    frames, labels = synthetic_clip()
    meter = waterlevel.WaterLevelMeter(BOXES, homo, frames_hint=4, device=gpu)
    overlays = []
    for t in range(T_CLIP):
        ov = meter.measure(torch.from_numpy(labels[t]).to(gpu), torch.from_numpy(frames[t]).to(gpu), NAMES[t])
        overlays.append(ov)
    assert meter.measure(torch.from_numpy(labels[0]).to(gpu), None, 'no-frame') is None and meter.t == T_CLIP + 1
    meter.t -= 1                                    # (that probe is not part of the clip)
    meter.names.pop()
    path = str(tmp_path_factory.mktemp('wl') / 'waterlevel.csv')
    meter.write_csv(path)
    return dict(homo=homo, frames=frames, labels=labels, meter=meter, overlays=[o.cpu().numpy() for o in overlays], csv=path,
                ref=reference_loop(labels, BOXES, homo))


def test_meter_levels_equal_the_reference_loop(metered):
    names, levels, avg = metered['meter'].result
    offsets, want, want_avg = metered['ref']
    assert metered['meter'].log.shape[0] == 16                      # grew 4 -> 8 -> 16 and every row landed where it belongs
    assert metered['meter'].offsets().tolist() == offsets
    assert names == NAMES and levels.shape == (T_CLIP, 2) and levels.dtype == np.float64
    assert np.array_equal(np.isnan(levels), np.isnan(want)) and np.array_equal(np.isnan(avg), np.isnan(want_avg))
    assert np.nanmax(np.abs(levels - want)) <= 1e-12 and np.nanmax(np.abs(avg - want_avg)) <= 1e-12
    if metered['homo'] is None:                                     # the clip exercises every branch of the rule
        col = [o[1] for o in offsets]
        assert -1 in col and 1 in col and max(col) > 1


def test_meter_csv_equals_pandas(metered):
    pd = pytest.importorskip('pandas')
    from datetime import datetime
    _, want, want_avg = metered['ref']
    df = pd.DataFrame(want, index=[datetime.strptime(n, '%Y-%m-%d-%H-%M-%S') for n in NAMES], columns=['est_ref0_px', 'est_ref1_px'])
    df['est_avg_px'] = want_avg
    assert open(metered['csv'], 'rb').read() == df.to_csv().encode('utf-8')


def test_meter_overlays_equal_overlay_plus_drawing(metered, gpu):
    from vfloodnet_amd import ops
    from vfloodnet_amd.data import color_palette
    offsets = metered['ref'][0]
    for t in range(T_CLIP):
        lab, frame = metered['labels'][t], metered['frames'][t]
        if metered['homo'] is not None:
            lab, frame = warp_ref(lab, metered['homo']), warp_frame_ref(frame, metered['homo'])
        base = ops.overlay_device(torch.from_numpy(frame).to(gpu), torch.from_numpy(lab).to(gpu), color_palette).cpu().numpy()
        assert np.array_equal(metered['overlays'][t], draw_ref(base, BOXES, offsets[t])), t


def test_meter_refuses_a_key_point_outside_the_image(gpu):
    from vfloodnet_amd import waterlevel
    meter = waterlevel.WaterLevelMeter([(10, 5, 8, 10)], device=gpu)
    lab = torch.zeros(48, 64, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        meter.measure(lab, bbox=[(60, 5, 8, 10)])
    with pytest.raises(ValueError):
        meter.measure(lab, bbox=[(10, 5, 8, 10), (1, 1, 1, 1)])
    assert meter.t == 0 and meter.names == []
    meter.measure(lab, bbox=[(20, 5, 8, 10)], stream=torch.cuda.Stream(gpu))
    assert meter.finish()[1].tolist() == [[0.0]]


# ------------------------------------------------------------------------------------------------ inline = offline
@pytest.mark.parametrize('mem_every', [1, 3])
def test_main_with_waterlevel_equals_est_waterlevel_over_its_masks(gpu, tmp_path, monkeypatch, mem_every):
    """``video_seg.main --waterlevel`` (static box, homography; frame by frame and in groups of three) writes the
    ``waterlevel.csv`` that ``est_waterlevel`` computes from the mask PNGs of that run, and the same mask files as a run
    without ``--waterlevel``."""
    from PIL import Image
    from tools import synth
    from vfloodnet_amd import video_seg, est_waterlevel
    from vfloodnet_amd.data import save_seg_mask, color_palette
    monkeypatch.setenv('VFN_AUTOTUNE', '0')
    T, H, W = 8, 120, 200
    frames, m0 = synth.clip(21, T, H, W)
    names = [f'2021-09-01-12-00-{t:02d}' for t in range(T)]
    fdir = tmp_path / 'frames'
    fdir.mkdir()
    for t in range(T):
        Image.fromarray((frames[t].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(str(fdir / f'{names[t]}.jpg'), quality=95)
    ckpt = str(tmp_path / 'ckpt.pth')
    torch.save({'epoch': 0, 'model': synth.make_state_dict(20200212), 'loss': 0.0, 'seed': 20200212}, ckpt)
    np.savetxt(str(tmp_path / 'ref_bbox.txt'), np.array([(60, 10, 20, 30), (120, 20, 15, 25)]), '%.4f')
    np.savetxt(str(tmp_path / 'homo_mat.txt'), np.array([[1.02, 0.05, -3.0], [0.01, 0.98, 2.0], [1e-4, 2e-4, 1.0]]), '%.4f')
    masks = {}
    for tag in ('with', 'without'):
        run = tmp_path / tag
        mdir = run / 'output' / 'segs' / 'clip' / 'mask'
        mdir.mkdir(parents=True)
        save_seg_mask(m0.numpy().astype(np.uint8), str(mdir / f'{names[0]}.png'), color_palette)
        monkeypatch.chdir(run)
        args = argparse.Namespace(gpu=0, budget=250000, viz=tag == 'with', model_path=ckpt, update_rate=0.1, merge_thres=0.95,
                                  test_path=str(fdir), test_name='clip', size=96, load_workers=2, mem_every=mem_every,
                                  waterlevel=tag == 'with', ref_bbox=str(tmp_path / 'ref_bbox.txt'), homo_mat=str(tmp_path / 'homo_mat.txt'))
        video_seg.main(args, gpu)
        masks[tag] = [open(str(mdir / f'{n}.png'), 'rb').read() for n in names]
    assert masks['with'] == masks['without']
    run = tmp_path / 'with'
    monkeypatch.chdir(run)
    inline_dir = run / 'output' / 'waterlevel' / 'clip_ref'
    assert sorted(p.name for p in (inline_dir / 'viz').iterdir()) == [f'{n}.png' for n in names]
    est_waterlevel.main(est_waterlevel.get_parser(['--test-name', 'clip', '--test-path', str(fdir), '--opt', 'ref', '--out-dir', 'offline',
                                                   '--ref-bbox', str(tmp_path / 'ref_bbox.txt'), '--homo-mat', str(tmp_path / 'homo_mat.txt')]), gpu)
    inline, offline = open(str(inline_dir / 'waterlevel.csv'), 'rb').read(), open(str(run / 'offline' / 'clip_ref' / 'waterlevel.csv'), 'rb').read()
    assert inline == offline and inline.count(b'\n') == T + 1 and b'2021-09-01 12:00:07,' in inline
    for n in names:                                # the annotated overlays are the same images as well
        assert np.array_equal(np.array(Image.open(str(inline_dir / 'viz' / f'{n}.png'))), np.array(Image.open(str(run / 'offline' / 'clip_ref' / 'viz' / f'{n}.png')))), n
