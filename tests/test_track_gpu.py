"""The tracker kernels (``csrc/track.hip``) against the definition restated in numpy (tests/track_ref.py): every logged box, flag and
the whole template equal, the score within 1e-6; the device-box scan and draw against the host-box entry points; and the
estimator with tracking end to end, stand-alone and inside ``video_seg.main``."""
import argparse
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from track_ref import TrackerRef, luma_ref, make_clip

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ kernels against the restatement
def test_luma_equals_the_restatement(gpu):
    from vfloodnet_amd import ops
    frame = np.random.RandomState(0).rand(3, 37, 53).astype(np.float32)
    frame[:, 0, :4] = [[0.0, 1.0, 0.5, 1 / 255]] * 3
    got = ops.track_luma(torch.from_numpy(frame).to(gpu)).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, luma_ref(frame))


def stripes(T, H=48, W=64):
    return [np.ascontiguousarray(np.tile(np.array([10, 80, 200, 120], np.uint8), (H, W // 4)))] * T


@functools.lru_cache(maxsize=None)
def case(name):
    """``(lumas or frames, is_frames, boxes, S)`` of a named case; built once."""
    if name == 'odd':                                     # neither side a multiple of 4
        boxes, S = [(40, 30, 23, 17)], 5
        return make_clip(11, 12, 96, 128, boxes, S)[0], True, boxes, S
    if name == 'edges':                                   # from 2 px off the top-left corner to the bottom-right edge: candidates
        boxes, S = [(2, 2, 23, 17)], 5                    # are skipped on every side (24 frames: 103 x 77 pixels in steps <= 5)
        steps = [(0, 0)] + [(min(5, 103 - 5 * k), min(4, 77 - 4 * k)) for k in range(21)] + [(0, 0), (0, 0)]
        steps = [(max(a, 0), max(b, 0)) for a, b in steps]
        frames, disp = make_clip(12, 24, 96, 128, boxes, S, shifts=steps)
        assert disp[-1].tolist() == [103, 77]
        return frames, True, boxes, S
    if name == 'three':                                   # R = 3 boxes of different sizes in one call
        boxes, S = [(40, 30, 23, 17), (80, 20, 8, 30), (20, 60, 41, 12)], 5
        return make_clip(13, 12, 96, 128, boxes, S)[0], True, boxes, S
    if name == 'big':                                     # more than one LDS tile each way, the maximum radius
        boxes, S = [(60, 60, 130, 70)], 32
        return make_clip(14, 12, 200, 260, boxes, S)[0], True, boxes, S
    if name == 'thin':                                    # w = 1, h = 1, both
        boxes, S = [(30, 30, 1, 17), (50, 40, 23, 1), (70, 50, 1, 1)], 5
        return make_clip(15, 12, 96, 128, boxes, S)[0], True, boxes, S
    if name == 'stripes':                                 # period 4: many candidates tie exactly
        return stripes(3), False, [(20, 20, 9, 7)], 5
    if name == 'replaced':
        boxes, S = [(40, 30, 23, 17)], 6
        return make_clip(16, 12, 96, 128, boxes, S, replaced=(5,))[0], True, boxes, S
    if name == 'constant':                                # every vp == 0: no candidate
        return [np.full((48, 64), 9, np.uint8)] * 3, False, [(20, 20, 9, 7)], 5
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per frame ``(boxes, flags, scores, templates)`` of the restatement; computed once and left unchanged."""
    data, is_frames, boxes, S = case(name)
    lumas = [luma_ref(f) for f in data] if is_frames else data
    tr = TrackerRef(lumas[0], boxes, S)
    rows = []
    for L in lumas:
        box, ok, score = tr.update(L)
        rows.append((box, ok, score, [t.copy() for t in tr.T16]))
    return rows


def run_device(gpu, name):
    from vfloodnet_amd import ops
    data, is_frames, boxes, S = case(name)
    T, R = len(data), len(boxes)
    logs = (torch.full((T, R, 4), -7, dtype=torch.int32, device=gpu), torch.full((T, R), -7, dtype=torch.int32, device=gpu),
            torch.full((T, R), -7.0, dtype=torch.float32, device=gpu))
    state, templates = None, []
    for t, d in enumerate(data):
        luma = ops.track_luma(torch.from_numpy(d).to(gpu)) if is_frames else torch.from_numpy(d).to(gpu)
        if state is None:
            state = ops.track_init(luma, np.array(boxes, np.int32), S)
        ops.track_update(state, luma, *logs, t)
        templates.append([state.template(r) for r in range(R)])
    assert not state.acc.cpu().numpy().any()              # the sums are left zero for the next frame
    return [l.cpu().numpy() for l in logs], templates


@pytest.mark.parametrize('name', ['odd', 'edges', 'three', 'big', 'thin', 'stripes', 'replaced', 'constant'])
def test_update_equals_the_restatement(gpu, name):
    (box, ok, score), templates = run_device(gpu, name)
    ref = reference(name)
    for t, (rbox, rok, rscore, rtpl) in enumerate(ref):
        assert np.array_equal(box[t], rbox), (t, box[t], rbox)
        assert np.array_equal(ok[t].astype(bool), rok) and set(np.unique(ok[t])) <= {0, 1}, t
        for got, want in zip(templates[t], rtpl):
            assert np.array_equal(got, want), t
        print(name, t, box[t].tolist(), ok[t].tolist(), score[t].tolist(), rscore.tolist())
        assert np.allclose(score[t], rscore, rtol=0, atol=1e-6, equal_nan=True), (t, score[t], rscore)
    oks = np.stack([r[1] for r in ref])
    boxes0 = np.array(case(name)[2])
    if name in ('odd', 'three', 'big', 'edges'):          # the case is what it says: the boxes are followed, and they move
        assert oks.all() and (ref[-1][0][:, :2] != boxes0[:, :2]).any()
    if name == 'edges':
        assert ref[-1][0][0].tolist() == [105, 79, 23, 17]
    if name == 'stripes':                                 # the first of the tied candidates: dy = -5, dx = -4
        assert ref[0][0][0].tolist() == [16, 15, 9, 7] and oks.all()
    if name == 'replaced':                                # box and template of frame 4 survive frame 5, and frame 6 finds it again
        assert oks[:, 0].tolist() == [True] * 5 + [False] + [True] * 6
        assert np.array_equal(box[5], box[4]) and np.array_equal(templates[5][0], templates[4][0])
    if name == 'constant':
        assert not oks.any() and (score == 0).all() and (box == boxes0).all()


def test_entry_points_refuse_bad_arguments(gpu):
    from vfloodnet_amd import _lib, ops
    L = _lib.lib()
    H, W, S = 600, 600, 5
    luma = torch.zeros(H, W, dtype=torch.uint8, device=gpu)
    frame = torch.zeros(3, H, W, dtype=torch.float32, device=gpu)
    state = torch.zeros(33 * 4, dtype=torch.int32, device=gpu)
    t16 = torch.zeros(513 * 513, dtype=torch.int16, device=gpu)
    acc = torch.zeros(33 * 65 * 65 * 3, dtype=torch.int64, device=gpu)
    logs = [torch.zeros(2, 33, 4, dtype=torch.int32, device=gpu), torch.zeros(2, 33, dtype=torch.int32, device=gpu),
            torch.zeros(2, 33, dtype=torch.float32, device=gpu)]
    p, s = _lib.ptr, _lib.stream()

    def ints(rows):
        return (C.c_int * (len(rows) * len(rows[0])))(*[v for r in rows for v in r])

    def init(boxes=((10, 10, 20, 20),), R=None, S=S, luma_=luma, state_=state, t16_=t16, acc_=acc, t16_n=None, acc_n=None):
        return L.vfn_track_init(p(luma_), H, W, ints(boxes) if boxes else None, len(boxes) if R is None else R, S, p(state_), p(t16_),
                                t16.numel() if t16_n is None else t16_n, p(acc_), acc.numel() if acc_n is None else acc_n, s)

    def update(sizes=((20, 20),), R=None, S=S, t=0, luma_=luma, state_=state, t16_=t16, acc_=acc, logs_=logs, acc_n=None):
        return L.vfn_track_update(p(luma_), H, W, ints(sizes) if sizes else None, len(sizes) if R is None else R, S, p(state_), p(t16_),
                                  t16.numel(), p(acc_), acc.numel() if acc_n is None else acc_n, p(logs_[0]), p(logs_[1]), p(logs_[2]),
                                  2, t, s)
    assert init() == 0 and update() == 0 and update(t=1) == 0
    assert init(boxes=((10, 10, 512, 512),)) == 0                                  # the caps themselves are fine
    bad = [init(boxes=((10, 10, 513, 20),)), init(boxes=((10, 10, 20, 513),)), init(boxes=((10, 10, 0, 20),)),
           init(S=0), init(S=33), init(boxes=((1, 1, 2, 2),) * 33), init(boxes=((1, 1, 2, 2),), R=0),
           init(boxes=((590, 10, 20, 20),)), init(boxes=((10, 590, 20, 20),)), init(boxes=((-1, 10, 20, 20),)), init(boxes=((10, -1, 20, 20),)),
           init(boxes=None, R=1), init(luma_=None), init(state_=None), init(t16_=None), init(acc_=None),
           init(t16_n=399), init(acc_n=11 * 11 * 3 - 1),
           update(sizes=((513, 20),)), update(sizes=((20, 0),)), update(S=0), update(S=33), update(sizes=((2, 2),) * 33),
           update(t=2), update(t=-1), update(sizes=None, R=1), update(luma_=None), update(state_=None), update(t16_=None),
           update(acc_=None), update(logs_=[None, logs[1], logs[2]]), update(logs_=[logs[0], None, logs[2]]),
           update(logs_=[logs[0], logs[1], None]), update(acc_n=11 * 11 * 3 - 1),
           L.vfn_track_luma_f32(None, p(luma), H, W, s), L.vfn_track_luma_f32(p(frame), None, H, W, s),
           L.vfn_track_luma_f32(p(frame), p(luma), 0, W, s)]
    assert bad == [1] * len(bad)                                                   # VFN_ERR_ARG, and nothing was launched
    lab, ov, log = torch.zeros(H, W, dtype=torch.uint8, device=gpu), torch.zeros(H, W, 3, dtype=torch.uint8, device=gpu), logs[1]
    bad = [L.vfn_waterline_scan_dev(None, H, W, p(state), 1, 1, p(log), 2, 0, s), L.vfn_waterline_scan_dev(p(lab), H, W, None, 1, 1, p(log), 2, 0, s),
           L.vfn_waterline_scan_dev(p(lab), H, W, p(state), 1, 1, None, 2, 0, s), L.vfn_waterline_scan_dev(p(lab), H, W, p(state), 33, 1, p(log), 2, 0, s),
           L.vfn_waterline_scan_dev(p(lab), H, W, p(state), 1, 1, p(log), 2, 2, s), L.vfn_waterline_scan_dev(p(lab), H, W, p(state), 1, 256, p(log), 2, 0, s),
           L.vfn_waterlevel_draw_dev(None, H, W, p(state), 1, p(log), 2, 0, s), L.vfn_waterlevel_draw_dev(p(ov), H, W, None, 1, p(log), 2, 0, s),
           L.vfn_waterlevel_draw_dev(p(ov), H, W, p(state), 1, None, 2, 0, s), L.vfn_waterlevel_draw_dev(p(ov), H, W, p(state), 33, p(log), 2, 0, s),
           L.vfn_waterlevel_draw_dev(p(ov), H, W, p(state), 1, p(log), 2, -1, s)]
    assert bad == [1] * len(bad)
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        ops.track_init(luma, [(590, 10, 20, 20)], 5)
    with pytest.raises(ValueError):
        ops.track_init(luma, [(10, 10, 20, 20)], 33)


# ------------------------------------------------------------------------------------------------ scan and draw under device boxes
def scan_ref(label, boxes, water=1):
    """The column scan under boxes: -1 for a key point without a row of the image below it."""
    H, W = label.shape
    out = []
    for x, y, w, h in boxes:
        kx, ky, d = int(x + w / 2), int(y + h), -1
        if 0 <= kx < W and 0 <= ky < H - 1:
            for row in range(ky + 1, H):
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


def boxes_for(kps):
    """Boxes whose key points (int(x + w / 2), y + h) are ``kps``."""
    return [(kx - 2, max(ky - 3, 0), 4, ky - max(ky - 3, 0)) for kx, ky in kps]


def test_scan_under_device_boxes_equals_the_host_entry_point(gpu):
    from vfloodnet_amd import ops, waterlevel
    H, W = 40, 64                                  # the five references of test_waterlevel_gpu's scan test
    lab = np.zeros((H, W), np.uint8)
    kps = [(3, 10), (9, 10), (20, 5), (30, H - 1), (40, 7)]
    lab[12:, 3] = 1
    lab[11:, 9] = 1
    lab[0:6, 20] = 1
    lab[:, 30] = 1
    lab[10:20, 40] = 2
    lab[20:, 40] = 1
    boxes = np.array(boxes_for(kps), np.int32)
    assert waterlevel.keypoints(boxes).tolist() == [list(k) for k in kps]
    for water, want in ((1, [2, 1, -1, -1, 13]), (2, [-1, -1, -1, -1, 3])):
        host = torch.full((3, 5), -7, dtype=torch.int32, device=gpu)
        dev = torch.full((3, 5), -7, dtype=torch.int32, device=gpu)
        ops.waterline_scan(torch.from_numpy(lab).to(gpu), np.array(kps, np.int32), host, 1, water)
        ops.waterline_scan_dev(torch.from_numpy(lab).to(gpu), torch.from_numpy(boxes).to(gpu), dev, 1, water)
        assert torch.equal(host, dev) and dev.cpu().numpy()[1].tolist() == want == scan_ref(lab, boxes, water)
    H, W = 300, 17                                 # beyond one stride of the wave
    lab = np.zeros((H, W), np.uint8)
    lab[257:, 5] = 1
    lab[299, 6] = 1
    kps = [(5, 2), (6, 0), (7, 0), (5, 256), (5, 192)]
    boxes = np.array(boxes_for(kps), np.int32)
    host, dev = (torch.zeros((1, 5), dtype=torch.int32, device=gpu) for _ in range(2))
    ops.waterline_scan(torch.from_numpy(lab).to(gpu), kps, host, 0)
    ops.waterline_scan_dev(torch.from_numpy(lab).to(gpu), torch.from_numpy(boxes).to(gpu), dev, 0)
    assert torch.equal(host, dev) and dev.cpu().numpy()[0].tolist() == [255, 299, -1, 1, 65]


def test_draw_under_device_boxes_equals_the_host_entry_point(gpu):
    from vfloodnet_amd import ops
    H, W = 48, 64                                  # the case of test_waterlevel_gpu's draw test
    ov = np.random.RandomState(3).randint(0, 256, (H, W, 3)).astype(np.uint8)
    boxes = np.array([(10, 5, 8, 10), (50, 30, 13, 17), (30, 4, 7, 9), (20, 20, 6, 5), (40, 2, 3, 1)], np.int32)
    log = torch.tensor([[0] * 5, [20, 9, -1, 1, 60]], dtype=torch.int32, device=gpu)
    host, dev = torch.from_numpy(ov).to(gpu), torch.from_numpy(ov).to(gpu)
    ops.waterlevel_draw(host, boxes, log, 1)
    out = ops.waterlevel_draw_dev(dev, torch.from_numpy(boxes).to(gpu), log, 1)
    assert out.data_ptr() == dev.data_ptr() and torch.equal(host, dev)
    assert np.array_equal(dev.cpu().numpy(), draw_ref(ov, boxes.tolist(), [20, 9, -1, 1, 60]))


def test_device_boxes_at_and_past_the_image_edge(gpu):
    """Key points on the last row (ky = H - 1), below it (ky = H) and right of the image (kx = W) log -1 and read nothing; the
    boxes are drawn clipped.  A box of nonsense (what an uninitialised row would hold) is neither scanned nor drawn."""
    from vfloodnet_amd import ops
    H, W = 40, 64
    lab = np.ones((H, W), np.uint8)
    boxes = [(10, 30, 8, 9), (20, 30, 8, 10), (60, 5, 8, 10), (30, 5, 8, 10), (2 ** 30, -2 ** 31, 2 ** 31 - 1, -5), (-3, 35, 6, 20)]
    assert [(int(x + w / 2), y + h) for x, y, w, h in boxes[:4]] == [(14, H - 1), (24, H), (W, 15), (34, 15)]
    dev_boxes = torch.tensor(boxes, dtype=torch.int64).to(torch.int32).to(gpu)
    log = torch.full((1, 6), -7, dtype=torch.int32, device=gpu)
    ops.waterline_scan_dev(torch.from_numpy(lab).to(gpu), dev_boxes, log, 0)
    assert log.cpu().numpy()[0].tolist() == [-1, -1, -1, 1, -1, -1]
    ov = np.random.RandomState(4).randint(0, 256, (H, W, 3)).astype(np.uint8)
    log = torch.tensor([[30, 30, 30, 30, 30, 30]], dtype=torch.int32, device=gpu)       # lines that run off the image too
    dev = torch.from_numpy(ov).to(gpu)
    ops.waterlevel_draw_dev(dev, dev_boxes, log, 0)
    drawn = boxes[:4] + boxes[5:]
    assert np.array_equal(dev.cpu().numpy(), draw_ref(ov, drawn, [30] * 5))


# ------------------------------------------------------------------------------------------------ the estimator with tracking
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1
KEYSTONE = np.array([[1.02, 0.05, -3.0], [0.01, 0.98, 2.0], [1e-4, 2e-4, 1.0]], np.float64)


def warp_ref(img, homo):
    """uint8 [H,W] or [H,W,C]: OpenCV's fixed-point bilinear remap stated in integers (include/vfn_hip.h)."""
    a = img[:, :, None] if img.ndim == 2 else img
    H, W, _ = a.shape
    m = np.linalg.inv(np.asarray(homo, np.float64)).reshape(9)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    Wd = m[6] * x + m[7] * y + m[8]
    with np.errstate(divide='ignore'):
        s = np.where(Wd != 0, 32.0 / Wd, 0.0)
    X = np.rint(np.clip((m[0] * x + m[1] * y + m[2]) * s, INT_MIN, INT_MAX)).astype(np.int64)
    Y = np.rint(np.clip((m[3] * x + m[4] * y + m[5]) * s, INT_MIN, INT_MAX)).astype(np.int64)
    sx, ax, sy, ay = X >> 5, (X & 31)[..., None], Y >> 5, (Y & 31)[..., None]

    def tap(yy, xx):
        ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
        return np.where(ok[..., None], a[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), 0)
    acc = ((32 - ay) * ((32 - ax) * tap(sy, sx) + ax * tap(sy, sx + 1)) + ay * ((32 - ax) * tap(sy + 1, sx) + ax * tap(sy + 1, sx + 1)) + 512) >> 10
    return acc.astype(np.uint8).reshape(img.shape)


T_CLIP, H_CLIP, W_CLIP, S_CLIP = 16, 96, 128, 6
CLIP_BOXES = [(30, 14, 23, 17), (84, 20, 16, 21)]
CLIP_NAMES = [f'2021-09-01-12-00-{2 * t:02d}' for t in range(T_CLIP)]


@functools.lru_cache(maxsize=None)
def shaky_clip():
    """``(frames uint8 [T][H][W][3], labels uint8 [T][H][W])``: the camera shakes, the water line rises by two rows a frame."""
    frames, disp = make_clip(21, T_CLIP, H_CLIP, W_CLIP, CLIP_BOXES, S_CLIP)
    assert len({int(d) for d in disp[:, 1]}) > 3
    labels = np.zeros((T_CLIP, H_CLIP, W_CLIP), np.uint8)
    for t in range(T_CLIP):
        labels[t, 90 - 2 * t:, :] = 1
    return np.ascontiguousarray((frames * 255).astype(np.uint8).transpose(0, 2, 3, 1)), labels


@functools.lru_cache(maxsize=None)
def restated_pipeline(calibrated):
    """``(csv bytes, box_log, ok)``: the restated tracker over the (warped) frames, the scan under its boxes, then the product's
    host steps (which test_waterlevel_gpu pins to scipy and pandas)."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import waterlevel
    frames, labels = shaky_clip()
    homo = KEYSTONE if calibrated else None
    lumas, offsets, tr, boxes, oks = [], [], None, [], []
    for t in range(T_CLIP):
        u8, lab = frames[t], labels[t]
        if homo is not None:
            u8, lab = warp_ref(u8, homo), warp_ref(lab, homo)
        L = luma_ref(u8.transpose(2, 0, 1).astype(np.float32) / np.float32(255))
        if tr is None:
            tr = TrackerRef(L, CLIP_BOXES, S_CLIP)
        box, ok, _ = tr.update(L)
        boxes.append(box)
        oks.append(ok)
        offsets.append(scan_ref(lab, box.tolist()))
    levels = waterlevel.levels_from_offsets(np.array(offsets))
    for r in range(levels.shape[1]):
        levels[:, r] = waterlevel.smooth(levels[:, r])
    return waterlevel.csv_bytes(CLIP_NAMES, levels, waterlevel.nanmean_rows(levels)), np.stack(boxes), np.stack(oks)


@pytest.fixture(scope='module')
def clip_on_disk(tmp_path_factory):
    from PIL import Image
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd.data import save_seg_mask, color_palette
    root = tmp_path_factory.mktemp('shaky')
    frames, labels = shaky_clip()
    (root / 'frames').mkdir()
    (root / 'masks').mkdir()
    for t, n in enumerate(CLIP_NAMES):
        Image.fromarray(frames[t]).save(str(root / 'frames' / f'{n}.png'))
        save_seg_mask(labels[t], str(root / 'masks' / f'{n}.png'), color_palette)
    np.savetxt(str(root / 'ref_bbox.txt'), np.array(CLIP_BOXES), '%.4f')
    np.savetxt(str(root / 'homo_mat.txt'), KEYSTONE, '%.6f')
    return root


@pytest.mark.parametrize('calibrated', [False, True], ids=['plain', 'calibrated'])
def test_estimator_with_tracking_equals_the_restated_pipeline(gpu, clip_on_disk, calibrated):
    from vfloodnet_amd import est_waterlevel
    root = clip_on_disk
    imgs = [str(root / 'frames' / f'{n}.png') for n in CLIP_NAMES]
    masks = [str(root / 'masks' / f'{n}.png') for n in CLIP_NAMES]
    out = {}
    for track in (True, False):
        d = root / f'out_{int(calibrated)}_{int(track)}'
        meter = est_waterlevel.est_by_reference(imgs, masks, str(d), str(root), 'clip', gpu, str(root / 'ref_bbox.txt'),
                                                str(root / 'homo_mat.txt') if calibrated else None, calibrated, viz=track and calibrated,
                                                track=track, track_radius=S_CLIP)
        out[track] = open(str(d / 'waterlevel.csv'), 'rb').read()
        if track:
            want_csv, want_box, want_ok = restated_pipeline(calibrated)
            assert np.array_equal(meter.box_log, want_box) and np.array_equal(meter.track_ok, want_ok)
            assert meter.track_ok.dtype == bool and meter.track_score.shape == (T_CLIP, 2) and want_ok.all()
            assert (meter.box_log[-1, :, :2] != np.array(CLIP_BOXES)[:, :2]).any()
            assert out[True] == want_csv
        else:
            assert not hasattr(meter, 'box_log')
    assert out[True] != out[False]                         # the static boxes measure the camera


def test_meter_warns_once_per_failed_frame_after_the_clip(gpu):
    from vfloodnet_amd import waterlevel
    frames, _ = make_clip(16, 8, 96, 128, [(40, 30, 23, 17)], 6, replaced=(3, 5))
    meter = waterlevel.WaterLevelMeter([(40, 30, 23, 17)], None, frames_hint=2, device=gpu, track=True, track_radius=6)
    lab = torch.zeros(96, 128, dtype=torch.uint8, device=gpu)
    with pytest.raises(ValueError):
        meter.measure(lab)                                 # a tracking meter needs the frame
    with pytest.raises(ValueError):
        meter.measure(lab, torch.from_numpy(frames[0]).to(gpu), bbox=[(1, 1, 2, 2)])
    assert meter.t == 0
    for t in range(8):
        ov = meter.measure(lab, torch.from_numpy(frames[t]).to(gpu), f'f{t}', overlay=t % 2 == 0)
        assert (ov is None) == (t % 2 == 1)
    with pytest.warns(UserWarning) as rec:
        meter.finish()
    assert [str(w.message) for w in rec] == ['Tracker failed at frame f3.', 'Tracker failed at frame f5.']
    assert meter.track_ok[:, 0].tolist() == [True, True, True, False, True, False, True, True] and meter.box_log.shape == (8, 1, 4)


def test_measure_with_tracking_never_waits_for_the_device(gpu):
    from vfloodnet_amd import waterlevel
    frames, labels = shaky_clip()
    meter = waterlevel.WaterLevelMeter(CLIP_BOXES, KEYSTONE, frames_hint=8, device=gpu, track=True, track_radius=S_CLIP)
    from vfloodnet_amd import ops
    dev = [(torch.from_numpy(labels[t]).to(gpu), ops.to_tensor_device(torch.from_numpy(frames[t]).to(gpu))) for t in range(4)]
    meter.measure(dev[0][0], dev[0][1], CLIP_NAMES[0])
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for t in range(1, 4):
            meter.measure(dev[t][0], dev[t][1], CLIP_NAMES[t])
    finally:
        torch.cuda.set_sync_debug_mode('default')
    meter.finish()
    assert np.array_equal(meter.box_log, restated_pipeline(True)[1][:4])


# ------------------------------------------------------------------------------------------------ inline = offline
def main_args(tmp_path, fdir, ckpt, mem_every, **more):
    return argparse.Namespace(gpu=0, budget=250000, viz=True, model_path=ckpt, update_rate=0.1, merge_thres=0.95, test_path=str(fdir),
                              test_name='clip', size=96, load_workers=2, mem_every=mem_every, waterlevel=True,
                              ref_bbox=str(tmp_path / 'ref_bbox.txt'), homo_mat=str(tmp_path / 'homo_mat.txt'), **more)


def write_clip(tmp_path, T=8, H=120, W=200):
    from PIL import Image
    from tools import synth
    from vfloodnet_amd.data import save_seg_mask, color_palette
    frames, m0 = synth.clip(21, T, H, W)
    names = [f'2021-09-01-12-00-{t:02d}' for t in range(T)]
    fdir = tmp_path / 'frames'
    fdir.mkdir()
    for t in range(T):
        Image.fromarray((frames[t].permute(1, 2, 0).numpy() * 255).astype(np.uint8)).save(str(fdir / f'{names[t]}.jpg'), quality=95)
    ckpt = str(tmp_path / 'ckpt.pth')
    torch.save({'epoch': 0, 'model': synth.make_state_dict(20200212), 'loss': 0.0, 'seed': 20200212}, ckpt)
    np.savetxt(str(tmp_path / 'ref_bbox.txt'), np.array([(60, 10, 20, 30), (120, 20, 15, 25)]), '%.4f')
    np.savetxt(str(tmp_path / 'homo_mat.txt'), KEYSTONE, '%.4f')

    def first_mask(run):
        mdir = run / 'output' / 'segs' / 'clip' / 'mask'
        mdir.mkdir(parents=True)
        save_seg_mask(m0.numpy().astype(np.uint8), str(mdir / f'{names[0]}.png'), color_palette)
    return names, fdir, ckpt, first_mask


def outputs(d, names):
    return [open(str(d / 'waterlevel.csv'), 'rb').read()] + [open(str(d / 'viz' / f'{n}.png'), 'rb').read() for n in names]


@pytest.mark.parametrize('mem_every', [1, 3])
def test_main_with_tracking_equals_est_waterlevel_over_its_masks(gpu, tmp_path, monkeypatch, mem_every):
    """``video_seg.main --waterlevel --track on`` writes the ``waterlevel.csv`` and the annotated overlays that ``est_waterlevel
    --track on`` computes from the mask PNGs of that run."""
    from PIL import Image
    from vfloodnet_amd import video_seg, est_waterlevel
    monkeypatch.setenv('VFN_AUTOTUNE', '0')
    names, fdir, ckpt, first_mask = write_clip(tmp_path)
    run = tmp_path / 'run'
    first_mask(run)
    monkeypatch.chdir(run)
    runner = video_seg.main(main_args(tmp_path, fdir, ckpt, mem_every, track='on', track_radius=7), gpu)
    assert runner.waterlevel.track and runner.waterlevel.box_log.shape == (len(names), 2, 4)
    offline = est_waterlevel.main(est_waterlevel.get_parser(['--test-name', 'clip', '--test-path', str(fdir), '--opt', 'ref', '--out-dir', 'offline',
                                                             '--ref-bbox', str(tmp_path / 'ref_bbox.txt'), '--homo-mat', str(tmp_path / 'homo_mat.txt'),
                                                             '--track', 'on', '--track-radius', '7']), gpu)
    assert np.array_equal(runner.waterlevel.box_log, offline.box_log) and np.array_equal(runner.waterlevel.track_ok, offline.track_ok)
    inline_dir, offline_dir = run / 'output' / 'waterlevel' / 'clip_ref', run / 'offline' / 'clip_ref'
    a, b = open(str(inline_dir / 'waterlevel.csv'), 'rb').read(), open(str(offline_dir / 'waterlevel.csv'), 'rb').read()
    assert a == b and a.count(b'\n') == len(names) + 1
    for n in names:
        assert np.array_equal(np.array(Image.open(str(inline_dir / 'viz' / f'{n}.png'))), np.array(Image.open(str(offline_dir / 'viz' / f'{n}.png')))), n


def test_track_off_is_the_run_without_the_flag(gpu, tmp_path, monkeypatch):
    """``--track off`` changes no byte: ``video_seg.main`` with it, ``est_waterlevel`` with it and ``est_waterlevel`` without the
    flag write the same ``waterlevel.csv`` and overlays (the last equals ``main`` without the flag by test_waterlevel_gpu)."""
    from vfloodnet_amd import video_seg, est_waterlevel
    monkeypatch.setenv('VFN_AUTOTUNE', '0')
    names, fdir, ckpt, first_mask = write_clip(tmp_path)
    run = tmp_path / 'run'
    first_mask(run)
    monkeypatch.chdir(run)
    runner = video_seg.main(main_args(tmp_path, fdir, ckpt, 1, track='off'), gpu)
    assert not runner.waterlevel.track and not hasattr(runner.waterlevel, 'box_log')
    base = ['--test-name', 'clip', '--test-path', str(fdir), '--opt', 'ref', '--ref-bbox', str(tmp_path / 'ref_bbox.txt'),
            '--homo-mat', str(tmp_path / 'homo_mat.txt')]
    est_waterlevel.main(est_waterlevel.get_parser(base + ['--out-dir', 'plain']), gpu)
    est_waterlevel.main(est_waterlevel.get_parser(base + ['--out-dir', 'off', '--track', 'off']), gpu)
    plain = outputs(run / 'plain' / 'clip_ref', names)
    assert outputs(run / 'off' / 'clip_ref', names) == plain
    inline = run / 'output' / 'waterlevel' / 'clip_ref'
    assert open(str(inline / 'waterlevel.csv'), 'rb').read() == plain[0]
