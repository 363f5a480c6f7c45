"""The reference-box tracker of include/vfn_hip.h restated in numpy (int64 and float64, no OpenCV), and a generator of clips whose
motion is known.  Shared by test_track_host.py (the definition follows known motion) and test_track_gpu.py (the kernels equal the
definition bit for bit)."""
import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

MAX_SIDE, MAX_RADIUS = 512, 32


def luma_ref(frame):
    """float32 [3,H,W] -> uint8 [H,W]: bytes by truncation of the f32 product x * 255, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    u8 = (np.asarray(frame, np.float32) * np.float32(255)).astype(np.uint8).astype(np.int64)
    return ((19595 * u8[0] + 38470 * u8[1] + 7471 * u8[2] + 0x8000) >> 16).astype(np.uint8)


class TrackerRef:
    """One clip's tracker state: ``box`` int [R][4] and ``T16`` (a list of int64 [h][w] arrays, 8.8 fixed point)."""

    def __init__(self, luma, boxes, S=16):
        H, W = luma.shape
        self.S = int(S)
        self.box = np.array(boxes, np.int64).reshape(-1, 4)
        assert 1 <= self.S <= MAX_RADIUS
        for x, y, w, h in self.box:
            assert 1 <= w <= MAX_SIDE and 1 <= h <= MAX_SIDE and 0 <= x <= W - w and 0 <= y <= H - h
        self.T16 = [luma[y:y + h, x:x + w].astype(np.int64) << 8 for x, y, w, h in self.box]

    def update(self, luma):
        """One frame for every reference: ``(boxes int [R][4], flags [R], scores float32 [R])`` after it."""
        flags, scores = [], []
        for r in range(len(self.box)):
            ok, score = self._update_one(r, luma)
            flags.append(ok)
            scores.append(score)
        return self.box.copy(), np.array(flags, bool), np.array(scores, np.float32)

    def _update_one(self, r, luma):
        S, T = self.S, self.T16[r]
        x, y, w, h = (int(v) for v in self.box[r])
        H, W = luma.shape
        N = w * h
        A, D = int(T.sum()), int((T * T).sum())
        # every candidate's window out of the luma padded by S zeros (the padding is only ever read by skipped candidates)
        pad = np.pad(luma.astype(np.int64), S)
        n = 2 * S + 1
        B, C, E = (np.zeros((n, n), np.int64) for _ in range(3))
        for j in range(n):                                   # dy = j - S ascending; within it dx = i - S ascending
            win = sliding_window_view(pad[y + j:y + j + h, x:x + w + 2 * S], (h, w))[0]      # [n][h][w]
            B[j], E[j], C[j] = win.sum((1, 2)), (win * win).sum((1, 2)), (win * T).sum((1, 2))
        dy, dx = np.mgrid[-S:S + 1, -S:S + 1]
        num, vp = N * C - A * B, N * E - B * B
        usable = (x + dx >= 0) & (x + dx + w <= W) & (y + dy >= 0) & (y + dy + h <= H) & (vp != 0)
        if not usable.any():
            return False, np.float32(0)
        fnum = num.astype(np.float64)
        with np.errstate(divide='ignore', invalid='ignore'):
            key = np.where(usable, fnum * np.abs(fnum) / vp.astype(np.float64), -np.inf)
        k = int(np.argmax(key.reshape(-1)))                  # the first of equal maxima, in visiting order
        bnum, bvp = int(num.reshape(-1)[k]), int(vp.reshape(-1)[k])
        vt = float(N) * float(D) - float(A) * float(A)
        vv = vt * float(bvp)
        with np.errstate(divide='ignore', invalid='ignore'):
            score = np.float32(np.float64(bnum) / np.sqrt(np.float64(vv)))
        if vt <= 0 or bnum <= 0 or float(bnum) * float(bnum) < 0.25 * vv:
            return False, score
        x, y = x + int(dx.reshape(-1)[k]), y + int(dy.reshape(-1)[k])
        self.box[r, :2] = x, y
        P = luma[y:y + h, x:x + w].astype(np.int64)
        self.T16[r] = T + (((P << 8) - T + 8) >> 4)
        return True, score


def track_clip_ref(lumas, boxes, S=16):
    """The tracker over a clip: init on the first luma, an update on every one of them (the first included).
    ``(box_log int [T][R][4], ok bool [T][R], score float32 [T][R], tracker)``."""
    tr = TrackerRef(lumas[0], boxes, S)
    rows = [tr.update(L) for L in lumas]
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), np.stack([r[2] for r in rows]), tr


def texture(rng, H, W):
    """A smooth random texture in [0.15, 0.85]: noise on a grid of 4-pixel cells plus a little per-pixel detail, blurred."""
    coarse = np.kron(rng.rand((H + 3) // 4 + 1, (W + 3) // 4 + 1), np.ones((4, 4)))[:H, :W]
    t = coarse + 0.25 * rng.rand(H, W)
    for axis in (0, 1):
        for _ in range(2):
            t = (np.roll(t, 1, axis) + t + np.roll(t, -1, axis)) / 3
    t = (t - t.min()) / (t.max() - t.min())
    return 0.15 + 0.7 * t


def make_clip(seed, T, H, W, boxes, S, replaced=(), shifts=None, gain_step=0.04, offset_step=0.004, sigma=0.01):
    """``(frames float32 [T][3][H][W] in [0,1], disp int [T][2])``: one texture seen through a camera that shakes by whole pixels.
    ``disp[t]`` = (dx, dy) by which the scene, and with it every box, stands displaced in frame t against frame 0; the steps are
    drawn from -S .. S (``shifts``: given steps [T][2] instead), mirrored where a box would leave the image, and cut down around the
    frames of ``replaced`` so that the step ACROSS a run of them stays within S (the tracker re-acquires from the last good frame).  Frame 0 is
    not displaced.  Gain falls by ``gain_step`` a frame, the offset rises, Gaussian noise of ``sigma``; a replaced frame is
    uniform noise."""
    rng = np.random.RandomState(seed)
    M = T * S + S + 1                                        # margin of the canvas
    canvas = np.stack([texture(rng, H + 2 * M, W + 2 * M) for _ in range(3)])
    canvas[1:] = 0.5 * canvas[1:] + 0.5 * canvas[0]          # the channels differ but share their structure
    boxes = np.array(boxes).reshape(-1, 4)
    run = max([1 + sum(1 for k in range(1, T) if all(t + j in replaced for j in range(k + 1))) for t in replaced] or [0])
    disp, cur = [], np.zeros(2, np.int64)
    for t in range(T):
        if t == 0:
            step = np.zeros(2, np.int64)
        elif shifts is not None:
            step = np.array(shifts[t], np.int64)
        else:
            lim = S // (1 + run) if (t in replaced or t - 1 in replaced) else S
            step = rng.randint(-lim, lim + 1, 2)
            for a, (lo, hi, size) in enumerate(((boxes[:, 0], boxes[:, 0] + boxes[:, 2], W), (boxes[:, 1], boxes[:, 1] + boxes[:, 3], H))):
                if (lo + cur[a] + step[a] < 0).any() or (hi + cur[a] + step[a] > size).any():
                    step[a] = -step[a]
        cur = cur + step
        disp.append(cur.copy())
    frames = np.empty((T, 3, H, W), np.float32)
    for t, (dx, dy) in enumerate(disp):
        if t in replaced:
            frames[t] = rng.rand(3, H, W)
            continue
        view = canvas[:, M - dy:M - dy + H, M - dx:M - dx + W]
        f = (1.0 - gain_step * t) * view + offset_step * t + sigma * rng.randn(3, H, W)
        frames[t] = np.clip(f, 0.0, 1.0)
    return frames, np.array(disp)
