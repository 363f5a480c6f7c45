"""Water level by reference object: the ``ref`` estimator of ``est_waterlevel.py`` (``estimation/reference_tracking.py:116-218``)
on the tensors the frame loop already holds on the device.

Per frame: two perspective warps (frame and label map, ``vfn_warp_perspective_*``), a column scan below each reference box
(``vfn_waterline_scan``) and the annotated overlay (``vfn_overlay_u8`` + ``vfn_waterlevel_draw_u8``).  With ``track=True`` the
boxes follow the (warped) frame: ``vfn_track_*`` (a translation-only correlation tracker stated in ``include/vfn_hip.h``, not
``cv2.TrackerCSRT``) moves them on the device and the scan and the drawing read them there.  The scan results collect
in a device log; ``WaterLevelMeter.finish`` fetches it once per clip and runs the reference's host steps (carry-forward / NaN
rule, Gaussian smoothing, mean over the references); ``write_csv`` writes ``waterlevel.csv`` as ``DataFrame.to_csv`` would.

Not built: the interactive point / ROI pickers (a missing record file is an error that names it), CSRT itself
(the built tracker adapts neither scale nor rotation and claims no agreement with OpenCV's boxes) and the matplotlib plot.
No OpenCV, pandas, scipy or matplotlib is imported.
"""
import csv
import io
import os
import warnings
from datetime import datetime

import numpy as np
import torch

from . import ops
from .data import color_palette

WATER_LABEL = 1                              # reference_tracking.py:21
TIME_FORMAT = '%Y-%m-%d-%H-%M-%S'            # reference_tracking.py:179


# ------------------------------------------------------------------------------------------------ host steps
def smooth(x, sigma=2.0, truncate=4.0):
    """``scipy.ndimage.gaussian_filter1d(x, sigma=2, mode='nearest')`` (reference_tracking.py:212) in numpy: weights
    exp(-k^2 / (2 sigma^2)) over k = -8 .. 8, normalised; the series is continued with its end values; a NaN makes the 8
    samples either side of it NaN."""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 1:
        raise ValueError('smooth: a 1-D series')
    if x.size == 0:
        return x.copy()
    radius = int(truncate * float(sigma) + 0.5)
    k = np.arange(-radius, radius + 1)
    w = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    w = w / w.sum()
    pad = np.concatenate([np.full(radius, x[0]), x, np.full(radius, x[-1])])
    # scipy's summation order for a symmetric kernel (ni_filters.c, NI_Correlate1D): the centre tap, then the pairs from the
    # outermost inwards, each pair added before it is weighted -- so that the values, and with them the CSV, agree to the bit
    n = x.size
    out = pad[radius:radius + n] * w[radius]
    for j in range(-radius, 0):
        out = out + (pad[radius + j:radius + j + n] + pad[radius - j:radius - j + n]) * w[j + radius]
    return out


def levels_from_offsets(offsets):
    """The per-frame estimates of reference_tracking.py:190-206 from the scan log int [T][R] (offset of the first water row below
    the key point, -1 = none): an offset of 1 is NaN, a larger one is the estimate, and a frame without water keeps the
    previous frame's estimate (0 before the first frame; a NaN is carried the same way).  float64 [T][R]."""
    off = np.asarray(offsets)
    out = np.empty(off.shape, np.float64)
    prev = np.zeros(off.shape[1], np.float64)
    for t in range(off.shape[0]):
        d = off[t]
        prev = np.where(d < 0, prev, np.where(d == 1, np.nan, d.astype(np.float64)))
        out[t] = prev
    return out


def nanmean_rows(x):
    """``np.nanmean(x, axis=1)`` without its warning for an all-NaN row (which gives NaN)."""
    ok = ~np.isnan(x)
    n = ok.sum(1)
    s = np.where(ok, x, 0.0).sum(1)
    return np.where(n > 0, s / np.maximum(n, 1), np.nan)


def keypoints(ref_bbox):
    """int [R][2]: (int(x + w / 2), int(y + h)) of every box after its values were truncated to int (reference_tracking.py:192-195)."""
    out = []
    for box in _boxes(ref_bbox):
        x, y, w, h = (int(v) for v in box)
        out.append([int(x + w / 2), int(y + h)])
    return np.asarray(out, np.int32).reshape(-1, 2)


def _boxes(ref_bbox):
    a = np.asarray(ref_bbox, dtype=np.float64)
    if a.ndim == 1:
        a = a[None]
    if a.ndim != 2 or a.shape[1] != 4 or a.shape[0] < 1 or not np.isfinite(a).all():
        raise ValueError(f'reference boxes: expected finite (x, y, w, h) rows, got shape {a.shape}')
    return a.astype(np.int64).astype(np.int32)              # truncation towards zero, as int(v)


def load_records(record_dir, test_name, calib=True):
    """``(homo_mat, ref_bbox)`` from ``<record_dir>/<test_name>/homo_mat.txt`` (3 x 3, ``np.loadtxt``; None without ``calib``) and
    ``ref_bbox.txt`` (one row of 4 values for one reference, or R rows; int [R][4]).  The reference opens a picker window when a
    file is missing; here that is an error naming the file."""
    homo = load_homo_mat(os.path.join(record_dir, test_name, 'homo_mat.txt')) if calib else None
    return homo, load_ref_bbox(os.path.join(record_dir, test_name, 'ref_bbox.txt'))


def load_homo_mat(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f'homography file {path} not found (the interactive point picker is not built: write the 3 x 3 matrix there)')
    m = np.loadtxt(path, dtype=np.float64)
    if m.shape != (3, 3):
        raise ValueError(f'{path}: expected a 3 x 3 matrix, got shape {m.shape}')
    return m


def load_ref_bbox(path):
    if not os.path.isfile(path):
        raise FileNotFoundError(f'reference box file {path} not found (the interactive ROI picker is not built: write one "x y w h" row per reference there)')
    return _boxes(np.loadtxt(path, dtype=np.float64))


def csv_bytes(names, levels, avg):
    """``waterlevel.csv`` as ``pd.DataFrame(levels, index=timestamps, columns=est_ref{i}_px).assign(est_avg_px=avg).to_csv()``
    writes it, without pandas: shortest-repr floats, an empty field for NaN, the index as ``YYYY-MM-DD HH:MM:SS`` (dates alone
    when every frame falls on midnight, as a DatetimeIndex prints).  A frame name that is no timestamp is written as it is
    (the reference raises)."""
    stamps = []
    for n in names:
        try:
            stamps.append(datetime.strptime(n, TIME_FORMAT))
        except (ValueError, TypeError):
            stamps.append(None)
    dates_only = bool(stamps) and all(s is not None and (s.hour, s.minute, s.second) == (0, 0, 0) for s in stamps)
    buf = io.StringIO()
    wr = csv.writer(buf, lineterminator='\n')
    R = levels.shape[1]
    wr.writerow([''] + [f'est_ref{i}_px' for i in range(R)] + ['est_avg_px'])
    for n, s, row, a in zip(names, stamps, levels, avg):
        idx = str(n) if s is None else (s.strftime('%Y-%m-%d') if dates_only else s.strftime('%Y-%m-%d %H:%M:%S'))
        wr.writerow([idx] + ['' if np.isnan(v) else repr(float(v)) for v in list(row) + [a]])
    return buf.getvalue().encode('utf-8')


def calibration_default(test_name):
    """The reference switches the homography on by test name (reference_tracking.py:117-140): off for ``houston`` and ``LSU``."""
    return not ('houston' in test_name or ('boston' not in test_name and 'LSU' in test_name))


def tracking_default(test_name):
    """The reference switches the box tracker on by test name (reference_tracking.py:117-140): off for ``houston`` and ``LSU``,
    on for ``boston`` and for every name it does not know."""
    return not ('houston' in test_name or ('boston' not in test_name and 'LSU' in test_name))


def resolve_records(test_name, ref_bbox_path=None, homo_mat_path=None, calib=None, record_dir='./records/groundtruth'):
    """``(homo_mat or None, ref_bbox)`` for a clip: explicit files win over ``<record_dir>/<test_name>/``; ``calib`` None = on when a
    homography file is given, else the reference's default by test name (``calibration_default``)."""
    if calib is None:
        calib = True if homo_mat_path else calibration_default(test_name)
    homo = load_homo_mat(homo_mat_path or os.path.join(record_dir, test_name, 'homo_mat.txt')) if calib else None
    return homo, load_ref_bbox(ref_bbox_path or os.path.join(record_dir, test_name, 'ref_bbox.txt'))


# ------------------------------------------------------------------------------------------------ the device side
class WaterLevelMeter:
    """One clip's water-level measurement.  ``ref_bbox``: (x, y, w, h) per reference (static; ``measure(bbox=...)`` overrides them
    for one frame); ``homo_mat``: the 3 x 3 source -> destination homography, or None for no calibration; ``frames_hint``: rows
    the device log starts with (it doubles when they run out).  All ``measure`` calls of a clip belong on one stream.
    ``track``: the boxes follow the frame (``ops.track_update``, search radius ``track_radius``): ``measure`` then needs the frame,
    and ``finish`` leaves ``box_log`` int [T][R][4], ``track_ok`` bool [T][R] and ``track_score`` float32 [T][R]."""

    def __init__(self, ref_bbox, homo_mat=None, frames_hint=256, device=None, water_label=WATER_LABEL, palette=color_palette,
                 alpha=0.4, track=False, track_radius=16):
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        if self.device.type != 'cuda':
            raise RuntimeError('WaterLevelMeter: the kernels run on the GPU; there is no CPU fallback')
        self.boxes = _boxes(ref_bbox)
        self.R = self.boxes.shape[0]
        self.inverse = ops.inverse_homography(homo_mat) if homo_mat is not None else None
        self.homo_mat = None if homo_mat is None else np.asarray(homo_mat, np.float64)
        self.water_label = int(water_label)
        self.palette, self.alpha = palette, alpha
        self.log = torch.full((max(1, int(frames_hint)), self.R), -1, dtype=torch.int32, device=self.device)
        self.track, self.track_radius, self.track_state = bool(track), int(track_radius), None
        if self.track:
            if not 1 <= self.track_radius <= ops.TRACK_MAX_RADIUS:
                raise ValueError(f'WaterLevelMeter: track_radius {track_radius} outside 1 .. {ops.TRACK_MAX_RADIUS}')
            self.track_logs = [torch.zeros((self.log.shape[0],) + tail, dtype=dt, device=self.device)
                               for tail, dt in (((self.R, 4), torch.int32), ((self.R,), torch.int32), ((self.R,), torch.float32))]
        self.names = []
        self.t = 0
        self._stream = None

    def measure(self, label_dev, frame_dev=None, name=None, bbox=None, stream=None, overlay=None):
        """Enqueue one frame: the warp(s) when calibrated, the tracker's step when tracking, the scan into the log and, with
        ``frame_dev`` (float32 [3,H,W] in [0,1]), the overlay with boxes and lines, which is returned (RGB uint8 [H,W,3] on the
        device; else None).  ``overlay=False``: the frame is for the tracker alone.  ``label_dev``: uint8 [H,W].  Runs on
        ``stream`` (default: the current one) and never synchronises."""
        if stream is not None:
            with torch.cuda.stream(stream):
                return self.measure(label_dev, frame_dev, name, bbox, overlay=overlay)
        if self.track and (frame_dev is None or bbox is not None):
            raise ValueError('WaterLevelMeter.measure: a tracking meter needs frame_dev and moves the boxes itself (no bbox=)')
        cur = torch.cuda.current_stream(self.device)
        if self._stream is None or cur != self._stream:
            self._stream = cur
            for log in [self.log] + (self.track_logs if self.track else []):
                log.record_stream(cur)
        boxes = self.boxes if bbox is None else _boxes(bbox)
        if boxes.shape[0] != self.R:
            raise ValueError(f'WaterLevelMeter.measure: {boxes.shape[0]} boxes for {self.R} references')
        kp = keypoints(boxes)
        H, W = label_dev.shape
        if not self.track and ((kp[:, 0] < 0) | (kp[:, 0] >= W) | (kp[:, 1] < 0) | (kp[:, 1] >= H)).any():      # before anything is enqueued or logged
            raise ValueError(f'WaterLevelMeter.measure: key point outside the {W} x {H} image: {kp.tolist()}')
        if self.t >= self.log.shape[0]:
            grown = torch.full((2 * self.log.shape[0], self.R), -1, dtype=torch.int32, device=self.device)
            grown[:self.t].copy_(self.log[:self.t])          # stream-ordered behind the scans that wrote those rows
            grown.record_stream(cur)
            self.log = grown
            if self.track:
                for k, old in enumerate(self.track_logs):
                    self.track_logs[k] = torch.zeros((2 * old.shape[0],) + tuple(old.shape[1:]), dtype=old.dtype, device=self.device)
                    self.track_logs[k][:self.t].copy_(old[:self.t])
                    self.track_logs[k].record_stream(cur)
        label = label_dev.contiguous()
        frame = frame_dev.contiguous() if frame_dev is not None else None
        if self.inverse is not None:
            label = ops.warp_perspective_u8(label, None, inverse=self.inverse)
            if frame is not None:
                frame = ops.warp_perspective_u8(frame, None, inverse=self.inverse)
        if self.track:                               # on the frame the estimator holds: the warped one when calibrated (:169, :184)
            luma = ops.track_luma(frame)
            if self.track_state is None:
                self.track_state = ops.track_init(luma, boxes, self.track_radius)
            ops.track_update(self.track_state, luma, *self.track_logs, self.t)
            dev_boxes = self.track_logs[0][self.t]   # the row the tracker just wrote
            ops.waterline_scan_dev(label, dev_boxes, self.log, self.t, self.water_label)
        else:
            ops.waterline_scan(label, kp, self.log, self.t, self.water_label)
        ov = None
        if frame is not None and (overlay is None or overlay):
            ov = ops.overlay_device(frame, label, self.palette, self.alpha)
            if self.track:
                ops.waterlevel_draw_dev(ov, dev_boxes, self.log, self.t)
            else:
                ops.waterlevel_draw(ov, boxes, self.log, self.t)
        self.names.append(str(self.t) if name is None else str(name))
        self.t += 1
        return ov

    def offsets(self):
        """The scan log so far, int32 [T][R] on the host (one D2H; waits for the stream the measurements ran on)."""
        if self.t == 0:
            return np.zeros((0, self.R), np.int32)
        with torch.cuda.stream(self._stream):
            return self.log[:self.t].cpu().numpy()

    def finish(self):
        """``(names, levels float64 [T][R], average float64 [T])``: one D2H of the log, then reference_tracking.py:190-217 on the host."""
        levels = levels_from_offsets(self.offsets())
        for r in range(self.R):
            levels[:, r] = smooth(levels[:, r])
        self.result = (list(self.names), levels, nanmean_rows(levels))
        if self.track:                               # the tracker's logs come back with the clip, so its warnings (:188) do too
            with torch.cuda.stream(self._stream) if self._stream is not None else torch.cuda.device(self.device):
                box, ok, score = (log[:self.t].cpu().numpy() for log in self.track_logs)
            self.box_log, self.track_ok, self.track_score = box, ok.astype(bool), score
            for t in np.flatnonzero(~self.track_ok.all(axis=1)):
                warnings.warn(f'Tracker failed at frame {self.names[t]}.')
        return self.result

    def write_csv(self, path):
        names, levels, avg = self.finish()
        with open(path, 'wb') as f:
            f.write(csv_bytes(names, levels, avg))
        return path


def measure_to_sink(meter, sink, label_dev, frame_dev, name, viz_path=None):
    """One frame of ``meter`` on the PNG sink's side stream (``png_device.PngSink``), behind whatever the current stream has
    enqueued; the annotated overlay goes to ``viz_path`` through the sink's encoder.  Returns the event after which
    ``label_dev`` / ``frame_dev`` are no longer read."""
    ready = torch.cuda.Event()
    ready.record()
    done = torch.cuda.Event()
    with torch.cuda.stream(sink.stream):
        sink.stream.wait_event(ready)
        wants_frame = bool(viz_path) or meter.track
        ov = meter.measure(label_dev, frame_dev if wants_frame else None, name, overlay=bool(viz_path))
        label_dev.record_stream(sink.stream)
        if frame_dev is not None and wants_frame:
            frame_dev.record_stream(sink.stream)
        done.record()
    if ov is not None:
        sink._submit(ov, None, viz_path, ready)
    return done
