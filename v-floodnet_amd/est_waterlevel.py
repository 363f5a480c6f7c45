"""Drop-in for the reference's ``est_waterlevel.py`` with ``--opt ref`` (``estimation/reference_tracking.est_by_reference``).

Same arguments and directory layout: frames from ``--test-path``, masks from ``./output/segs/<name>/mask``, records from
``./records/groundtruth/<name>/``, results in ``<out-dir>/<name>_ref/`` (``waterlevel.csv`` and ``viz/``).  The warps, the
column scan and the annotated overlay run on the GPU (``waterlevel.WaterLevelMeter``); the viz PNGs are compressed there too
(``png_device.PngSink``).  ``video_seg.main --waterlevel`` produces the same files in the pass that writes the masks.

The ``people`` / ``stopsign`` estimators (Detectron2, MeshTransformer) are out of scope and raise ``NotImplementedError``;
so does any other ``--opt``, as in the reference.
"""
import argparse
import os
from glob import glob

import numpy as np
import torch

from . import ops, waterlevel
from .data import AsyncWriter, load_image_in_PIL
from .png_device import PngSink


def get_parser(argv=None):
    """est_waterlevel.py:10-21 plus the record overrides."""
    parser = argparse.ArgumentParser(description='Estimate Water Level (MI355X-native, reference object)')
    parser.add_argument('--test-name', type=str, required=True, help='Name of the test video')
    parser.add_argument('--test-path', type=str, required=True, help='Input image directory.')
    parser.add_argument('--out-dir', default='output/waterlevel', help='A file or directory to save output results.')
    parser.add_argument('--opt', type=str, help='Estimation options. Only "ref" is built.')
    parser.add_argument('--gpu', type=int, default=0, help='GPU card id.')
    parser.add_argument('--ref-bbox', type=str, default=None, help='Reference boxes, one "x y w h" row each (default: records/groundtruth/<name>/ref_bbox.txt).')
    parser.add_argument('--homo-mat', type=str, default=None, help='3 x 3 homography file (default: records/groundtruth/<name>/homo_mat.txt).')
    parser.add_argument('--no-calib', action='store_true', help='No perspective calibration, whatever the test name.')
    parser.add_argument('--no-viz', dest='viz', action='store_false', default=True, help='Skip the annotated overlays under viz/.')
    parser.add_argument('--track', choices=['off', 'on', 'auto'], default='off',
                        help='Follow the reference boxes through the clip (a translation-only correlation tracker, not CSRT). '
                             'auto: the reference\'s rule by test name (off for houston and LSU).')
    parser.add_argument('--track-radius', type=int, default=16, help='Search radius of the tracker in pixels per frame (1 .. 32).')
    return parser.parse_args(argv)


def use_calibration(args):
    """Calibration on or off: ``--no-calib`` and ``--homo-mat`` decide; otherwise the reference's rule by test name."""
    if getattr(args, 'no_calib', False):
        return False
    if getattr(args, 'homo_mat', None):
        return True
    return waterlevel.calibration_default(args.test_name)


def use_tracking(args):
    """``--track``: on, off, or the reference's rule by test name."""
    mode = getattr(args, 'track', 'off') or 'off'
    return waterlevel.tracking_default(args.test_name) if mode == 'auto' else mode == 'on'


def est_by_reference(img_list, water_mask_list, out_dir, record_dir, test_name, device=None, ref_bbox_path=None,
                     homo_mat_path=None, calib=None, viz=True, track=False, track_radius=16):
    """reference_tracking.py:116-218 without the pickers and the plot, with the project's own tracker in CSRT's place when
    ``track`` is set (the frames are then loaded without ``viz`` too); returns the ``WaterLevelMeter``."""
    if len(img_list) != len(water_mask_list):
        raise ValueError(f'{len(img_list)} frames but {len(water_mask_list)} masks')
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    homo, boxes = waterlevel.resolve_records(test_name, ref_bbox_path, homo_mat_path, calib, record_dir)
    os.makedirs(out_dir, exist_ok=True)
    viz_dir = os.path.join(out_dir, 'viz')
    if viz:
        os.makedirs(viz_dir, exist_ok=True)
    meter = waterlevel.WaterLevelMeter(boxes, homo, frames_hint=len(img_list), device=device, track=track, track_radius=track_radius)
    writer = AsyncWriter(4)
    with torch.cuda.device(device):
        sink = PngSink(device, writer)
        for img_path, mask_path in zip(img_list, water_mask_list):
            name = os.path.basename(img_path)[:-4]
            label = torch.from_numpy(np.array(load_image_in_PIL(mask_path, 'P'), np.uint8)).to(device)
            frame = None
            if viz or track:
                rgb = torch.from_numpy(np.array(load_image_in_PIL(img_path, 'RGB'), np.uint8)).to(device)
                if tuple(rgb.shape[:2]) != tuple(label.shape):
                    raise ValueError(f'{img_path} is {tuple(rgb.shape[:2])}, its mask {mask_path} {tuple(label.shape)}')
                frame = ops.to_tensor_device(rgb)
            waterlevel.measure_to_sink(meter, sink, label, frame, name, os.path.join(viz_dir, f'{name}.png') if viz else None)
        writer.close()
        meter.write_csv(os.path.join(out_dir, 'waterlevel.csv'))
    return meter


def main(args, device=None):
    """est_waterlevel.py:24-39."""
    if args.opt != 'ref':
        raise NotImplementedError(args.opt)
    water_mask_dir = os.path.join('./output/segs/', args.test_name, 'mask')
    img_list = sorted(glob(os.path.join(args.test_path, '*.jpg')) + glob(os.path.join(args.test_path, '*.png')))
    water_mask_list = sorted(glob(os.path.join(water_mask_dir, '*.png')))
    out_dir = os.path.join(args.out_dir, f'{args.test_name}_{args.opt}')
    if device is None:
        if not torch.cuda.is_available():
            raise ValueError('a GPU is required: the estimator has no CPU path')
        device = torch.device('cuda', getattr(args, 'gpu', 0))
    return est_by_reference(img_list, water_mask_list, out_dir, './records/groundtruth', args.test_name, device,
                            getattr(args, 'ref_bbox', None), getattr(args, 'homo_mat', None), use_calibration(args),
                            getattr(args, 'viz', True), use_tracking(args), getattr(args, 'track_radius', 16))


if __name__ == '__main__':
    _args = get_parser()
    print(_args)
    main(_args)
