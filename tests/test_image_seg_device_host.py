"""The device image-segmentation pipeline's rules, checked where no GPU is needed: the NumPy restatements of its two resizes
(tests/imgseg_ref.py, which the kernels are held to byte for byte in tests/test_image_seg_device_gpu.py) against the installed
Pillow and torch, the host-built coefficient tables against the restatement, the overlay source, and the host-side plumbing
(keyword, command line)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

import imgseg_ref as R

GOLD = R.GOLD


@pytest.mark.parametrize('src,dst', R.RESIZE_CASES)
def test_resize_restatement_equals_pillow(src, dst):
    a = R.photo(src[0] * 1000 + src[1], *src)
    want = np.array(Image.fromarray(a).resize((dst[1], dst[0]), Image.BILINEAR))
    assert np.array_equal(R.np_resize_bilinear(a, *dst), want)


@pytest.mark.parametrize('n_in,n_out', [(131, 64), (24, 64), (1, 64), (1080, 416), (95, 32)])
def test_host_tables_are_the_restatements(n_in, n_out):
    """``train_dataset.resize_tables(..., 'bilinear')`` (vectorised; what the product uploads) = the C loops restated."""
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd.train_dataset import resize_tables
    bounds, kk = resize_tables(n_in, n_out, 'bilinear')
    rb, rk, ksize = R.bilinear_coeffs(n_in, n_out)
    assert kk.shape == (n_out, ksize) and np.array_equal(bounds, np.array(rb)) and np.array_equal(kk, np.array(rk))
    assert bounds[:, 0].min() >= 0 and (bounds[:, 0] + bounds[:, 1]).max() <= n_in and bounds[:, 1].max() <= ksize


def test_norm_equals_norm_imagenet_and_the_golden():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    g = np.load(GOLD)
    a = g['small_frame_u8']
    got = R.np_norm(R.np_resize_bilinear(a, 416, 416))
    want = image_seg.norm_imagenet(Image.fromarray(a), (416, 416)).numpy()
    assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got[:, ::16, ::16], g['small_norm'])
    b = R.photo(3, 95, 131)
    assert np.array_equal(R.np_norm(R.np_resize_bilinear(b, 32, 64)).view(np.uint32),
                          image_seg.norm_imagenet(Image.fromarray(b), (32, 64)).numpy().view(np.uint32))


def _upsample_case(p, H, W, cap):
    want = torch.nn.functional.interpolate(torch.from_numpy(p)[None, None], size=[H, W], mode='bilinear', align_corners=False)
    want = want.squeeze().round().numpy().astype(np.uint8)
    got = R.np_upsample_round(p, H, W)
    band = R.in_band(p, H, W)
    diff = got != want
    print(f'{p.shape} -> {(H, W)}: {int(diff.sum())} labels differ from torch, {int(band.sum())} of {band.size} pixels in the band')
    assert not (diff & ~band).any()
    if cap:
        assert band.sum() <= 0.0005 * band.size
    assert set(np.unique(got)) <= {0, 1}


@pytest.mark.parametrize('name', ['c1', 'small'])
def test_upsample_restatement_agrees_with_torch_on_the_standin(name):
    p, H, W = R.standin_prob(name)
    _upsample_case(p, H, W, cap=True)


@pytest.mark.parametrize('hw,HW', [((32, 32), (37, 61)), ((64, 96), (120, 214)), ((48, 40), (30, 33))])
def test_upsample_restatement_agrees_with_torch_on_smooth_maps(hw, HW):
    _upsample_case(R.smooth_map(hw[0], *hw), *HW, cap=False)


def test_upsample_rounds_halves_to_even():
    p = np.full((4, 4), 0.5, np.float32)
    assert not R.np_upsample_round(p, 9, 7).any()                     # rint(0.5) = 0
    assert np.array_equal(R.np_upsample_round(np.full((4, 4), 1.5, np.float32), 5, 5), np.full((5, 5), 2, np.uint8))


def test_overlay_source_roundtrip():
    """``vfn_overlay_u8`` takes the frame as f32 and truncates x * 255: for a decoded byte u, trunc((u / 255.0f) * 255.0f) == u
    for all 256 values, so the decoded f32 frame overlays the photograph's own bytes (no uint8-source kernel needed)."""
    u = np.arange(256, dtype=np.uint8)
    f = (u.astype(np.float32) / np.float32(255.0)) * np.float32(255.0)
    assert f.dtype == np.float32 and np.array_equal(f.astype(np.uint8), u) and np.array_equal(np.trunc(f), u.astype(np.float32))


def test_device_pipeline_needs_a_gpu_device(tmp_path):
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    from tools.standin import StandIn
    with pytest.raises(RuntimeError):
        image_seg.test_waterseg('unused.pth', str(tmp_path), 'x', str(tmp_path / 'out'), torch.device('cpu'), model=StandIn(),
                                pipeline='device')
    with pytest.raises(ValueError):
        image_seg.test_waterseg('unused.pth', str(tmp_path), 'x', str(tmp_path / 'out'), torch.device('cpu'), model=StandIn(),
                                pipeline='fast')
    with pytest.raises(RuntimeError):
        image_seg.ImageSegRunner(StandIn(), torch.device('cpu'))
    assert not (tmp_path / 'out').exists()                             # refused before anything is created


def test_command_line_flags():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import image_seg
    a = image_seg.get_args(['--test-path', 'p', '--test-name', 'n'])
    assert (a.model_path, a.out_path, a.batch, a.viz, a.gpu, a.pipeline) == \
        ('./records/link_efficientb4_model.pth', os.path.join('./', 'output', 'segs'), 1, True, 0, 'device')
    a = image_seg.get_args(['--model-path', 'm.pth', '--test-path', 'p', '--test-name', 'n', '--out-path', 'o', '--batch', '4',
                            '--no-viz', '--gpu', '1'])
    assert (a.model_path, a.out_path, a.batch, a.viz, a.gpu) == ('m.pth', 'o', 4, False, 1)
