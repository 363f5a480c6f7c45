"""The tracker's definition (tests/track_ref.py) follows known motion, and the host side of ``--track``: the reference's rule by
test name, the new flags, the ABI table.  No GPU."""
import os
import re

import numpy as np
import pytest

from track_ref import TrackerRef, luma_ref, make_clip, track_clip_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOX = (40, 30, 23, 17)


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_the_definition_recovers_every_shift(seed):
    """14 frames, 96 x 128, steps from -5 .. 5 at S = 5 under falling gain, rising offset and noise: every box is the first one
    displaced by the clip's known motion, and every correlation is high."""
    frames, disp = make_clip(seed, 14, 96, 128, [BOX], 5)
    assert np.abs(np.diff(disp, axis=0)).max() >= 4          # the clip does move
    box, ok, score, _ = track_clip_ref([luma_ref(f) for f in frames], [BOX], 5)
    assert ok.all() and score.min() > 0.9
    assert np.array_equal(box[:, 0, :2], np.array(BOX[:2]) + disp) and (box[:, 0, 2:] == BOX[2:]).all()


@pytest.mark.parametrize('seed,replaced', [(4, (9,)), (5, (3, 10)), (6, (6, 7))])
def test_replaced_frames_are_flagged_and_the_box_is_found_again(seed, replaced):
    frames, disp = make_clip(seed, 14, 96, 128, [BOX], 6, replaced=replaced)
    lumas = [luma_ref(f) for f in frames]
    tr = TrackerRef(lumas[0], [BOX], 6)
    last_good = None
    for t, L in enumerate(lumas):
        before = (tr.box.copy(), tr.T16[0].copy())
        box, ok, score = tr.update(L)
        if t in replaced:                                    # fails: nothing moves, nothing is learnt
            assert not ok[0] and score[0] < 0.5
            assert np.array_equal(box, before[0]) and np.array_equal(tr.T16[0], before[1])
            assert np.array_equal(box[0, :2], np.array(BOX[:2]) + disp[last_good])
        else:
            assert ok[0] and np.array_equal(box[0, :2], np.array(BOX[:2]) + disp[t]), t
            last_good = t


def test_a_flat_template_fails_without_moving():
    frames, _ = make_clip(7, 3, 64, 80, [BOX], 4)
    lumas = [luma_ref(f) for f in frames]
    lumas[0][BOX[1]:BOX[1] + BOX[3], BOX[0]:BOX[0] + BOX[2]] = 77        # vt == 0
    box, ok, score, tr = track_clip_ref(lumas, [BOX], 4)
    assert not ok.any() and (box[:, 0] == BOX).all() and (tr.T16[0] == 77 << 8).all()
    flat = [np.full((64, 80), 9, np.uint8)] * 2                          # every vp == 0: no candidate at all
    box, ok, score, _ = track_clip_ref(flat, [BOX], 4)
    assert not ok.any() and (box[:, 0] == BOX).all() and (score == 0).all()


def test_equal_keys_go_to_the_first_candidate_visited():
    """Stripes of period 4 along x, constant along y: every dy and every dx = 0 (mod 4) correlates perfectly; the first such
    candidate in the order dy ascending, then dx ascending wins."""
    L = np.tile(np.array([10, 80, 200, 120], np.uint8), (48, 16))
    tr = TrackerRef(L, [(20, 20, 9, 7)], 5)
    box, ok, _ = tr.update(L)
    assert ok[0] and box[0].tolist() == [16, 15, 9, 7]


def test_tracking_default_is_the_references_rule():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd.waterlevel import tracking_default
    assert [tracking_default(n) for n in ('houston_x', 'boston_y', 'LSU_z', 'anything')] == [False, True, False, True]


def test_the_parsers_take_the_new_flags_and_default_to_off():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import est_waterlevel, video_seg
    base = ['--test-name', 'boston_y', '--test-path', 'x']
    for parse in (est_waterlevel.get_parser, video_seg.get_args):
        a = parse(base)
        assert a.track == 'off' and a.track_radius == 16 and not est_waterlevel.use_tracking(a)
        a = parse(base + ['--track', 'on', '--track-radius', '8'])
        assert a.track == 'on' and a.track_radius == 8 and est_waterlevel.use_tracking(a)
        assert est_waterlevel.use_tracking(parse(base + ['--track', 'auto']))
        assert not est_waterlevel.use_tracking(parse(['--test-name', 'houston_x', '--test-path', 'x', '--track', 'auto']))
        with pytest.raises(SystemExit):
            parse(base + ['--track', 'csrt'])


def test_the_new_entry_points_are_declared_and_bound():
    import vfloodnet_amd  # noqa: F401
    from vfloodnet_amd import _lib, ops
    hdr = open(os.path.join(ROOT, 'include', 'vfn_hip.h')).read()
    for name in ('vfn_track_luma_f32', 'vfn_track_init', 'vfn_track_update', 'vfn_waterline_scan_dev', 'vfn_waterlevel_draw_dev'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', hdr) and name in _lib.ALL_SYMBOLS and name in _lib.SIGNATURES
    assert int(re.search(r'#define VFN_TRACK_MAX_SIDE (\d+)', hdr).group(1)) == ops.TRACK_MAX_SIDE == 512
    assert int(re.search(r'#define VFN_TRACK_MAX_RADIUS (\d+)', hdr).group(1)) == ops.TRACK_MAX_RADIUS == 32
    assert _lib.ABI_VERSION >= 17
