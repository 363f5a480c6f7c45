"""The host side of the image model's validation (vfloodnet_amd/image_dataset.py, val_image_seg.py): the listing rules of
``WaterDataset_RGB``, the order in which ``draw_sample_params`` consumes its generator, ``select_best``, and the third header of
the C ABI.  No GPU."""
import os

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ listing rules
def _touch_pair(root, sub, stem, image=True, label=True):
    if image:
        Image.fromarray(np.zeros((4, 5, 3), np.uint8)).save(os.path.join(root, 'JPEGImages', sub, stem + '.jpg'))
    if label:
        Image.fromarray(np.zeros((4, 5), np.uint8), 'P').save(os.path.join(root, 'Annotations', sub, stem + '.png'))


def test_listing_rules(tmp_path):
    from vfloodnet_amd.image_dataset import WaterDataset_RGB
    root = str(tmp_path)
    for sub in ('zeta', 'alpha'):
        os.makedirs(os.path.join(root, 'JPEGImages', sub))
        os.makedirs(os.path.join(root, 'Annotations', sub))
    with open(os.path.join(root, 'train_imgs.txt'), 'w') as f:
        f.write('zeta\nalpha\n')                                    # file order, not alphabetical order
    for stem in ('10', '9', '100', '2'):
        _touch_pair(root, 'zeta', stem)
    _touch_pair(root, 'zeta', '7', label=False)                     # a photograph without a label is dropped
    _touch_pair(root, 'alpha', 'b')
    _touch_pair(root, 'alpha', 'aa')
    for mode in ('train_offline', 'val_offline'):
        ds = WaterDataset_RGB(mode, root, (32, 32))
        stems = [(os.path.basename(os.path.dirname(p)), os.path.basename(p)) for p in ds.img_list]
        assert stems == [('zeta', '2.jpg'), ('zeta', '9.jpg'), ('zeta', '10.jpg'), ('zeta', '100.jpg'), ('alpha', 'b.jpg'),
                         ('alpha', 'aa.jpg')]
        assert [os.path.basename(p)[:-4] for p in ds.label_list] == ['2', '9', '10', '100', 'b', 'aa']
        assert len(ds) == 6
    with pytest.raises(ValueError):
        WaterDataset_RGB('eval', root, (32, 32))
    with pytest.raises(ValueError):
        WaterDataset_RGB('val_offline', root, (32, 48))
    item = WaterDataset_RGB('val_offline', root, 32)[4]
    assert item['index'] == 4 and item['name'].endswith('b.jpg') and set(item) == {'img', 'label', 'name', 'index'}


# ------------------------------------------------------------------------------------------------ the drawer
class Script:
    """A generator that answers from a script and records every call with its arguments."""

    def __init__(self, answers):
        self.answers, self.calls = list(answers), []

    def _next(self, call):
        self.calls.append(call)
        assert self.answers, f'the drawer asked for more than the script holds: {call}'
        return self.answers.pop(0)

    def random(self):
        return self._next(('random',))

    def uniform(self, a, b):
        return self._next(('uniform', a, b))

    def randint(self, a, b):
        return self._next(('randint', a, b))


CROP_DRAW = [('uniform', 0.08, 1.0), ('uniform', 0.75, 1.33333333), ('random',)]


def test_drawer_every_operation_skipped():
    from vfloodnet_amd.image_dataset import draw_sample_params
    W, H = 100, 80
    # colour x 3, affine and flip refused (0.8 is not < 0.8; 0.5 is not < 0.5); the crop: area 0.5, ratio 1, no swap
    rng = Script([0.8, 0.9, 0.99, 0.8, 0.5, 0.5, 1.0, 0.5, 7, 11])
    p = draw_sample_params(rng, W, H)
    side = int(round((0.5 * W * H) ** 0.5))
    assert rng.calls == [('random',)] * 5 + CROP_DRAW + [('randint', 0, H - side), ('randint', 0, W - side)]
    assert not rng.answers
    assert p['brightness'] is None and p['contrast'] is None and p['hue'] is None and p['affine'] is None and p['flip'] is False
    assert p['crop'] == (7, 11, side, side)


def test_drawer_every_operation_taken_and_swapped_crop():
    import math
    from vfloodnet_amd.image_dataset import draw_sample_params
    from vfloodnet_amd.train_dataset import inverse_affine_matrix
    W, H = 100, 80
    # the crop is accepted at the first attempt, with the swap: area 0.25, ratio 1.25 -> w 50, h 40 -> swapped: w 40, h 50
    rng = Script([0.0, 0.7, 0.79, 1.5, 0.1, 0.3, 12.0, 0.15, -0.05, 1.1, -7.0, 0.49, 0.25, 1.25, 0.2, 3, 5])
    p = draw_sample_params(rng, W, H)
    w0 = int(round(math.sqrt(0.25 * W * H * 1.25)))
    h0 = int(round(math.sqrt(0.25 * W * H / 1.25)))
    assert (w0, h0) == (50, 40)
    assert rng.calls == [('random',), ('uniform', 0.1, 1.2), ('random',), ('uniform', 0.2, 1.8), ('random',), ('random',),
                         ('uniform', -20, 20), ('uniform', -0.2, 0.2), ('uniform', -0.2, 0.2), ('uniform', 0.7, 1.3),
                         ('uniform', -20, 20), ('random',)] + CROP_DRAW + [('randint', 0, H - w0), ('randint', 0, W - h0)]
    assert not rng.answers
    assert p['brightness'] == 0.7 and p['contrast'] == 1.5 and p['hue'] == 25 and p['flip'] is True
    assert p['affine'] == inverse_affine_matrix(W, H, 12.0, (0.15, -0.05), 1.1, -7.0)
    assert p['crop'] == (3, 5, w0, h0)                               # (i, j, h, w) with h = the old w


def test_drawer_ten_refusals_give_the_centred_square():
    from vfloodnet_amd.image_dataset import draw_sample_params
    W, H = 40, 400
    # every attempt: the whole area at ratio 1 -> a 126 x 126 box, wider than the image, swapped or not
    rng = Script([0.9, 0.9, 0.9, 0.9, 0.9] + [1.0, 1.0, 0.0, 1.0, 1.0, 0.9] * 5)
    p = draw_sample_params(rng, W, H)
    assert rng.calls == [('random',)] * 5 + CROP_DRAW * 10
    assert not rng.answers
    assert p['crop'] == (180, 0, 40, 40)


def test_sample_rng_depends_on_seed_epoch_index_only():
    from vfloodnet_amd.image_dataset import draw_sample_params, sample_rng
    a = draw_sample_params(sample_rng(3, 1, 4), 93, 67)
    assert a == draw_sample_params(sample_rng(3, 1, 4), 93, 67)
    others = [draw_sample_params(sample_rng(*k), 93, 67) for k in ((4, 1, 4), (3, 2, 4), (3, 1, 5))]
    assert all(o != a for o in others)
    i, j, h, w = a['crop']
    assert 0 <= i <= 67 - h and 0 <= j <= 93 - w and h >= 1 and w >= 1


# ------------------------------------------------------------------------------------------------ select_best
def test_select_best():
    from vfloodnet_amd.val_image_seg import select_best
    assert select_best([0.2, 0.5, 0.5, 0.3]) == 1                    # a tie keeps the earlier checkpoint
    assert select_best([0.0, 0.0]) is None                           # nothing exceeds the starting score 0
    assert select_best([]) is None
    assert select_best([0.1, 0.4, 0.9]) == 2
    assert select_best([0.9, 0.4]) == 0


# ------------------------------------------------------------------------------------------------ the header
def test_image_val_header_parses_and_is_exported():
    import ctypes as C
    from vfloodnet_amd import _lib
    with open(os.path.join(ROOT, 'include', 'vfn_image_val.h')) as f:
        defines, enums, structs, protos = _lib.parse_header(f.read())
    assert not structs and not enums                                 # entry points only
    assert sorted(protos) == ['vfn_imgval_affine_window', 'vfn_imgval_jitter', 'vfn_imgval_label_gather',
                              'vfn_imgval_resize_norm', 'vfn_seg_scores_f64']
    assert protos == _lib.SIGNATURES_IMAGE_VAL
    assert defines == {'VFN_SEG_SCORES_CHUNK': 2048, 'VFN_SEG_SCORES_MAX_BLOCKS': 1024}
    assert not set(protos) & set(_lib.SIGNATURES) and not set(protos) & set(_lib.SIGNATURES_WINOGRAD6)
    assert protos['vfn_seg_scores_f64'] == [C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_int, C.c_int, C.c_void_p]
    assert os.path.isfile(_lib.LIB_PATH), 'libvfn_hip.so is not built'
    L = C.CDLL(_lib.LIB_PATH)                                        # (loading needs no GPU)
    assert [s for s in protos if not hasattr(L, s)] == []
