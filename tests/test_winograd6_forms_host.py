"""vfn_winograd6_form (include/vfn_winograd6.h) under every setting of VFN_WINO6_XFORM.  The variable is read once per process, so
every setting is asked in a fresh child.  No device work: the query only looks at the shape."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (N, H, W, C): the F(6x6) transform shapes of the 480x854 plan (profiles/r11_tune_wino6_transforms.json) ...
PLAN_SHAPES = [(1, 30, 54, 640), (1, 30, 54, 1024), (1, 60, 108, 256), (1, 60, 108, 512), (1, 120, 216, 256), (2, 30, 54, 256),
               (2, 30, 54, 512), (2, 30, 54, 640), (2, 30, 54, 1024), (2, 60, 108, 128), (2, 60, 108, 256), (2, 60, 108, 512),
               (2, 120, 216, 64), (2, 120, 216, 256)]
# ... and those of tests/test_winograd6_forms_gpu.py, input (Cin) and output (Cout) side
TEST_SHAPES = [(1, 5, 7, 32), (2, 12, 20, 64), (1, 13, 19, 128), (1, 13, 19, 96), (2, 30, 54, 256), (1, 6, 6, 36), (1, 6, 6, 20),
               (2, 8, 14, 132), (2, 8, 14, 260), (1, 7, 7, 512), (1, 7, 7, 640)]
SHAPES = PLAN_SHAPES + TEST_SHAPES

_CHILD = r'''
import json, sys
sys.path.insert(0, sys.argv[1])
from vfloodnet_amd import _lib
L = _lib.lib()
shapes = json.loads(sys.argv[2])
print(json.dumps([[L.vfn_winograd6_form(*s, io, r) for io, r in ((0, 0), (1, 0), (1, 1))] for s in shapes]))
'''

_ASKED = {}


def ask(setting):
    """[[input, output, output with residual] per shape] in a child with VFN_WINO6_XFORM = setting (None: unset); asked once."""
    if setting not in _ASKED:
        env = dict(os.environ)
        env.pop('VFN_WINO6_XFORM', None)
        if setting is not None:
            env['VFN_WINO6_XFORM'] = setting
        r = subprocess.run([sys.executable, '-c', _CHILD, ROOT, json.dumps(SHAPES)], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        _ASKED[setting] = json.loads(r.stdout.strip().splitlines()[-1])
    return _ASKED[setting]


def test_zero_forces_form0_everywhere():
    assert all(f == [0, 0, 0] for f in ask('0'))


@pytest.mark.parametrize('setting', [None, 'auto', '1', '2'])
def test_the_wave_uniform_form_only_where_a_wave_lies_in_one_tile(setting):
    """A valid form for every shape; a form that reads the tile index of a wave's first lane (1) never for a C / 2 that is no multiple
    of 64 (it is not built at present: 1 is never returned)."""
    for (N, H, W, C), forms in zip(SHAPES, ask(setting)):
        assert all(f in (0, 1, 2) for f in forms), (setting, (N, H, W, C), forms)
        if (C // 2) % 64:
            assert 1 not in forms, (setting, (N, H, W, C), forms)


def test_forced_forms_apply_wherever_they_can():
    """2 applies to every shape; 1 (the form that was measured out) selects form 0."""
    for (N, H, W, C), f1, f2 in zip(SHAPES, ask('1'), ask('2')):
        assert f1 == [0, 0, 0] and f2 == [2, 2, 2], ((N, H, W, C), f1, f2)


def test_unset_and_auto_are_the_same_rule():
    assert ask(None) == ask('auto')


def test_a_refused_shape_has_no_form():
    from vfloodnet_amd import _lib
    L = _lib.lib()
    assert L.vfn_winograd6_form(1, 8, 8, 30, 0, 0) == -1 and L.vfn_winograd6_form(0, 8, 8, 32, 1, 0) == -1
