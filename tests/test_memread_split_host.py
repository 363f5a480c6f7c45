"""The slice choice of the f32 stored-scores apply kernel (feature_bank.pick_apply_split): the full query tiles in ``nsplit`` bank
slices, a partial last tile in ``nsplit_tail`` longer ones.  Held to its own cost model (feature_bank.apply_split_cost: rounds over
256 CUs x the longest workgroup, in 32-column groups x chunks) against the rule before it, pick_nsplit with every tile alike."""
import os

import numpy as np
import pytest

from vfloodnet_amd import feature_bank as F
from vfloodnet_amd.feature_bank import MAX_SPLIT, QT_SCAN, pick_apply_split, pick_nsplit

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden', 'c2_480x854_100.npz')
SHAPES = [(1620, 2), (8160, 2), (1536, 2), (148, 1)]
BANKS = [1, 64, 100, 191, 192, 3000, 59500, 98584, 250000]


@pytest.fixture(autouse=True)
def _no_switches(monkeypatch):
    for name in ('VFN_APPLY_TAIL', 'VFN_APPLY_SPLIT', 'VFN_NSPLIT_SCAN'):
        monkeypatch.delenv(name, raising=False)


def _uniform(hw, obj_n, b):
    return pick_nsplit(hw, obj_n, b, QT_SCAN, MAX_SPLIT)


@pytest.mark.parametrize('hw,obj_n', SHAPES)
def test_slice_counts_in_range(hw, obj_n):
    for b in BANKS:
        s, t = pick_apply_split(hw, obj_n, b)
        assert 1 <= s <= MAX_SPLIT and 0 <= t <= s, (b, s, t)
        nchunks = max(1, (b + 63) // 64)
        if s > 1:
            assert nchunks // s >= 3, (b, s)                  # at least 3 chunks per slice
        if t > 1:
            assert nchunks // t >= 3, (b, t)


def test_no_partial_tile_is_the_uniform_rule():
    for b in BANKS:
        assert pick_apply_split(1536, 2, b) == (_uniform(1536, 2, b), 0)


def test_partial_tiles_take_the_tail_split():
    """live = 3 (C2, 1080p), 2 and 1: a tail slice count of its own, never more slices than the full tiles; a live count without a
    measured weight keeps the uniform rule."""
    for hw, obj_n in ((1620, 2), (8160, 2), (1600, 2), (1568, 2), (148, 1)):
        s, t = pick_apply_split(hw, obj_n, 59500)
        assert 1 <= t <= s, (hw, s, t)
    assert pick_apply_split(1620, 2, 59500) == (10, 8)                # one round of 2 * (12 * 10 + 8) = 256 workgroups


def test_live_count_without_a_weight_stays_uniform(monkeypatch):
    monkeypatch.setattr(F, 'APPLY_TAIL_WEIGHT', {3: F.APPLY_TAIL_WEIGHT[3]})
    for hw in (148, 168):
        for b in BANKS:
            assert pick_apply_split(hw, 1, b) == (_uniform(hw, 1, b), 0)
    assert pick_apply_split(1620, 2, 59500)[1] > 0


def test_modelled_cost_on_the_golden_clip():
    """C2, every bank size of the golden clip: never above the uniform rule's cost, and <= 0.96 of it in the sum (the least-cost
    pairs give 0.9456 with w(3) = 1; ties may cost up to 1 % more)."""
    sizes = np.load(GOLDEN)['bank_sizes'].max(axis=1)
    assert len(sizes) == 99
    new = old = 0.0
    for b in sizes.tolist():
        nchunks = (b + 63) // 64
        s, t = pick_apply_split(1620, 2, b)
        c_new = F.apply_split_cost(1620, 2, nchunks, s, t)
        c_old = F.apply_split_cost(1620, 2, nchunks, _uniform(1620, 2, b), 0)
        print(f'SPLITCOST B={b} chunks={nchunks} pair=({s},{t}) cost={c_new:.0f} uniform={c_old:.0f}')
        assert c_new <= c_old, (b, s, t)
        new, old = new + c_new, old + c_old
    print(f'SPLITCOST sum ratio {new / old:.4f}')
    assert new <= 0.96 * old


def test_cost_model_arithmetic():
    """The issue's figures: 910 chunks, (19, 0) = 2 rounds x 48 chunks x 4 groups; (10, 8) = one round of 256 workgroups."""
    assert F.apply_split_cost(1620, 2, 910, 19, 0) == 2 * 48 * 4
    assert F.apply_split_cost(1620, 2, 910, 10, 8) == max(91 * 4, 114 * 3 * F.APPLY_TAIL_WEIGHT[3])
    assert 2 * (12 * 10 + 8) == 256


def test_switch_restores_the_uniform_rule(monkeypatch):
    monkeypatch.setenv('VFN_APPLY_TAIL', '0')
    for hw, obj_n in SHAPES:
        for b in BANKS:
            assert pick_apply_split(hw, obj_n, b) == (_uniform(hw, obj_n, b), 0)
