"""The certified bank match (f32 FeatureBank.update: bf16x3 scores, certification by the derived error bound, exact f32 rescoring of
the winner, an f32 scan of the columns left open) against the full f32 scan it replaces (VFN_CERTIFIED_MATCH=0): match_idx /
match_corr and the bank after the update must be IDENTICAL bit for bit -- on random banks, on adversarial near-ties (duplicated
rows, rows one ulp apart, one direction at several magnitudes, an all-equal bank, ties across bank slices, zero-norm entries and
columns) and over the full C2 clip."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


class _Switch:
    """VFN_CERTIFIED_MATCH set for a block (read by FeatureBank.update at every call)."""
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.old = os.environ.get('VFN_CERTIFIED_MATCH')
        os.environ['VFN_CERTIFIED_MATCH'] = '1' if self.on else '0'

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop('VFN_CERTIFIED_MATCH', None)
        else:
            os.environ['VFN_CERTIFIED_MATCH'] = self.old


def _make_bank(gpu, keys, values, hw, budget=250000):
    from vfloodnet_amd.feature_bank import FeatureBank
    o = len(keys)
    fb = FeatureBank(o, budget, gpu, precision='fp32')
    fb._alloc(hw, max(k.shape[0] for k in keys))
    for i in range(o):
        n = keys[i].shape[0]
        fb._kbuf[i, :n].copy_(keys[i])
        fb._vbuf[i, :n].copy_(values[i])
        fb._ibuf[i, :n, 0] = 0.0
        fb._ibuf[i, :n, 1] = 1.0
    fb._set_lengths([int(k.shape[0]) for k in keys])
    return fb


def _update_both(gpu, keys, values, new, frame_idx=3, updates=1):
    """Run ``updates`` updates on two identical banks, certified and f32; return both banks' match outputs and contents."""
    o, hw = new.shape[-3], new.shape[-2]
    out = {}
    for on in (True, False):
        fb = _make_bank(gpu, keys, values, hw)
        with _Switch(on):
            for u in range(updates):
                kv = new[u] if new.dim() == 4 else new
                fb.update([kv[i, :, :128].t() for i in range(o)], [kv[i, :, 128:].t() for i in range(o)], frame_idx + u)
        torch.cuda.synchronize()
        n = fb._sync_len()
        out[on] = dict(idx=fb._midx.clone(), corr=fb._mcorr.clone(), n=list(n),
                       k=[fb._kbuf[i, :n[i]].clone() for i in range(o)], v=[fb._vbuf[i, :n[i]].clone() for i in range(o)],
                       info=[fb._ibuf[i, :n[i]].clone() for i in range(o)], stats=fb.match_stats() if on else None)
    return out


def _assert_identical(out):
    a, b = out[True], out[False]
    assert torch.equal(a['idx'], b['idx'])
    assert torch.equal(a['corr'].view(torch.int32), b['corr'].view(torch.int32))
    assert a['n'] == b['n']
    for x, y in zip(a['k'] + a['v'] + a['info'], b['k'] + b['v'] + b['info']):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def _random_case(gpu, lens, hw, seed):
    g = torch.Generator(device=gpu).manual_seed(seed)
    keys = [torch.randn(n, 128, device=gpu, generator=g) * (1 + i) for i, n in enumerate(lens)]
    values = [torch.randn(n, 512, device=gpu, generator=g) for n in lens]
    new = torch.randn(len(lens), hw, 640, device=gpu, generator=g)
    for i, n in enumerate(lens):                   # a third of the new keys are noisy copies of bank entries: merges happen
        src = torch.randint(0, n, (hw // 3,), device=gpu, generator=g)
        new[i, :hw // 3, :128] = keys[i][src] * 0.7 + 0.05 * torch.randn(hw // 3, 128, device=gpu, generator=g)
    return keys, values, new


@pytest.mark.parametrize('hw', [1620, 157])
@pytest.mark.parametrize('lens', [[60], [65, 1000], [5000, 4937, 129], [25037, 113000]])
def test_random_banks_bit_identical(gpu, lens, hw):
    out = _update_both(gpu, *_random_case(gpu, lens, hw, sum(lens) + hw))
    _assert_identical(out)
    st = out[True]['stats']
    print(f'lens {lens} hw {hw}: uncertain {st["uncertain"]} of {st["columns"]} per object')


def test_two_updates_keep_the_key_image(gpu):
    """The key image is re-split incrementally after merge / append: the second update still matches the f32 path."""
    keys, values, new0 = _random_case(gpu, [3000, 2500], 1620, 11)
    _, _, new1 = _random_case(gpu, [3000, 2500], 1620, 12)
    new1[:, :500, :128] = new0[:, :500, :128] * 1.3          # merged entries of update 1 are the best matches of update 2
    _assert_identical(_update_both(gpu, keys, values, torch.stack([new0, new1]), updates=2))


def _adversarial(gpu, kind, B=4000, hw=1620):
    g = torch.Generator(device=gpu).manual_seed(7)
    base = torch.randn(B, 128, device=gpu, generator=g)
    new = torch.randn(1, hw, 640, device=gpu, generator=g)
    if kind == 'duplicates':                       # every new key's best entry exists twice (adjacent and far apart)
        base[1::2] = base[0::2][:B // 2]
        base[B - 200:] = base[:200]
        new[0, :, :128] = base[torch.arange(hw, device=gpu) % B] * 2.0
    elif kind == 'ulp':                            # pairs of entries one ulp apart in every channel
        base[1::2] = torch.nextafter(base[0::2], torch.full_like(base[0::2], float('inf')))[:B // 2]
        new[0, :, :128] = base[(torch.arange(hw, device=gpu) * 7) % B]
    elif kind == 'magnitudes':                     # one direction at several magnitudes: equal cosines, different rounding
        d = torch.randn(128, device=gpu, generator=g)
        for j, c in enumerate([1.0, 0.5, 3.0, 1e-3, 7.25, 1e3, 2.0, 0.1]):
            base[j * 500] = d * c
        new[0, :hw // 2, :128] = d * torch.linspace(0.2, 5.0, hw // 2, device=gpu)[:, None]
    elif kind == 'all_equal':
        base[:] = base[0]
        new[0, :hw // 2, :128] = base[0] * 1.5
    elif kind == 'straddle':                       # the same entry at both ends of the bank: ties across bank slices
        for j in range(64):
            base[B - 1 - 31 * j] = base[31 * j]
        new[0, :, :128] = base[(torch.arange(hw, device=gpu) % 64) * 31] + 1e-6
    elif kind == 'zero_rows':                      # a zero-norm entry makes every column uncertain; so does a zero column
        base[17] = 0.0
        new[0, 5, :128] = 0.0
    return [base], [torch.randn(B, 512, device=gpu, generator=g)], new


@pytest.mark.parametrize('kind', ['duplicates', 'ulp', 'magnitudes', 'all_equal', 'straddle', 'zero_rows'])
def test_adversarial_ties_bit_identical(gpu, kind):
    out = _update_both(gpu, *_adversarial(gpu, kind))
    _assert_identical(out)
    st = out[True]['stats']
    print(f'{kind}: uncertain {st["uncertain"]} of {st["columns"]}')
    if kind in ('all_equal', 'zero_rows'):
        assert st['uncertain'] == [st['columns']]          # nothing can be certified: every column took the f32 path


def test_c2_full_clip_identical(gpu):
    """The 99-frame C2 clip (480x854, f32, golden weights), certified vs f32 match in one process: labels and bank sizes identical
    at every frame, and the final banks bit for bit."""
    from golden_util import GOLDEN, state_dict
    from tools import synth
    from vfloodnet_amd import AFB_URR
    from vfloodnet_amd.video_seg import run_clip
    path = os.path.join(GOLDEN, 'c2_480x854_100.npz')
    g = np.load(path)
    H, W = [int(x) for x in g['shape']]
    T = int(np.unpackbits(g['labels'], axis=-1).shape[0])
    model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
    model.load_state_dict(state_dict(), strict=True)
    frames, m0 = synth.clip(int(g['seed']), T, H, W)
    frames = frames.to(gpu)
    out = {}
    for on in (True, False):
        with _Switch(on):
            out[on] = run_clip(model, frames, m0)
    a, b = out[True], out[False]
    assert a['bank_sizes'] == b['bank_sizes']
    assert torch.equal(a['labels'], b['labels'])
    fa, fb_ = a['fb'], b['fb']
    for x, y in zip(fa.keys + fa.values + fa.info, fb_.keys + fb_.values + fb_.info):
        assert torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))
    st = fa.match_stats()
    rate = sum(st['uncertain']) / max(1, st['columns'] * fa.obj_n)
    print(f'C2 clip: {st["updates"]} certified updates, uncertain columns {st["uncertain"]} of {st["columns"]} per object '
          f'({100 * rate:.2f} %)')
