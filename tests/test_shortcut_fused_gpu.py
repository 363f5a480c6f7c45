"""A Bottleneck's shortcut convolution inside its conv3's launch (vfn_conv1x1_shortcut_fused_f32, include/vfn_shortcut_fused.h;
csrc/conv_winograd.hip: wino_gemm_dual_kernel): against the two layers launched one after the other WITHOUT any K split (bit for
bit), against float64, its refusals, and in the engine's plans.

Every output is a slice of a larger buffer with GUARD sentinel floats on either side and the sentinel inside before the launch; the
shortcut's input has a pixel stride wider than its channel count, the spare columns holding NaN.

"No K split" for the two-launch side: a tiled configuration whose waves all walk the whole K range (vfn_conv_cfg_wk <= 1: 1 is what
the library reports for the plain kernels, values above 1 are the waves-along-K kernels) with ksplit = 1, or the persistent 1x1
kernel, which has no split at all."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from golden_util import load, state_dict, t, close_logits

pytestmark = pytest.mark.gpu

SENT = -1.0e30
GUARD = 256
N = 2
# (shortcut stride, H, W of the shortcut's input): stride 1 at 5x7 -> M = 70, one full and one partial 64-row tile; stride 2 at odd
# sizes (7x9 -> 4x5: the last sampled row and column are the image's last) and at even ones (6x8 -> 3x4)
GEOMS = [(1, 5, 7), (2, 7, 9), (2, 6, 8)]
CHANNELS = list(itertools.product((32, 96), (32, 64), (48, 160)))          # (shortcut Cin, main Cin, Cout)
TILED_UNSPLIT = 3                      # 64 x 64 tiles, one workgroup per tile, every wave walks all of K


class _Out:
    def __init__(self, gpu, *shape):
        self.shape, self.n = shape, int(torch.tensor(shape).prod())
        self.buf = torch.full((self.n + 2 * GUARD,), SENT, device=gpu)
        self.t = self.buf[GUARD:GUARD + self.n].view(*shape)

    def cpu(self, what=''):
        b = self.buf.cpu()
        guard = torch.full((GUARD,), SENT)
        assert torch.equal(b[:GUARD], guard) and torch.equal(b[GUARD + self.n:], guard), ('guard overwritten', what)
        inside = b[GUARD:GUARD + self.n].view(*self.shape)
        assert not (inside == SENT).any(), ('sentinel left inside', what, int((inside == SENT).sum()))
        assert not (inside != inside).any(), ('NaN inside', what)
        return inside

    def untouched(self):
        return bool((self.buf == SENT).all())


_DATA = {}


def _data(stride, H, W, csc, cmain, cout):
    """Inputs of one layer pair and its float64 composition (before the last ReLU), computed once and shared, never modified."""
    key = (stride, H, W, csc, cmain, cout)
    if key not in _DATA:
        g = torch.Generator().manual_seed(9000 + len(_DATA))
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        x = torch.randn(N, H, W, csc, generator=g)
        t2 = torch.randn(N, Ho, Wo, cmain, generator=g)
        w_sc, w_m = torch.randn(cout, csc, generator=g) / csc ** 0.5, torch.randn(cout, cmain, generator=g) / cmain ** 0.5
        aff = lambda: (1 + 0.1 * torch.randn(cout, generator=g), 0.1 * torch.randn(cout, generator=g))
        (s_sc, b_sc), (s_m, b_m) = aff(), aff()
        xs = x[:, ::stride, ::stride].double().reshape(-1, csc)
        r = xs @ w_sc.double().t() * s_sc.double() + b_sc.double()
        ref = t2.double().reshape(-1, cmain) @ w_m.double().t() * s_m.double() + b_m.double() + r
        _DATA[key] = dict(x=x, t2=t2, w_sc=w_sc, w_m=w_m, s_sc=s_sc, b_sc=b_sc, s_m=s_m, b_m=b_m, ref=ref, Ho=Ho, Wo=Wo)
    return _DATA[key]


class _Pair:
    """The two descriptors on device copies of ``_data``; the shortcut's input with pixel stride csc + 8 (NaN in the spare columns)."""

    def __init__(self, gpu, stride, H, W, csc, cmain, cout):
        from vfloodnet_amd import ops
        d = _data(stride, H, W, csc, cmain, cout)
        self.d, self.gpu, self.cout, self.stride, self.H, self.W, self.csc = d, gpu, cout, stride, H, W, csc
        self.M = N * d['Ho'] * d['Wo']
        self.x = torch.full((N, H, W, csc + 8), float('nan'), device=gpu)
        self.x[..., :csc] = d['x'].to(gpu)
        self.t2 = d['t2'].to(gpu)
        self.w_sc, self.w_m = ops.pad_rows(d['w_sc'].to(gpu)), ops.pad_rows(d['w_m'].to(gpu))
        self.aff = [d[k].to(gpu) for k in ('s_sc', 'b_sc', 's_m', 'b_m')]

    def descs(self, out, relu_out, ds=None, res=None):
        """(shortcut, main): ``ds`` = where the shortcut layer writes when launched alone, ``res`` = the main layer's residual."""
        from vfloodnet_amd import ops
        sc = ops.make_conv_desc(self.x, self.w_sc, self.cout, 1, 1, self.stride, 0, ds, self.aff[0], self.aff[1], cin=self.csc,
                                in_ld=self.csc + 8, out_ld=self.cout, N=N, H=self.H, W=self.W)
        main = ops.make_conv_desc(self.t2, self.w_m, self.cout, 1, 1, 1, 0, out, self.aff[2], self.aff[3], res, False, relu_out)
        return sc, main

    def two_launches(self, relu_out, down_cfg=TILED_UNSPLIT):
        from vfloodnet_amd import ops
        assert down_cfg >= ops.PCONV_CFG0 or (ops.conv_cfg_kind(down_cfg) == 0 and ops.conv_cfg_wk(down_cfg) <= 1)
        ds, out = _Out(self.gpu, self.M, self.cout), _Out(self.gpu, self.M, self.cout)
        sc, main = self.descs(out.t, relu_out, ds.t, ds.t)
        assert sc.ksplit <= 1 and main.ksplit <= 1
        ops.conv2d_launch(sc, down_cfg, 0)
        ops.conv2d_launch(main, ops.pconv_cfg(3, 512), 0)
        torch.cuda.synchronize()
        ds.cpu('ds')
        return out.cpu('two launches')

    def fused(self, relu_out, tc, wgs):
        from vfloodnet_amd import ops
        out = _Out(self.gpu, self.M, self.cout)
        sc, main = self.descs(out.t, relu_out)
        assert ops.shortcut_fused_eligible(sc, main, 0) and (tc, 768) in ops.shortcut_fused_cfg_options(sc, main)
        ops.shortcut_fused_launch(sc, main, tc, wgs)
        torch.cuda.synchronize()
        return out.cpu(f'fused cfg {tc} wgs {wgs}')


def _tile_cfgs(cout):
    from vfloodnet_amd import ops
    return [tc for tc in range(4) if not (ops.WINO_GEMM_TILES[tc][1] > 64 and cout < 128)]


@pytest.mark.parametrize('geom', GEOMS)
def test_fused_equals_two_unsplit_launches_and_float64(gpu, geom):
    """Bit equality with `down` then `conv3 (res = ds)`, and the float64 composition at the tolerance tests/test_conv_gpu.py holds a
    1x1 layer to (2e-4 max(1, max|ref|)): every channel combination, ReLU on and off, every configuration of the fused form (the four
    tiles, operands one K tile ahead: the two-ahead instantiations went to scratch and are not built) eligible for the filter count.  Stride 1: the shortcut layer alone through the persistent kernel gives the same bits as through the tiled one."""
    from vfloodnet_amd import ops
    stride, H, W = geom
    n = 0
    for csc, cmain, cout in CHANNELS:
        pair = _Pair(gpu, stride, H, W, csc, cmain, cout)
        for relu_out in (False, True):
            two = pair.two_launches(relu_out)
            if stride == 1:
                assert torch.equal(pair.two_launches(relu_out, ops.pconv_cfg(3, 512)), two)
            ref = F.relu(pair.d['ref']) if relu_out else pair.d['ref']
            tol = 2e-4 * max(1.0, ref.abs().max().item())
            assert (two.double() - ref).abs().max().item() < tol
            worst = 0.0
            for tc in _tile_cfgs(cout):
                y = pair.fused(relu_out, tc, 512)
                worst = max(worst, (y.double() - ref).abs().max().item())
                assert torch.equal(y, two), (geom, csc, cmain, cout, relu_out, tc, (y - two).abs().max().item())
                n += 1
            print(f'{geom} Csc {csc} Cmain {cmain} Cout {cout} relu {relu_out}: max err vs float64 {worst:.3e} (tol {tol:.3e})')
            assert worst < tol, (worst, tol)
    assert n == 2 * (4 * 2 + 4 * 4)


@pytest.mark.parametrize('stride', [1, 2])
def test_unit_and_phase_seams(gpu, stride):
    """Many units per workgroup (M = 960 over 8 workgroups: the prefetch crosses phase seams and unit seams with the other source's
    resource in flight) and more workgroups than units (M = 70, 64-wide tiles of 48 filters: one or two units, eight workgroups), all
    tile shapes (one K tile ahead: the only depth the fused form has), against the two launches bit for bit."""
    many = _Pair(gpu, stride, 20 * stride, 24 * stride, 96, 64, 160)
    assert many.M == 960
    two = many.two_launches(True)
    for tc in range(4):
        assert torch.equal(many.fused(True, tc, 8), two), ('many units', tc)
    few = _Pair(gpu, stride, 5 * stride, 7 * stride, 96, 64, 48)
    assert few.M == 70
    two = few.two_launches(False)
    for tc in (2, 3):
        assert torch.equal(few.fused(False, tc, 256), two), ('more workgroups than units', tc)


def test_refusals_and_the_predicate(gpu):
    """Every condition the entry point does not run returns VFN_ERR_ARG, writes nothing, and ops.shortcut_fused_eligible says so too."""
    import ctypes as C
    from vfloodnet_amd import ops, _lib
    ERR = 1                            # VFN_ERR_ARG (csrc/common.h)
    pair = _Pair(gpu, 2, 7, 9, 32, 32, 48)
    out = _Out(gpu, pair.M, 48)
    some = torch.zeros(4096, device=gpu)

    def call(sc, main, tc=3):
        return _lib.lib().vfn_conv1x1_shortcut_fused_f32(C.byref(sc), C.byref(main), tc, 512, _lib.stream())

    def both(f):                       # the change applied to the shortcut alone, then to the main layer alone
        for which in (0, 1):
            pair_ = list(pair.descs(out.t, True))
            f(pair_[which])
            yield which, pair_

    def set_(**kw):
        def f(d):
            for k, v in kw.items():
                setattr(d, k, v)
        return f

    changes = {
        '3x3': set_(KH=3, KW=3), 'pad': set_(pad=1), 'Cin % 32': set_(Cin=16), 'in_ld % 4': set_(in_ld=42), 'in_ld < Cin': set_(in_ld=28),
        'mask': set_(mask=_lib.ptr(some)), 'in_lp': set_(in_lp=1), 'out_lp': set_(out_lp=_lib.ptr(some)), 'w_batch_rows': set_(w_batch_rows=64),
        'w_packed': set_(w_packed=1), 'ksplit': set_(ksplit=2), 'res': set_(res=_lib.ptr(some)), 'Cout': set_(Cout=44), 'M': set_(M=pair.M - 1),
        'offsets past the buffer-resource limit': set_(in_ld=1 << 29), 'cout_pad': set_(cout_pad=48),
    }
    n = 0
    for name, f in changes.items():
        for which, (sc, main) in both(f):
            assert call(sc, main) == ERR, (name, which)
            assert not ops.shortcut_fused_eligible(sc, main, 0), (name, which)
            n += 1
    for stride, which in ((3, 0), (4, 0), (2, 1)):
        sc, main = pair.descs(out.t, True)
        (sc, main)[which].stride = stride
        assert call(sc, main) == ERR and not ops.shortcut_fused_eligible(sc, main, 0), ('stride', stride, which)
    sc, main = pair.descs(out.t, True)
    assert call(sc, main, 4) == ERR and call(sc, main, 8) == ERR and call(sc, main, -1) == ERR
    assert call(sc, main, 1) == 0                          # (64 x 128 tiles on 48 filters: run -- cout_pad is 256 -- just never chosen)
    assert not ops.shortcut_fused_eligible(sc, main, 1) and not ops.shortcut_fused_eligible(sc, main, 2)      # an f32 kernel
    torch.cuda.synchronize()
    out.cpu('after the accepted call')
    out2 = _Out(gpu, pair.M, 48)
    for name, f in changes.items():
        for which, (sc, main) in both(f):
            main.out = _lib.ptr(out2.t)
            assert call(sc, main) == ERR
    torch.cuda.synchronize()
    assert n == 2 * len(changes) and out2.untouched()


def _model(gpu):
    from vfloodnet_amd import AFB_URR
    model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
    model.load_state_dict(state_dict(), strict=True)
    return model


def _lists(plan):
    return {'mem': plan.mem, 'pre1': plan.qsets[0].pre[1], 'pre2': plan.qsets[0].pre[2]}


def test_plan_fuses_each_down_block_and_meets_the_golden(gpu, monkeypatch):
    """The 96x160 sample of tests/test_golden_gpu.py::test_blocks with the switch on: that test's tolerances (keys / values 5e-4,
    close_logits at 1e-3); each of the three `down` blocks is ONE launch in the memory encoder's list and in the query lists, no
    `down` launch is left, and every list's FLOP sum equals the two-launch plan's."""
    from vfloodnet_amd import FeatureBank, engine as E, ops
    plans = {}
    for switch in ('0', '1'):
        monkeypatch.setattr(E, '_SHORTCUT_FUSED', switch)
        model = _model(gpu)
        g = load('blocks_96x160.npz')
        frames, m0 = t(g['frames']).to(gpu), t(g['mask'])
        oh = torch.stack([1 - m0, m0], 0).unsqueeze(0).to(gpu)
        k, v = model.memorize(frames[0:1], oh)
        assert (torch.stack([x.cpu() for x in k]) - t(g['key0'])).abs().max() < 5e-4
        assert (torch.stack([x.cpu() for x in v]) - t(g['val0'])).abs().max() < 5e-4
        fb = FeatureBank(2, 250000, gpu)
        fb.init_bank(k, v)
        score, _ = model.segment(frames[1:2], fb)
        ok, dl, dp = close_logits(score.cpu(), t(g['score']), 1e-3)
        print(f'VFN_SHORTCUT_FUSED={switch}: max |dlogit| {dl:.3e}, max |dsigmoid| {dp:.3e}')
        assert ok, (dl, dp)
        plans[switch] = model.engine().last_query[0]
    for name in _lists(plans['1']):
        on, off = _lists(plans['1'])[name], _lists(plans['0'])[name]
        fused = [l for l in on if l.fn is ops.shortcut_fused_launch]
        assert len(fused) == 3 and all('.down+conv3[' in l.name for l in fused), (name, [l.name for l in fused])
        assert not any('.0.conv3[' in l.name or '.down[' in l.name for l in on if l.fn is not ops.shortcut_fused_launch), name
        assert sum('.down[' in l.name for l in off) == 3 and not any(l.fn is ops.shortcut_fused_launch for l in off), name
        assert len(on) == len(off) - 3, (name, len(on), len(off))
        assert sum(l.flops for l in on) == sum(l.flops for l in off), name


def test_graph_replay_with_fused_shortcuts_is_bit_identical(gpu):
    """A three-frame clip at 96x160, switch on: the run that replays captured graphs equals the launch-by-launch run bit for bit
    (labels, logits of the last frame, bank sizes), graphs were captured, and the plan holds fused launches."""
    from tools import synth
    from vfloodnet_amd import engine as E, ops
    from vfloodnet_amd.video_seg import ClipRunner
    assert E._GRAPHS and E._SHORTCUT_FUSED != '0'
    frames, m0 = synth.clip(4, 3, 96, 160)
    frames = frames.to(gpu)
    onehot = synth.onehot(m0).unsqueeze(0).to(gpu)
    res = {}
    for mode in ('graphs', 'eager'):
        model = _model(gpu)
        model.engine().eager = (mode == 'eager')
        runner = ClipRunner(model, 2, 250000, size=96)
        runner.start(frames[0:1], onehot)
        labs = []
        for i in range(1, frames.shape[0]):
            lab = runner.step(frames[i:i + 1], next_frames=[frames[u:u + 1] for u in range(i + 1, min(frames.shape[0], i + 4))])
            labs.append(torch.from_numpy(lab.numpy().copy()))
        plan = model.engine().last_query[0]
        assert sum(l.fn is ops.shortcut_fused_launch for l in plan.mem) == 3
        res[mode] = (torch.stack(labs), plan.score.clone(), runner.bank_sizes(), sum(len(pl.graphs.graphs) for pl in model.engine().plans.values()))
    assert res['eager'][3] == 0 and res['graphs'][3] >= 1, (res['eager'][3], res['graphs'][3])
    assert torch.equal(res['graphs'][0], res['eager'][0])
    assert torch.equal(res['graphs'][1], res['eager'][1])
    assert res['graphs'][2] == res['eager'][2]
