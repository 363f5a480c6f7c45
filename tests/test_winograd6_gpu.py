"""Winograd F(6x6, 3x3) of the f32 inference layers (csrc/conv_winograd.hip: vfn_winograd6_input_f32 -> vfn_winograd_gemm_f32 with 64
components -> vfn_winograd6_output_f32; filter banks from refresh kind 6) against float64, piece by piece and as a layer, and in the
engine against the reference's golden logits."""
import pytest
import torch
import torch.nn.functional as F

from golden_util import load, state_dict, t, close_logits

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout): smaller than one tile; H a multiple of 6, W not; both ragged and Cout no tile multiple; the res4 shape
CASES = [(1, 5, 7, 32, 32), (2, 12, 20, 64, 64), (1, 13, 19, 128, 96), (2, 30, 54, 256, 256)]

BT = torch.tensor([[1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0],
                   [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0], [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                   [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0], [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
                   [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0], [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
                   [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
                   [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 0], [0, 1, 1, 16, 16, 1 / 16, 1 / 16, 0],
                   [0, 1, -1, 32, -32, 1 / 32, -1 / 32, 1]], dtype=torch.float64)
G = torch.tensor([[1, 0, 0], [-2 / 9, -2 / 9, -2 / 9], [-2 / 9, 2 / 9, -2 / 9], [1 / 90, 1 / 45, 2 / 45], [1 / 90, -1 / 45, 2 / 45],
                  [32 / 45, 16 / 45, 8 / 45], [32 / 45, -16 / 45, 8 / 45], [0, 0, 1]], dtype=torch.float64)


def test_the_matrices_are_a_convolution():
    """(No device work.)  A^T [(G g G^T) (.) (B^T d B)] A is the 3x3 correlation of an 8x8 patch.  The constants of the bounds below:
    67.0625 is the largest absolute row sum of A^T; 12.5 is that of B^T's rows 0, 1, 2 and 7 (rows 5 and 6 sum to 15: the input
    transform's bound is the tighter figure)."""
    gen = torch.Generator().manual_seed(6)
    d, g = torch.randn(8, 8, generator=gen, dtype=torch.float64), torch.randn(3, 3, generator=gen, dtype=torch.float64)
    y = AT @ ((G @ g @ G.T) * (BT @ d @ BT.T)) @ AT.T
    assert (y - F.conv2d(d.view(1, 1, 8, 8), g.view(1, 1, 3, 3))[0, 0]).abs().max() < 1e-12
    assert BT.abs().sum(1).tolist() == [12.5, 12.5, 12.5, 7.5, 7.5, 15.0, 15.0, 12.5] and AT.abs().sum(1).max().item() == 67.0625


_DATA = {}


def _data(case):
    """Inputs and the float64 convolutions of one case, computed once and shared (never modified)."""
    if case not in _DATA:
        N, H, W, Cin, Cout = case
        g = torch.Generator().manual_seed(1000 + CASES.index(case))
        x = torch.randn(N, Cin, H, W, generator=g)
        w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
        scale = 1 + 0.1 * torch.randn(Cout, generator=g)
        shift = 0.1 * torch.randn(Cout, generator=g)
        res = torch.randn(N, Cout, H, W, generator=g)
        conv = {r: F.conv2d((F.relu(x) if r else x).double(), w.double(), padding=1) for r in (False, True)}
        _DATA[case] = dict(x=x, w=w, scale=scale, shift=shift, res=res, conv=conv)
    return _DATA[case]


def _rms(a):
    return float((a * a).mean().sqrt())


@pytest.mark.parametrize('case', CASES)
def test_winograd_f6x6_layer_matches_torch_cpu(gpu, case):
    """conv2d_winograd(tile=6) against float64 F.conv2d at the tolerance of test_winograd_f4x4_matches_torch_cpu, 2e-4 max(1, max|ref|):
    ReLU in and out, scale and shift, a residual with and without res_mod (one image's worth, repeated over the batch), and nothing at
    all.  C >= 128: F(6x6)'s r.m.s. error stays below 4x F(4x4)'s on the same layer (the float64-transform emulation gives 2x)."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout = case
    d = _data(case)
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().to(gpu)
    xd, resd, sc, sh = nhwc(d['x']), nhwc(d['res']), d['scale'].to(gpu), d['shift'].to(gpu)
    res1 = d['res'][0:1]                                   # res_mod = H W: the first image's residual for every image of the batch
    res1d = nhwc(res1).view(H * W, Cout)
    aff = lambda c: c * d['scale'].double().view(1, -1, 1, 1) + d['shift'].double().view(1, -1, 1, 1)
    variants = [
        ('all', dict(scale=sc, shift=sh, res=resd, relu_in=True, relu_out=True), F.relu(aff(d['conv'][True]) + d['res'].double())),
        ('plain', dict(), d['conv'][False]),
        ('res_mod', dict(scale=sc, shift=sh, res=res1d, res_mod=H * W, relu_out=True), F.relu(aff(d['conv'][False]) + res1.double())),
        ('relu_in+res', dict(res=resd, relu_in=True), d['conv'][True] + d['res'].double()),
    ]
    cfgs = [ops.wino_gemm_cfg(3, 512)] + ([ops.wino_gemm_cfg(5, 768)] if Cout >= 128 else [])       # 64 x 64 tiles; 64 x 128, two K tiles ahead
    for name, kw, ref in variants:
        tol = 2e-4 * max(1.0, ref.abs().max().item())
        for cfg in cfgs:
            y = ops.conv2d_winograd(xd, d['w'], cfg=cfg, tile=6, **kw)
            err = (y.permute(0, 3, 1, 2).cpu().double() - ref).abs().max().item()
            print(f'{case} {name} cfg {cfg}: max err {err:.3e} (tol {tol:.3e})')
            assert err < tol, (name, cfg, err, tol)
    if Cin >= 128:
        ref = d['conv'][False]
        y6 = ops.conv2d_winograd(xd, d['w'], cfg=cfgs[0], tile=6).permute(0, 3, 1, 2).cpu().double()
        y4 = ops.conv2d_winograd(xd, d['w'], cfg=cfgs[0], tile=4).permute(0, 3, 1, 2).cpu().double()
        top = ref.abs().max().item()
        e4, e6 = _rms(y4 - ref), _rms(y6 - ref)
        print(f'{case} rel. to the largest output: F4 rms {e4 / top:.2e} max {(y4 - ref).abs().max().item() / top:.2e} | '
              f'F6 rms {e6 / top:.2e} max {(y6 - ref).abs().max().item() / top:.2e} | ratio {e6 / e4:.2f}')
        assert e6 < 4 * e4, (e4, e6)


@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('relu', [False, True])
def test_input_transform_against_float64(gpu, case, relu):
    """V = B^T d B of the 8x8 patches at stride 6 (pad 1).  |V - V64| <= 16 * 2^-24 * 12.5^2 * max|d|: 12.5 the largest absolute row
    sum of B^T per pass, 16 additions per element.  Rows >= the tile count are zeros whatever the buffer held; the image sits in a
    NaN-filled allocation (pixel stride > C, rows of NaN before and after), so a tap outside the image that was read instead of
    taken as zero would surface as a NaN -- and the result equals the compact tensor's bit for bit."""
    from vfloodnet_amd import ops
    N, H, W, C, _ = case
    x = _data(case)['x']
    th, tw = (H + 5) // 6, (W + 5) // 6
    tiles, rows = N * th * tw, ops.winograd6_rows(N, H, W)
    assert tiles == ops.winograd6_tiles(N, H, W) and rows % 64 == 0 and rows >= tiles
    xin = (F.relu(x) if relu else x).double()
    xp = F.pad(xin, (1, 6 * tw + 1 - W, 1, 6 * th + 1 - H))
    patches = xp.unfold(2, 8, 6).unfold(3, 8, 6)                                   # [N, C, th, tw, 8, 8]
    V64 = torch.einsum('ia,nctuab,jb->ijntuc', BT, patches, BT).reshape(64, tiles, C)
    xd = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    V = torch.full((64, rows, C), float('nan'), device=gpu)
    ops.winograd_input(xd, V, rows, relu, tile=6)
    bound = 16 * 2.0 ** -24 * 12.5 ** 2 * xin.abs().max().item()
    err = (V[:, :tiles].cpu().double() - V64).abs().max().item()
    print(f'{case} relu={relu}: max |V - V64| {err:.3e} (bound {bound:.3e})')
    assert err <= bound, (err, bound)
    assert bool((V[:, tiles:] == 0).all())
    ld = C + 8
    big = torch.full((N * H * W + 2 * W + 32, ld), float('nan'), device=gpu)
    inner = big[W + 16:W + 16 + N * H * W]
    inner[:, :C] = xd.view(-1, C)
    V2 = torch.full((64, rows, C), float('nan'), device=gpu)
    ops.winograd_input(inner, V2, rows, relu, N, H, W, C, ld, tile=6)
    assert torch.equal(V2, V)


@pytest.mark.parametrize('case', CASES)
def test_output_transform_against_float64(gpu, case):
    """Y = A^T M A per tile (no epilogue), |Y - Y64| <= 16 * 2^-24 * 67.0625^2 * max|M|.  The output has a pixel stride wider than Cout
    and spare rows behind it, all holding a guard value: pixels past the image edge and columns past Cout are not written (a pixel past
    the right edge would land on the next row's first pixels and spoil their values)."""
    from vfloodnet_amd import ops
    N, H, W, _, Cout = case
    th, tw = (H + 5) // 6, (W + 5) // 6
    tiles, rows = N * th * tw, ops.winograd6_rows(N, H, W)
    g = torch.Generator().manual_seed(77 + CASES.index(case))
    M = torch.randn(64, rows, Cout, generator=g)
    Y64 = torch.einsum('ia,abntuc,jb->ntiujc', AT, M[:, :tiles].double().view(8, 8, N, th, tw, Cout), AT)
    Y64 = Y64.reshape(N, 6 * th, 6 * tw, Cout)[:, :H, :W]
    GUARD = -12345.0
    ld = Cout + 4
    buf = torch.full((N * H * W + 7 * W + 64, ld), GUARD, device=gpu)
    ops.winograd_output(M.to(gpu), rows, buf, N, H, W, Cout, None, None, None, 0, 0, False, out_ld=ld, tile=6)
    got = buf[:N * H * W, :Cout].view(N, H, W, Cout).cpu().double()
    bound = 16 * 2.0 ** -24 * 67.0625 ** 2 * M.abs().max().item()
    err = (got - Y64).abs().max().item()
    print(f'{case}: max |Y - Y64| {err:.3e} (bound {bound:.3e})')
    assert err <= bound, (err, bound)
    assert bool((buf[:, Cout:] == GUARD).all()) and bool((buf[N * H * W:] == GUARD).all())


def test_refreshed_filter_banks_equal_the_host_image(gpu):
    """The 64 banks the refresher writes (refresh kind 6, csrc/refresh.hip) after the parameter changed in place are bit-equal to
    ops.pack_winograd6_weight of the new values (float64, same order of operations on both sides); a layer over a slice of the
    input channels too."""
    from vfloodnet_amd import engine as E, ops
    from vfloodnet_amd.refresh import Refresher
    torch.manual_seed(66)
    conv = torch.nn.Conv2d(96, 80, 3, padding=1).to(gpu)
    reg = Refresher(gpu)
    whole = E.ConvLayer(conv, None, gpu, reg=reg)
    part = E.ConvLayer(conv, None, gpu, cin_range=(32, 96), reg=reg)
    U, Up = whole.w_wino6(), part.w_wino6()
    assert tuple(U.shape) == (64 * 256, 96) and tuple(Up.shape) == (64 * 256, 64)
    assert torch.equal(U, ops.pack_winograd6_weight(conv.weight).to(gpu))
    with torch.no_grad():
        conv.weight.mul_(1.7).add_(0.01 * torch.randn_like(conv.weight))
    assert not torch.equal(U, ops.pack_winograd6_weight(conv.weight).to(gpu))
    reg.run()
    assert torch.equal(U, ops.pack_winograd6_weight(conv.weight).to(gpu))
    assert torch.equal(Up, ops.pack_winograd6_weight(conv.weight[:, 32:96]).to(gpu))


def _n_f6(plan):
    from vfloodnet_amd import ops
    return sum(1 for lst in plan.all_lists() for l in lst if l.fn is ops.winograd_input and l.args[-1] == 6)


@pytest.mark.parametrize('f6', ['0', '2'])
def test_engine_logits_meet_the_golden_with_and_without_f6(gpu, f6, monkeypatch):
    """The 96x160 sample of tests/test_golden_gpu.py::test_blocks with every eligible 3x3 layer as Winograd (VFN_WINOGRAD=2), as
    F(4x4) everywhere (VFN_WINOGRAD_F6=0) and as F(6x6) everywhere (=2): the logits meet that test's tolerance (close_logits at 1e-3)
    and its key / value tolerance (5e-4) both ways."""
    from vfloodnet_amd import AFB_URR, FeatureBank, engine as E
    monkeypatch.setattr(E, '_WINOGRAD', '2')
    monkeypatch.setattr(E, '_WINOGRAD_F6', f6)
    model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
    model.load_state_dict(state_dict(), strict=True)
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
    print(f'VFN_WINOGRAD_F6={f6}: max |dlogit| {dl:.3e}, max |dsigmoid| {dp:.3e}')
    assert ok, (dl, dp)
    n6 = _n_f6(model.engine().last_query[0])
    assert (n6 == 0) if f6 == '0' else (n6 >= 30), n6


def test_graph_replay_of_the_f6_lists_is_bit_identical(gpu, monkeypatch):
    """A short clip at the network's own size with F(6x6) on every eligible layer: the run that replays captured graphs equals the
    launch-by-launch run bit for bit (labels, logits of the last frame, bank sizes), and graphs were captured."""
    from tools import synth
    from vfloodnet_amd import AFB_URR, engine as E
    from vfloodnet_amd.video_seg import ClipRunner
    assert E._GRAPHS
    monkeypatch.setattr(E, '_WINOGRAD', '2')
    monkeypatch.setattr(E, '_WINOGRAD_F6', '2')
    frames, m0 = synth.clip(4, 8, 96, 160)
    frames = frames.to(gpu)
    onehot = synth.onehot(m0).unsqueeze(0).to(gpu)
    out = {}
    for mode in ('graphs', 'eager'):
        model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
        model.load_state_dict(state_dict(), strict=True)
        model.engine().eager = (mode == 'eager')
        runner = ClipRunner(model, 2, 250000, size=96)
        runner.start(frames[0:1], onehot)
        labs = []
        for i in range(1, frames.shape[0]):
            lab = runner.step(frames[i:i + 1], next_frames=[frames[u:u + 1] for u in range(i + 1, min(frames.shape[0], i + 4))])
            labs.append(torch.from_numpy(lab.numpy().copy()))
        plan = model.engine().last_query[0]
        assert (plan.H0, plan.W0) == (96, 160) and _n_f6(plan) >= 30
        out[mode] = (torch.stack(labs), plan.score.clone(), runner.bank_sizes(), sum(len(pl.graphs.graphs) for pl in model.engine().plans.values()))
    assert out['eager'][3] == 0 and out['graphs'][3] >= 1, (out['eager'][3], out['graphs'][3])
    assert torch.equal(out['graphs'][0], out['eager'][0])
    assert torch.equal(out['graphs'][1], out['eager'][1])
    assert out['graphs'][2] == out['eager'][2]
