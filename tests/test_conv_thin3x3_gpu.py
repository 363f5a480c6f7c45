"""The LDS-resident 3x3 kernel of the 32-filter layers (csrc/conv_thin3x3.hip, vfn_conv3x3_thin_f32; 8 x 16 pixel blocks, persistent
grid) against float64 F.conv2d on the CPU at the tolerance every convolution configuration is held to, against the tiled kernel
without split-K, and at the edge of its domain."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

COUT = 32
# (N, H, W, workgroups): every pixel an edge pixel, one partial block; one full and one partial block in y and in x (8 + 1 rows, 16 + 16 + 1
# columns; 8 + 5 rows, 16 + 5 columns, two images); 24 blocks on 4 workgroups (six rounds of the persistent walk and the patch prefetch,
# plain striding) and on 8 (three rounds, one block run per XCD)
CASES = [(2, 5, 7, 0), (1, 9, 33, 0), (2, 13, 21, 0), (1, 48, 64, 4), (1, 48, 64, 8)]
CINS = [32, 64]

_DATA = {}


def _data(shape, cin):
    """Inputs and the float64 convolutions of one (N, H, W) and Cin, computed once and shared (never modified)."""
    key = shape + (cin,)
    if key not in _DATA:
        N, H, W = shape
        g = torch.Generator().manual_seed(3300 + 7 * len(_DATA))
        x = torch.randn(N, cin, H, W, generator=g)
        w = torch.randn(COUT, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        scale = 1 + 0.1 * torch.randn(COUT, generator=g)
        shift = 0.1 * torch.randn(COUT, generator=g)
        res = torch.randn(N, COUT, H, W, generator=g)
        conv = {r: F.conv2d((F.relu(x) if r else x).double(), w.double(), padding=1) for r in (False, True)}
        _DATA[key] = dict(x=x, w=w, scale=scale, shift=shift, res=res, conv=conv)
    return _DATA[key]


def _packed(w, gpu):
    from vfloodnet_amd import ops
    return ops.pad_rows(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous().to(gpu))


def _variants(d, gpu, N, H, W):
    """(name, descriptor arguments, float64 reference): nothing at all; ReLU in and out with scale, shift and a full residual; a residual
    of one image shared by the batch (res_mod = H W); ReLU on the input alone with a residual."""
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().to(gpu)
    resd, sc, sh = nhwc(d['res']), d['scale'].to(gpu), d['shift'].to(gpu)
    res1 = d['res'][0:1]
    res1d = nhwc(res1).view(H * W, COUT)
    aff = lambda c: c * d['scale'].double().view(1, -1, 1, 1) + d['shift'].double().view(1, -1, 1, 1)
    return [
        ('plain', dict(), d['conv'][False]),
        ('all', dict(scale=sc, shift=sh, res=resd, relu_in=True, relu_out=True), F.relu(aff(d['conv'][True]) + d['res'].double())),
        ('res_mod', dict(scale=sc, shift=sh, res=res1d, res_mod=H * W, relu_out=True), F.relu(aff(d['conv'][False]) + res1.double())),
        ('relu_in+res', dict(res=resd, relu_in=True), d['conv'][True] + d['res'].double()),
    ]


def _launch(xd, wp, cin, out, cfg, N, H, W, scale=None, shift=None, res=None, relu_in=False, relu_out=False, res_mod=0, in_ld=None, out_ld=None):
    from vfloodnet_amd import ops
    d = ops.make_conv_desc(xd, wp, COUT, 3, 3, 1, 1, out, scale, shift, res, relu_in, relu_out, cin=cin, in_ld=in_ld, out_ld=out_ld,
                           res_ld=COUT if res is not None else None, N=N, H=H, W=W)
    d.res_mod = int(res_mod)
    ops.conv2d_launch(d, cfg, 0)
    return out


@pytest.mark.parametrize('cin', CINS)
@pytest.mark.parametrize('case', CASES)
def test_thin3x3_matches_torch_cpu_and_the_tiled_kernel(gpu, case, cin):
    """Against float64 F.conv2d: 2e-4 max(1, max|ref|), the tolerance of tests/test_winograd6_gpu.py.  Against the tiled kernel
    (128 x 32 tiles, configuration 6, no split-K): bit-equal -- the kernel walks the taps, the 8-channel blocks and the channel pairs
    (c, c + 4) of every MFMA in the tiled kernel's order and its epilogue is the same expression, so equality is asserted in place of the
    2e-5 max(1, max|ref|) that two different summation orders would be held to."""
    from vfloodnet_amd import ops
    N, H, W, wgs = case
    d = _data((N, H, W), cin)
    xd = d['x'].permute(0, 2, 3, 1).contiguous().to(gpu)
    wp = _packed(d['w'], gpu)
    cfg = ops.thin3x3_cfg(cin, wgs)
    assert ops.is_thin3x3_cfg(cfg) and ops.thin3x3_cfg_info(cfg) == (cin, wgs) and ops.conv_cfg_name(cfg) == f'conv_thin3x3_kernel<{cin}>'
    for name, kw, ref in _variants(d, gpu, N, H, W):
        top = max(1.0, ref.abs().max().item())
        y = _launch(xd, wp, cin, torch.full((N, H, W, COUT), float('nan'), device=gpu), cfg, N, H, W, **kw)
        yt = _launch(xd, wp, cin, torch.full((N, H, W, COUT), float('nan'), device=gpu), 6, N, H, W, **kw)
        err = (y.permute(0, 3, 1, 2).cpu().double() - ref).abs().max().item()
        print(f'{case} cin {cin} {name}: max err {err:.3e} (tol {2e-4 * top:.3e}); max |thin - tiled| {(y - yt).abs().max().item():.3e}')
        assert err < 2e-4 * top, (name, err)
        assert torch.equal(y, yt), name


@pytest.mark.parametrize('cin', CINS)
def test_thin3x3_honours_the_leading_dimensions(gpu, cin):
    """in_ld > Cin and out_ld > 32: the input sits in a NaN-filled allocation (NaN columns past Cin, NaN rows before and after), so a tap
    outside the image that was read instead of taken as zero, or a column past the layer's channels, would surface as a NaN; the output
    columns past 32 and the rows around the output keep their guard value, and the result equals the compact tensors' bit for bit."""
    from vfloodnet_amd import ops
    N, H, W = 2, 13, 21
    d = _data((N, H, W), cin)
    xd = d['x'].permute(0, 2, 3, 1).contiguous().to(gpu)
    wp = _packed(d['w'], gpu)
    cfg = ops.thin3x3_cfg(cin, 0)
    kw = dict(scale=d['scale'].to(gpu), shift=d['shift'].to(gpu), res=d['res'].permute(0, 2, 3, 1).contiguous().to(gpu), relu_in=True, relu_out=True)
    y = _launch(xd, wp, cin, torch.empty(N, H, W, COUT, device=gpu), cfg, N, H, W, **kw)
    M, in_ld, out_ld, GUARD = N * H * W, cin + 8, COUT + 4, -12345.0
    big = torch.full((M + 2 * W + 32, in_ld), float('nan'), device=gpu)
    inner = big[W + 16:W + 16 + M]
    inner[:, :cin] = xd.view(-1, cin)
    buf = torch.full((M + 2 * W + 32, out_ld), GUARD, device=gpu)
    out = buf[W + 16:W + 16 + M]
    _launch(inner, wp, cin, out, cfg, N, H, W, in_ld=in_ld, out_ld=out_ld, **kw)
    assert torch.equal(out[:, :COUT], y.view(-1, COUT))
    assert bool((buf[:, COUT:] == GUARD).all()) and bool((buf[:W + 16] == GUARD).all()) and bool((buf[W + 16 + M:] == GUARD).all())
    # the same without any ReLU: a ReLU that dropped a NaN would hide exactly the read the NaN gutters are there to show
    kw.update(relu_in=False, relu_out=False)
    y = _launch(xd, wp, cin, torch.empty(N, H, W, COUT, device=gpu), cfg, N, H, W, **kw)
    assert bool(torch.isfinite(y).all())
    buf.fill_(GUARD)
    _launch(inner, wp, cin, out, cfg, N, H, W, in_ld=in_ld, out_ld=out_ld, **kw)
    assert torch.equal(out[:, :COUT], y.view(-1, COUT))
    assert bool((buf[:, COUT:] == GUARD).all()) and bool((buf[:W + 16] == GUARD).all()) and bool((buf[W + 16 + M:] == GUARD).all())


def test_thin3x3_refuses_what_is_outside_its_domain(gpu):
    """Cout != 32, stride 2, 1x1 and Cin = 48: VFN_ERR_ARG and nothing written; ops.thin3x3_eligible agrees with the entry point (and
    with it on a layer inside the domain)."""
    from vfloodnet_amd import _lib, ops
    L = _lib.lib()
    GUARD = -7.0

    def status(cin, cout, k, stride):
        N, H, W = 1, 9, 17
        x = torch.randn(N, H, W, cin, device=gpu)
        wp = ops.pad_rows(torch.randn(cout, k * k * cin, device=gpu))
        Ho = (H + 2 * (k // 2) - k) // stride + 1
        Wo = (W + 2 * (k // 2) - k) // stride + 1
        out = torch.full((N, Ho, Wo, cout), GUARD, device=gpu)
        d = ops.make_conv_desc(x, wp, cout, k, k, stride, k // 2, out)
        st = L.vfn_conv3x3_thin_f32(C.byref(d), 0, _lib.stream())
        torch.cuda.synchronize()
        assert ops.thin3x3_eligible(d, 0) == (st == 0)
        return st, bool((out == GUARD).all())

    for args in ((64, 48, 3, 1), (64, 32, 3, 2), (64, 32, 1, 1), (48, 32, 3, 1)):
        st, untouched = status(*args)
        assert st == 1 and untouched, args
    st, untouched = status(64, 32, 3, 1)
    assert st == 0 and not untouched
