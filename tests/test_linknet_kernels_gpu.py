"""The bootstrap model's kernels one by one (``csrc/linknet_ops.hip``, ``vfn_dilate2_f32``, the transposed convolution through the
implicit GEMM) against plain torch on the CPU in float64, at the smallest shapes that reach each edge: images smaller than the
filter window, odd sizes before a stride-2 stage, leading dimensions wider than the channel count, more squeeze-excite channels
than one wavefront, M = 1.  ``tests/test_linknet.py`` compares the whole model end to end, where one kernel's fault at one edge
is diluted by the 230 launches around it.

Every output buffer holds NaN before the launch ("never written" and "written where it should not be" both show); input columns
a kernel has no business reading hold NaN as well.

Bounds of the activation kernels (stem, depthwise, gate, head) come from the reference alone: the same formula evaluated in
float32 on the CPU lies ``e32 / max(1, |ref|max)`` from the float64 result; a kernel may be 8 x the largest such ratio over its
case list away (another summation order, FMA chains of up to 27 / 25 / 2688 terms, the hardware's fast exponential), times the
case's ``max(1, |ref|max)``.  The element-wise kernels (column scale, add, dilate) are one rounding or none: bit equality.  The
transposed convolution keeps the implicit-GEMM kernel's bound of tests/test_conv_gpu.py, ``2e-4 * max(1, |ref|max)``."""
import functools
import itertools
import re
import zlib

import pytest
import torch
import torch.nn.functional as F

NAN = float('nan')
FACTOR = 8.0
VFN_ERR_ARG = 1                        # include/vfn_hip.h


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _swish(x):
    return x * torch.sigmoid(x)


def conv_pad_crop(x, w, s, pb, Ho, Wo, groups=1):
    """x [N,C,H,W] under ``pb`` zeros before the image and as many after it as an ``Ho x Wo`` output needs, convolved with stride
    ``s``, cropped to ``Ho x Wo``: what the stem and depthwise kernels are handed (pad_before, Ho, Wo)."""
    k = w.shape[-1]
    H, W = x.shape[-2:]
    pa_h = max((Ho - 1) * s + k - pb - H, 0)
    pa_w = max((Wo - 1) * s + k - pb - W, 0)
    return F.conv2d(F.pad(x, (pb, pa_w, pb, pa_h)), w, stride=s, groups=groups)[..., :Ho, :Wo]


def transposed_ref(x, conv_t, bn, dt):
    """ConvTranspose2d(4, 2, 1) with bias -> eval-mode BatchNorm -> ReLU in ``dt``; x [N,mid,h,w]."""
    y = F.conv_transpose2d(x.to(dt), conv_t.weight.detach().to(dt), conv_t.bias.detach().to(dt), stride=2, padding=1)
    y = F.batch_norm(y, bn.running_mean.to(dt), bn.running_var.to(dt), bn.weight.detach().to(dt), bn.bias.detach().to(dt), False, 0.0, bn.eps)
    return F.relu(y)


def _transposed_layer(mid):
    g = _gen('convT', mid)
    conv_t = torch.nn.ConvTranspose2d(mid, mid, 4, stride=2, padding=1)
    bn = torch.nn.BatchNorm2d(mid, eps=1e-5).eval()
    with torch.no_grad():
        conv_t.weight.copy_(1.6 * torch.randn(mid, mid, 4, 4, generator=g) / (4 * mid) ** 0.5)      # (4 of the 16 taps meet an output pixel)
        conv_t.bias.copy_(0.3 * torch.randn(mid, generator=g))
        bn.weight.copy_(1 + 0.1 * torch.randn(mid, generator=g))
        bn.bias.copy_(0.1 * torch.randn(mid, generator=g))
        bn.running_mean.copy_(0.2 * torch.randn(mid, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(mid, generator=g))
    return conv_t, bn


def _same_pad_before(k, s):
    from vfloodnet_amd.linknet import _same_pad_before as f
    return f(k, s)


def _ratio(ref32, ref64):
    return (ref32.double() - ref64).abs().max().item() / max(1.0, ref64.abs().max().item())


def _err(got, ref64):
    """The kernel's distance from the float64 reference in units of max(1, |ref|max); NaN anywhere -> inf."""
    d = (got.double() - ref64).abs().max().item()
    return float('inf') if d != d else d / max(1.0, ref64.abs().max().item())


def _report(name, what, ratio, errs):
    """errs: (error, case) of every launch.  Prints the figures, then holds the worst launch to the bound."""
    worst, case = max(errs, key=lambda e: e[0])
    print(f'{name} {what}: float32 ratio {ratio:.3e}  bound {FACTOR * ratio:.3e}  kernel error {worst:.3e}  ({len(errs)} launches)')
    assert worst <= FACTOR * ratio, (name, case, f'error {worst:.3e}', f'bound {FACTOR * ratio:.3e}', f'{worst / (FACTOR * ratio):.1f} x the bound')


# ------------------------------------------------------------------------------------------------------------------ stem
STEM_SIZES = [(3, 3), (4, 6), (5, 7), (32, 64)]
STEM_CASES = [(N, hw, ld, pb) for N in (1, 2) for hw in STEM_SIZES for ld in (48, 64) for pb in (0, 1)]


def _stem_inputs(case):
    N, (H, W), ld, pb = case
    g = _gen('stem', case)
    x = torch.randn(N, 3, H, W, generator=g)
    w = 1.6 * torch.randn(48, 3, 3, 3, generator=g) / 27 ** 0.5
    sc, sh = torch.zeros(64), torch.zeros(64)                     # (as the product packs them: zeros in the padding)
    sc[:48] = 1 + 0.1 * torch.randn(48, generator=g)
    sh[:48] = 0.1 * torch.randn(48, generator=g)
    return x, w, sc, sh


def _stem_ref(case, inputs, dt):
    N, (H, W), ld, pb = case
    x, w, sc, sh = (t.to(dt) for t in inputs)
    y = conv_pad_crop(x, w, 2, pb, (H + 1) // 2, (W + 1) // 2)
    return _swish(y * sc[:48].view(1, -1, 1, 1) + sh[:48].view(1, -1, 1, 1))


# ------------------------------------------------------------------------------------------------------------- depthwise
DW_SIZES = [(1, 1), (2, 3), (7, 9), (13, 13), (8, 12)]
DW_CHANNELS = [(4, 4, 4), (36, 40, 64), (160, 160, 160)]
DW_KINDS = [(k, s, sw) for k in (3, 5) for s in (1, 2) for sw in (0, 1)]


def _dw_pads(k, s):
    return sorted({_same_pad_before(k, s), 0})


def _dw_cases(kinds=DW_KINDS):
    return [(k, s, sw, pb, hw, N, ch) for (k, s, sw) in kinds for pb in _dw_pads(k, s) for hw in DW_SIZES for N in (1, 2) for ch in DW_CHANNELS]


def _dw_legal(case):
    k, s, sw, pb, (H, W), N, ch = case
    return H // s >= 1 and W // s >= 1          # (1, 1) under stride 2 has no output pixel: the launcher must refuse it


def _dw_inputs(case):
    k, s, sw, pb, (H, W), N, (C, ld_x, ld_o) = case
    g = _gen('dw', case)
    x = torch.full((N, H, W, ld_x), NAN)                          # columns C.. are not the kernel's to read
    x[..., :C] = 1.5 * torch.randn(N, H, W, C, generator=g)
    w = 1.6 * torch.randn(C, 1, k, k, generator=g) / k
    sc = 1 + 0.1 * torch.randn(C, generator=g)
    sh = 0.1 * torch.randn(C, generator=g)
    return x, w, sc, sh


def _dw_ref(case, inputs, dt):
    k, s, sw, pb, (H, W), N, (C, ld_x, ld_o) = case
    x, w, sc, sh = (t.to(dt) for t in inputs)
    xin = x[..., :C].permute(0, 3, 1, 2)
    if sw:
        xin = _swish(xin)
    y = conv_pad_crop(xin, w, s, pb, H // s, W // s, groups=C)
    return _swish(y * sc.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1))


# ------------------------------------------------------------------------------------------------------------------ gate
GATE_SHAPES = [(4, 1, 32), (48, 12, 64), (65, 17, 96), (144, 6, 160), (100, 256, 128), (1632, 68, 1632), (2688, 112, 2688)]
GATE_CASES = [(shp, M) for shp in GATE_SHAPES for M in (1, 6, 300)]


def _gate_inputs(case):
    (C, sq, Cpad), M = case
    g = _gen('gate', case)
    x = 0.5 * torch.randn(M, Cpad, generator=g) + torch.randn(1, Cpad, generator=g)       # per-channel means of order 1
    w1 = torch.randn(sq, C, generator=g) / C ** 0.5
    b1 = 0.2 * torch.randn(sq, generator=g)
    w2 = torch.randn(C, sq, generator=g) / sq ** 0.5
    b2 = 0.2 * torch.randn(C, generator=g)
    return x, w1, b1, w2, b2


def _gate_ref(case, inputs, dt):
    (C, sq, Cpad), M = case
    x, w1, b1, w2, b2 = (t.to(dt) for t in inputs)
    mean = x[:, :C].mean(0).view(1, C, 1, 1)
    s = _swish(F.conv2d(mean, w1.view(sq, C, 1, 1), b1))
    return torch.sigmoid(F.conv2d(s, w2.view(C, sq, 1, 1), b2)).view(C)


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_SHAPES = [(4, 4), (32, 32), (32, 60)]
HEAD_CASES = [(shp, prob, M) for shp in HEAD_SHAPES for prob in (0, 1) for M in (1, 257, 2048)]
HEAD_BIAS = 0.3


def _head_inputs(case):
    (C, ld), prob, M = case
    g = _gen('head', case)
    x = torch.full((M, ld), NAN)
    x[:, :C] = torch.randn(M, C, generator=g)
    w = 1.6 * torch.randn(C, generator=g) / C ** 0.5
    return x, w


def _head_ref(case, inputs, dt):
    (C, ld), prob, M = case
    x, w = (t.to(dt) for t in inputs)
    z = F.conv2d(x[:, :C].reshape(M, C, 1, 1), w.view(1, C, 1, 1), torch.tensor([HEAD_BIAS], dtype=dt)).view(M)
    return torch.sigmoid(z) if prob else z


_KERNELS = {'stem': (lambda: STEM_CASES, _stem_inputs, _stem_ref), 'dwconv': (lambda: [c for c in _dw_cases() if _dw_legal(c)], _dw_inputs, _dw_ref),
            'gate': (lambda: GATE_CASES, _gate_inputs, _gate_ref), 'head': (lambda: HEAD_CASES, _head_inputs, _head_ref)}


@functools.lru_cache(maxsize=None)
def _table(kernel):
    """case -> float64 reference, and the largest float32-on-the-CPU ratio over the kernel's whole case list: computed once,
    shared by that kernel's tests, never changed."""
    cases, make, ref = _KERNELS[kernel]
    refs, worst = {}, 0.0
    with torch.no_grad():
        for case in cases():
            inputs = make(case)
            r64 = ref(case, inputs, torch.float64)
            worst = max(worst, _ratio(ref(case, inputs, torch.float32), r64))
            refs[case] = r64
    assert 0 < worst < 1e-5, worst                               # (float32 arithmetic on values of order 1)
    return refs, worst


# ------------------------------------------------------------------------------------------------- reference self-check (CPU)
def test_reference_helpers_on_the_cpu():
    """The tests' own references, in float64 and without a GPU: pad-then-convolve-then-crop equals the oracle's static "same"
    padding wherever that is defined (even and odd sizes down to 1 x 1, all four (k, s) pairs, depthwise groups) and yields the
    ``H // s`` outputs the product asks for; the transposed-convolution reference equals F.conv2d of the zero-inserted input
    under the PRODUCT-packed filters, scale and shift."""
    from oracle import linknet_ref as R
    from vfloodnet_amd.linknet import pack_transposed
    g = _gen('self-check')
    checked = 0
    for k, s in ((3, 1), (3, 2), (5, 1), (5, 2)):
        b, a = R.same_pad(k, s)
        assert b == _same_pad_before(k, s)
        for H, W in itertools.product(range(1, 10), repeat=2):
            if H + b + a < k or W + b + a < k:
                continue                                          # the oracle's form has no output here
            x = torch.randn(2, 6, H, W, generator=g, dtype=torch.float64)
            w = torch.randn(6, 1, k, k, generator=g, dtype=torch.float64)
            want = R._conv_same(x, w, k, s, groups=6)
            Ho, Wo = want.shape[-2:]
            if s == 1:
                assert (Ho, Wo) == (H, W)
            elif H >= 2 and W >= 2:
                assert (Ho, Wo) == (H // 2, W // 2)               # what linknet.py passes as Ho, Wo
            got = conv_pad_crop(x, w, s, b, Ho, Wo, groups=6)
            assert got.shape == want.shape and (got - want).abs().max().item() <= 1e-12, (k, s, H, W)
            checked += 1
        # the stem's form: three input planes, dense filters, ceil(H / 2) outputs
        for H, W in ((3, 3), (4, 6), (5, 7)):
            x = torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
            w = torch.randn(5, 3, k, k, generator=g, dtype=torch.float64)
            if H + b + a >= k and W + b + a >= k:
                want = R._conv_same(x, w, k, s)
                got = conv_pad_crop(x, w, s, b, want.shape[-2], want.shape[-1])
                assert (got - want).abs().max().item() <= 1e-12
    assert checked > 250
    # windows larger than the image: by hand
    x = torch.tensor([[[[2.0]]]], dtype=torch.float64)
    w = torch.arange(25, dtype=torch.float64).view(1, 1, 5, 5)
    assert conv_pad_crop(x, w, 1, 2, 1, 1).item() == 2.0 * 12 and conv_pad_crop(x, w, 1, 0, 1, 1).item() == 0.0
    x = torch.arange(6, dtype=torch.float64).view(1, 1, 2, 3)
    assert conv_pad_crop(x, w, 2, 1, 1, 1).item() == sum(float(x[0, 0, i, j]) * float(w[0, 0, i + 1, j + 1]) for i in range(2) for j in range(3))

    for mid, mid_p in ((8, 32), (40, 64)):
        conv_t, bn = _transposed_layer(mid)
        wp, sc, sh = pack_transposed(conv_t, bn, mid_p, torch.device('cpu'))
        assert wp.shape == (256, 16 * mid_p) and sc.shape == sh.shape == (mid_p,)
        assert not wp[mid:].any() and not sc[mid:].any() and not sh[mid:].any()
        wc = wp[:mid_p].view(mid_p, 4, 4, mid_p).permute(0, 3, 1, 2).double()            # K ordered (kh, kw, cin)
        assert not wc[:, mid:].any()
        for h, w_ in ((1, 1), (2, 3), (5, 7)):
            x = torch.randn(1, mid, h, w_, generator=g, dtype=torch.float64)
            z = torch.zeros(1, mid_p, 2 * h, 2 * w_, dtype=torch.float64)
            z[:, :mid, ::2, ::2] = x
            acc = F.conv2d(F.pad(z, (2, 1, 2, 1)), wc)
            plain = F.conv_transpose2d(x, conv_t.weight.detach().double(), stride=2, padding=1)
            assert acc.shape == (1, mid_p, 2 * h, 2 * w_) and (acc[:, :mid] - plain).abs().max().item() <= 1e-12
            got = F.relu(acc * sc.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1))
            ref = transposed_ref(x, conv_t, bn, torch.float64)
            assert not got[:, mid:].any()
            assert (got[:, :mid] - ref).abs().max().item() <= 1e-5 * max(1.0, ref.abs().max().item())     # (scale / shift folded in float32)


# -------------------------------------------------------------------------------------------------------------- GPU tests
def _L():
    from vfloodnet_amd import _lib
    return _lib.lib()


@pytest.mark.gpu
@pytest.mark.parametrize('ld', [48, 64])
@pytest.mark.parametrize('hw', STEM_SIZES)
def test_stem_kernel(gpu, hw, ld):
    from vfloodnet_amd._lib import ptr, stream, check
    refs, ratio = _table('stem')
    H, W = hw
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    errs = []
    for case in [c for c in STEM_CASES if c[1] == hw and c[2] == ld]:
        N, _, _, pb = case
        x, w, sc, sh = (t.contiguous().to(gpu) for t in _stem_inputs(case))
        out = torch.full((N, Ho, Wo, ld), NAN, device=gpu)
        check(_L().vfn_ln_stem_f32(ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(out), N, H, W, Ho, Wo, ld, pb, stream()), 'vfn_ln_stem_f32')
        out = out.cpu()
        assert torch.equal(out[..., 48:], torch.zeros(N, Ho, Wo, ld - 48)), case
        errs.append((_err(out[..., :48].permute(0, 3, 1, 2), refs[case]), case))
    _report('stem', f'{H}x{W} ld {ld}', ratio, errs)
    x = torch.zeros(1, 3, 2, 8, device=gpu)
    with pytest.raises(RuntimeError):                      # an image smaller than the window, a leading dimension that is no multiple of 16
        check(_L().vfn_ln_stem_f32(ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(out.to(gpu)), 1, 2, 8, 1, 4, 48, 0, stream()), 'vfn_ln_stem_f32')
    with pytest.raises(RuntimeError):
        check(_L().vfn_ln_stem_f32(ptr(x), ptr(w), ptr(sc), ptr(sh), ptr(out.to(gpu)), 1, 3, 3, 2, 2, 56, 0, stream()), 'vfn_ln_stem_f32')


@pytest.mark.gpu
@pytest.mark.parametrize('k,s,swish_in', DW_KINDS)
def test_dwconv_kernel(gpu, k, s, swish_in):
    from vfloodnet_amd._lib import ptr, stream, check
    refs, ratio = _table('dwconv')
    errs, refused = [], 0
    for case in _dw_cases([(k, s, swish_in)]):
        _, _, _, pb, (H, W), N, (C, ld_x, ld_o) = case
        Ho, Wo = H // s, W // s
        x, w, sc, sh = _dw_inputs(case)
        wk = w.view(C, k * k).t().contiguous().to(gpu)             # tap-major [k*k][C], as LinknetB4._pack lays it out
        x, sc, sh = x.to(gpu), sc.to(gpu), sh.to(gpu)
        out = torch.full((N, max(Ho, 1), max(Wo, 1), ld_o), NAN, device=gpu)
        args = (ptr(x), ptr(wk), ptr(sc), ptr(sh), ptr(out), N, H, W, C, ld_x, ld_o, k, s, pb, Ho, Wo, swish_in, stream())
        if not _dw_legal(case):
            with pytest.raises(RuntimeError):
                check(_L().vfn_ln_dwconv_f32(*args), 'vfn_ln_dwconv_f32')
            refused += 1
            continue
        check(_L().vfn_ln_dwconv_f32(*args), 'vfn_ln_dwconv_f32')
        out = out.cpu()
        assert torch.isnan(out[..., C:]).all(), case                # C channels written, no more
        errs.append((_err(out[..., :C].permute(0, 3, 1, 2), refs[case]), case))
    assert refused == (len(_dw_pads(k, s)) * 2 * len(DW_CHANNELS) if s == 2 else 0)      # exactly the 1 x 1 images under stride 2
    _report('dwconv', f'k {k} stride {s} swish_in {swish_in}', ratio, errs)


@pytest.mark.gpu
@pytest.mark.parametrize('C,sq,Cpad', GATE_SHAPES)
def test_se_gate_kernel(gpu, C, sq, Cpad):
    from vfloodnet_amd._lib import ptr, stream, check
    refs, ratio = _table('gate')
    errs = []
    NB = 256
    for M in (1, 6, 300):
        case = ((C, sq, Cpad), M)
        x, w1, b1, w2, b2 = (t.contiguous().to(gpu) for t in _gate_inputs(case))
        sums, part, gate = torch.full((Cpad,), NAN, device=gpu), torch.full((NB * Cpad,), NAN, device=gpu), torch.full((Cpad,), NAN, device=gpu)
        check(_L().vfn_colsum_f32(ptr(x), M, Cpad, Cpad, ptr(part), NB, ptr(sums), stream()), 'vfn_colsum_f32')
        check(_L().vfn_ln_se_gate_f32(ptr(sums), 1.0 / M, ptr(w1), ptr(b1), ptr(w2), ptr(b2), ptr(gate), C, sq, Cpad, stream()),
              'vfn_ln_se_gate_f32')
        gate = gate.cpu()
        assert torch.equal(gate[C:], torch.zeros(Cpad - C)), case
        errs.append((_err(gate[:C], refs[case]), case))
    _report('se_gate', f'C {C} sq {sq} Cpad {Cpad}', ratio, errs)
    big = torch.zeros(257 * C, device=gpu)
    for bad_sq, bad_cpad in ((257, Cpad), (sq, C - 1)):
        with pytest.raises(RuntimeError):
            check(_L().vfn_ln_se_gate_f32(ptr(sums), 1.0, ptr(big), ptr(big), ptr(big), ptr(big), ptr(gate.to(gpu)), C, bad_sq, bad_cpad, stream()),
                  'vfn_ln_se_gate_f32')


@pytest.mark.gpu
@pytest.mark.parametrize('rows,K', [(1, 4), (3, 36), (256, 1632)])
def test_scale_cols_kernel(gpu, rows, K):
    from vfloodnet_amd._lib import ptr, stream, check
    g = _gen('scale_cols', rows, K)
    w, gate = torch.randn(rows, K, generator=g), torch.rand(K, generator=g)
    wd, gd = w.to(gpu), gate.to(gpu)
    out = torch.full((rows, K), NAN, device=gpu)
    check(_L().vfn_ln_scale_cols_f32(ptr(wd), ptr(gd), ptr(out), rows, K, stream()), 'vfn_ln_scale_cols_f32')
    assert torch.equal(out.cpu(), w * gate)                       # one rounding per element
    assert torch.equal(wd.cpu(), w)
    with pytest.raises(RuntimeError):
        check(_L().vfn_ln_scale_cols_f32(ptr(wd), ptr(gd), ptr(out), 1, 6, stream()), 'vfn_ln_scale_cols_f32')


@pytest.mark.gpu
@pytest.mark.parametrize('n', [4, 1028, 4 * 65537])
def test_add_kernel(gpu, n):
    from vfloodnet_amd._lib import ptr, stream, check
    g = _gen('add', n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    ad, bd = a.to(gpu), b.to(gpu)
    out = torch.full((n,), NAN, device=gpu)
    check(_L().vfn_ln_add_f32(ptr(ad), ptr(bd), ptr(out), n, stream()), 'vfn_ln_add_f32')
    assert torch.equal(out.cpu(), a + b)
    assert torch.equal(ad.cpu(), a) and torch.equal(bd.cpu(), b)
    check(_L().vfn_ln_add_f32(ptr(ad), ptr(bd), ptr(ad), n, stream()), 'vfn_ln_add_f32')       # in place, as the decoder's skip add
    assert torch.equal(ad.cpu(), a + b) and torch.equal(bd.cpu(), b)
    with pytest.raises(RuntimeError):
        check(_L().vfn_ln_add_f32(ptr(ad), ptr(bd), ptr(out), n + 2, stream()), 'vfn_ln_add_f32')


@pytest.mark.gpu
@pytest.mark.parametrize('prob', [0, 1])
@pytest.mark.parametrize('C,ld', HEAD_SHAPES)
def test_head_kernel(gpu, C, ld, prob):
    from vfloodnet_amd._lib import ptr, stream, check
    refs, ratio = _table('head')
    errs = []
    for M in (1, 257, 2048):
        case = ((C, ld), prob, M)
        x, w = (t.to(gpu) for t in _head_inputs(case))
        out = torch.full((M + 3,), NAN, device=gpu)
        check(_L().vfn_ln_head_f32(ptr(x), ptr(w), HEAD_BIAS, ptr(out), M, C, ld, prob, stream()), 'vfn_ln_head_f32')
        out = out.cpu()
        assert torch.isnan(out[M:]).all(), case
        errs.append((_err(out[:M], refs[case]), case))
    _report('head', f'C {C} ld {ld} prob {prob}', ratio, errs)


@pytest.mark.gpu
@pytest.mark.parametrize('C', [4, 36])
@pytest.mark.parametrize('small,large', [((1, 1), (2, 2)), ((3, 5), (6, 10)), ((3, 5), (5, 9))])
@pytest.mark.parametrize('N', [1, 2])
def test_dilate2_kernel(gpu, N, small, large, C):
    from vfloodnet_amd._lib import ptr, stream, check
    (Ho, Wo), (H, W) = small, large
    g = torch.randn(N, Ho, Wo, C, generator=_gen('dilate', N, small, large, C))
    gd = g.to(gpu)
    out = torch.full((N, H, W, C), NAN, device=gpu)
    check(_L().vfn_dilate2_f32(ptr(gd), ptr(out), N, Ho, Wo, H, W, C, stream()), 'vfn_dilate2_f32')
    want = torch.zeros(N, H, W, C)
    want[:, ::2, ::2] = g
    assert torch.equal(out.cpu(), want)


_WS = {}


def _workspace(gpu):
    from vfloodnet_amd.engine import WS_FLOATS
    if 'ws' not in _WS:
        _WS['ws'] = torch.empty(WS_FLOATS, device=gpu)
    return _WS['ws']


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', [(1, 1), (2, 3), (5, 7), (13, 13)])
@pytest.mark.parametrize('mid', [8, 40, 112])
def test_transposed_conv_through_the_implicit_gemm(gpu, mid, h, w):
    """The decoder's ConvTranspose2d(4, 2, 1) + BatchNorm + ReLU exactly as ``_predict_eager`` builds it -- the product's packing,
    vfn_dilate2_f32, a 4 x 4 / pad 2 descriptor with Ho / Wo / M overwritten -- through every tile configuration, every K split
    (both finishes) and ``LinknetB4._conv`` itself."""
    from vfloodnet_amd import ops, engine
    from vfloodnet_amd._lib import ptr, stream, check
    from vfloodnet_amd.linknet import LinknetB4, pack_transposed, _cp
    N, mid_p = 1, _cp(mid)
    conv_t, bn = _transposed_layer(mid)
    x = torch.randn(N, mid, h, w, generator=_gen('convT-x', mid, h, w)).relu()            # (the layer in front ends in a ReLU)
    with torch.no_grad():
        ref = transposed_ref(x, conv_t, bn, torch.float64)
    tol = 2e-4 * max(1.0, ref.abs().max().item())
    wp, sc, sh = pack_transposed(conv_t.to(gpu), bn.to(gpu), mid_p, gpu)
    a = torch.zeros(N, h, w, mid_p, device=gpu)
    a[..., :mid] = x.permute(0, 2, 3, 1).to(gpu)
    H2, W2 = 2 * h, 2 * w
    z = torch.full((N, H2, W2, mid_p), NAN, device=gpu)
    check(_L().vfn_dilate2_f32(ptr(a), ptr(z), N, h, w, H2, W2, mid_p, stream()), 'vfn_dilate2_f32')
    t = torch.empty(N, H2, W2, mid_p, device=gpu)

    def desc():
        d = ops.make_conv_desc(z, wp, mid_p, 4, 4, 1, 2, t, sc, sh, None, False, True, N=N, H=H2, W=W2)
        assert (d.Ho, d.Wo) == (H2 + 1, W2 + 1)                              # what the formula gives: one row / column too many
        d.Ho, d.Wo, d.M = H2, W2, N * H2 * W2
        return d

    def verify(what):
        torch.cuda.synchronize()
        got = t.cpu()
        assert torch.equal(got[..., mid:], torch.zeros(N, H2, W2, mid_p - mid)), what
        err = (got[..., :mid].permute(0, 3, 1, 2).double() - ref).abs().max().item()
        assert err == err and err < tol, (what, err, tol)
        return err

    worst, ran, skipped = 0.0, 0, []
    for cfg, (bm_, bn_) in enumerate(ops.conv_cfg_tiles()):
        if wp.shape[0] < ((mid_p + bn_ - 1) // bn_) * bn_:
            continue
        d = desc()
        if ops.conv_cfg_kind(cfg) == 2:
            ops.set_streamk(d, *ops.streamk_scratch(gpu))
        t.fill_(NAN)
        try:
            ops.conv2d_launch(d, cfg, 0)
        except RuntimeError as e:
            m = re.search(r'failed with status (-?\d+)', str(e))
            if m is None or int(m.group(1)) != VFN_ERR_ARG:
                raise
            skipped.append(cfg)
            continue
        worst = max(worst, verify(f'cfg {cfg}'))
        ran += 1
    d = desc()
    choice = engine.choose_cfg(d.M, d.Cout, d.KH * d.KW * d.Cin, 0)
    assert choice[0] not in skipped and ran > 0, (choice, skipped)
    # K splits: partial slabs + separate reduce, and the in-launch finish where whole filter tiles allow it
    ws = torch.empty(8 * t.numel(), device=gpu)
    cnt = torch.zeros(4096, dtype=torch.int32, device=gpu)
    splits = ops.valid_splits(d, 8)[1:]
    assert splits                                                # K = 16 taps x mid_p / 32 tiles: always divisible
    for ks in splits:
        outs = []
        for counters in (None, cnt if mid_p % 64 == 0 else None):
            t.fill_(NAN)
            ops.set_splitk(d, ks, ws, counters=counters)
            for _ in range(2):                                   # twice: the counters must return to rest
                ops.conv2d_launch(d, 3)
            worst = max(worst, verify(f'split {ks} counters {counters is not None}'))
            outs.append(t.clone())
        assert torch.equal(outs[0], outs[1]), 'in-launch finish must be bit-identical to the reduce launch'
        assert int(cnt.abs().sum()) == 0
    # ... and the product's own launcher
    t.fill_(NAN)
    LinknetB4._conv({'ws': _workspace(gpu)}, z, wp, mid_p, 4, 2, t, sc, sh, N, H2, W2, relu_out=True, Ho=H2, Wo=W2)
    worst = max(worst, verify('LinknetB4._conv'))
    print(f'transposed conv mid {mid} ({mid_p}) {h}x{w}: {ran} configurations + {len(splits)} splits, worst error {worst:.3e} (bound {tol:.3e}); '
          f'{len(skipped)} configurations refused the 4x4 descriptor {skipped}; choose_cfg -> {tuple(choice[:3])}')


# ------------------------------------------------------------------------------------ smallest inputs, feature by feature
@functools.lru_cache(maxsize=None)
def _weights():
    from tools import synth_linknet as S
    return S.make_state_dict(H=96, W=128)


def _nchw(tap, C):
    return tap[..., :C].permute(0, 3, 1, 2).cpu().double()


@pytest.mark.gpu
@pytest.mark.parametrize('H,W', [(32, 32), (32, 64), (64, 32)])
def test_smallest_inputs_feature_by_feature(gpu, H, W):
    """The smallest legal inputs (deepest feature 1 x 1: 5 x 5 depthwise windows larger than the image, 1 x 1 convolutions with
    M = 1): logits / probabilities within test_linknet_hip_vs_oracle's bounds of the float64 oracle, and every tapped feature
    within 8 x the float32 CPU oracle's own distance from it."""
    from oracle import linknet_ref as R
    from tools import synth_linknet as S
    from vfloodnet_amd.linknet import LinknetB4
    sd = _weights()
    x = S.frame(3, H, W)
    names = ['stem', 'stage 6', 'stage 10', 'stage 22', 'stage 32'] + [f'decoder {j}' for j in range(5)]

    def oracle(dt):
        s = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in sd.items()}
        with torch.no_grad():
            feats = R.encoder(s, x.to(dt))
            dec = []
            d = R.decoder(s, feats, taps=dec)
            z = F.conv2d(d, s['segmentation_head.0.weight'], s['segmentation_head.0.bias'])
        return feats[1:] + dec, z
    f64, z_ref = oracle(torch.float64)
    f32, _ = oracle(torch.float32)
    p_ref = torch.sigmoid(z_ref)
    model = LinknetB4.from_checkpoint(sd, gpu)
    taps = []
    z_eager = model._predict_eager(model._packed or model._pack(), x.to(gpu), True, taps=taps)
    z = model.predict(x.to(gpu), logits=True)
    assert torch.equal(z, z_eager)
    z = z.cpu().double()
    p = model.predict(x.to(gpu)).cpu().double()
    err = (z - z_ref).abs().max().item()
    print(f'linknet {H}x{W}: max |dlogit| {err:.2e} (logit std {z_ref.std().item():.2f}), max |dprob| {(p - p_ref).abs().max().item():.2e}')
    assert z.shape == z_ref.shape == (1, 1, H, W)
    assert err < 2e-3 and (p - p_ref).abs().max() < 5e-4
    sure = z_ref.abs() > 5e-3
    assert torch.equal((p > 0.5)[sure], (p_ref > 0.5)[sure])
    assert len(taps) == len(f64) == 10
    failures = []
    for name, tap, r64, r32 in zip(names, taps, f64, f32):
        C = r64.shape[1]
        assert tuple(tap.shape[:3]) == (1, r64.shape[2], r64.shape[3]) and tap.shape[3] >= C
        assert not tap[..., C:].any(), name                         # padded channels stay 0
        scale = r64.abs().max().item()
        ratio = (r32.double() - r64).abs().max().item() / scale
        got = (_nchw(tap, C) - r64).abs().max().item() / scale
        print(f'  {name:10s} [{C} x {r64.shape[2]} x {r64.shape[3]}]: float32 ratio {ratio:.3e}  bound {FACTOR * ratio:.3e}  HIP {got:.3e}')
        if not got <= FACTOR * ratio:
            failures.append((name, got, FACTOR * ratio))
    assert not failures, failures
    # a batch of two different frames = the two single-frame calls, bit for bit
    xa, xb = x.to(gpu), S.frame(4, H, W).to(gpu)
    both = model.predict(torch.cat([xa, xb], 0))
    assert both.shape == (2, 1, H, W) and not torch.equal(both[0], both[1])
    assert torch.equal(both[0:1], model.predict(xa)) and torch.equal(both[1:2], model.predict(xb))
