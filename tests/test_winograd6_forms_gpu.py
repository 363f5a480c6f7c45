"""The forms of the F(6x6) transforms (csrc/conv_winograd.hip; include/vfn_winograd6.h: vfn_winograd6_form): the lane-split form (2)
and the measured rule (auto) write the bytes of form 0 -- input transform, output transform with every epilogue, and a whole layer --
and meet the float64 bounds of tests/test_winograd6_gpu.py on their own.  Setting 1 named a wave-uniform variant of form 0 that was
measured out: it selects form 0 and stays in the cases, so that they cover whatever it selects."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout): the four of tests/test_winograd6_gpu.py; one tile exactly, a wave spanning tiles; C / 2 = 66 (a wave straddles
# two tiles), ragged on both edges, the tile index crossing images; several waves per tile, KeyValue's Cout
CASES = [(1, 5, 7, 32, 32), (2, 12, 20, 64, 64), (1, 13, 19, 128, 96), (2, 30, 54, 256, 256),
         (1, 6, 6, 36, 20), (2, 8, 14, 132, 260), (1, 7, 7, 512, 640)]
FORMS = {'1': 1, '2': 2, 'auto': 3}          # the argument of vfn_winograd6_force_form (3: the rule, whatever VFN_WINO6_XFORM says)

BT = torch.tensor([[1, 0, -21 / 4, 0, 21 / 4, 0, -1, 0],
                   [0, 1, 1, -17 / 4, -17 / 4, 1, 1, 0], [0, -1, 1, 17 / 4, -17 / 4, -1, 1, 0],
                   [0, 1 / 2, 1 / 4, -5 / 2, -5 / 4, 2, 1, 0], [0, -1 / 2, 1 / 4, 5 / 2, -5 / 4, -2, 1, 0],
                   [0, 2, 4, -5 / 2, -5, 1 / 2, 1, 0], [0, -2, 4, 5 / 2, -5, -1 / 2, 1, 0],
                   [0, -1, 0, 21 / 4, 0, -21 / 4, 0, 1]], dtype=torch.float64)
AT = torch.tensor([[1, 1, 1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 1 / 2, -1 / 2, 0], [0, 1, 1, 4, 4, 1 / 4, 1 / 4, 0],
                   [0, 1, -1, 8, -8, 1 / 8, -1 / 8, 0], [0, 1, 1, 16, 16, 1 / 16, 1 / 16, 0],
                   [0, 1, -1, 32, -32, 1 / 32, -1 / 32, 1]], dtype=torch.float64)


@contextlib.contextmanager
def forced(form):
    from vfloodnet_amd import _lib
    L = _lib.lib()
    assert L.vfn_winograd6_force_form(form) == 0
    try:
        yield L
    finally:
        assert L.vfn_winograd6_force_form(-1) == 0


def _taken(L, name, case, C, is_output, has_res):
    """The form the call takes: 2 when forced, 0 for setting 1, one of the two under the rule."""
    N, H, W = case[:3]
    got = L.vfn_winograd6_form(N, H, W, C, is_output, has_res)
    assert got in {'1': (0,), '2': (2,), 'auto': (0, 2)}[name], (name, got)
    return got


_IN, _OUT = {}, {}


def _input_data(case, relu):
    """x and the float64 transform of one case, computed once and shared (never modified)."""
    if (case, relu) not in _IN:
        N, H, W, C, _ = case
        x = torch.randn(N, C, H, W, generator=torch.Generator().manual_seed(2000 + CASES.index(case)))
        th, tw = (H + 5) // 6, (W + 5) // 6
        xin = (F.relu(x) if relu else x).double()
        xp = F.pad(xin, (1, 6 * tw + 1 - W, 1, 6 * th + 1 - H))
        patches = xp.unfold(2, 8, 6).unfold(3, 8, 6)                                   # [N, C, th, tw, 8, 8]
        V64 = torch.einsum('ia,nctuab,jb->ijntuc', BT, patches, BT).reshape(64, N * th * tw, C)
        _IN[(case, relu)] = (x, V64, 16 * 2.0 ** -24 * 12.5 ** 2 * xin.abs().max().item())
    return _IN[(case, relu)]


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('relu', [False, True])
@pytest.mark.parametrize('case', CASES)
def test_input_forms_equal_form0_and_meet_the_float64_bound(gpu, case, relu, form):
    """V pre-filled with NaN; from a contiguous tensor and from a NaN-filled allocation with ld_x = C + 8 (a tap outside the image that
    was read would surface as a NaN): torch.equal with form 0's V, zeros in rows >= tiles, |V - V64| <= 16 * 2^-24 * 12.5^2 * max|d|."""
    from vfloodnet_amd import ops
    N, H, W, C, _ = case
    x, V64, bound = _input_data(case, relu)
    tiles, rows = ops.winograd6_tiles(N, H, W), ops.winograd6_rows(N, H, W)
    xd = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    ld = C + 8
    big = torch.full((N * H * W + 2 * W + 32, ld), float('nan'), device=gpu)
    inner = big[W + 16:W + 16 + N * H * W]
    inner[:, :C] = xd.view(-1, C)

    def run(strided):
        V = torch.full((64, rows, C), float('nan'), device=gpu)
        if strided:
            ops.winograd_input(inner, V, rows, relu, N, H, W, C, ld, tile=6)
        else:
            ops.winograd_input(xd, V, rows, relu, tile=6)
        return V

    with forced(0):
        V0 = [run(False), run(True)]
    with forced(FORMS[form]) as L:
        took = _taken(L, form, case, C, 0, 0)
        V1 = [run(False), run(True)]
    err = (V1[0][:, :tiles].cpu().double() - V64).abs().max().item()
    print(f'{case} relu={relu} form {form} (takes {took}): max |V - V64| {err:.3e} (bound {bound:.3e})')
    for strided in (0, 1):
        assert torch.equal(V1[strided], V0[strided]), (form, took, strided)
        assert bool((V1[strided][:, tiles:] == 0).all())
    assert err <= bound, (err, bound)


def _output_data(case):
    if case not in _OUT:
        N, H, W, _, Cout = case
        th, tw = (H + 5) // 6, (W + 5) // 6
        rows = (N * th * tw + 63) // 64 * 64
        g = torch.Generator().manual_seed(3000 + CASES.index(case))
        M = torch.randn(64, rows, Cout, generator=g)
        Y64 = torch.einsum('ia,abntuc,jb->ntiujc', AT, M[:, :N * th * tw].double().view(8, 8, N, th, tw, Cout), AT)
        Y64 = Y64.reshape(N, 6 * th, 6 * tw, Cout)[:, :H, :W]
        _OUT[case] = dict(M=M, Y64=Y64, rows=rows, scale=1 + 0.1 * torch.randn(Cout, generator=g), shift=0.1 * torch.randn(Cout, generator=g),
                          res=torch.randn(N * H * W, Cout, generator=g))
    return _OUT[case]


GUARD = -12345.0
VARIANTS = ['plain', 'affine_relu', 'res', 'res_mod', 'nan_in_M', 'nan_in_res']


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('case', CASES)
def test_output_forms_equal_form0_and_meet_the_float64_bound(gpu, case, form):
    """Random M; a guard-filled output with out_ld = Cout + 4 and spare rows.  No epilogue; scale + shift + ReLU; a residual; a residual
    with res_mod = H W; a NaN seeded into M; a NaN seeded into the residual: torch.equal with form 0 (so a NaN comes out where form 0 puts
    it), guards intact, and |Y - Y64| <= 16 * 2^-24 * 67.0625^2 * max|M| without an epilogue."""
    from vfloodnet_amd import ops
    N, H, W, _, Cout = case
    d = _output_data(case)
    rows, ld, npix = d['rows'], Cout + 4, N * H * W
    Md, sc, sh, resd = d['M'].to(gpu), d['scale'].to(gpu), d['shift'].to(gpu), d['res'].to(gpu)
    Mnan = Md.clone()
    Mnan[11, 0, Cout // 2] = float('nan')
    Mnan[63, (N * ((H + 5) // 6) * ((W + 5) // 6)) - 1, Cout - 1] = float('nan')
    resnan = resd.clone()
    resnan[npix // 2, Cout // 3] = float('nan')
    res1 = resd[:H * W].contiguous()

    def run(variant):
        buf = torch.full((npix + 7 * W + 64, ld), GUARD, device=gpu)
        m, scale, shift, res, res_mod, relu = Md, None, None, None, 0, False
        if variant == 'affine_relu':
            scale, shift, relu = sc, sh, True
        elif variant == 'res':
            scale, shift, res = sc, sh, resd
        elif variant == 'res_mod':
            scale, shift, res, res_mod, relu = sc, sh, res1, H * W, True
        elif variant == 'nan_in_M':
            m, scale, shift, relu = Mnan, sc, sh, True
        elif variant == 'nan_in_res':
            res, relu = resnan, True
        ops.winograd_output(m, rows, buf, N, H, W, Cout, scale, shift, res, Cout if res is not None else 0, res_mod, relu, out_ld=ld, tile=6)
        return buf

    with forced(0):
        ref = {v: run(v) for v in VARIANTS}
    with forced(FORMS[form]) as L:
        took = (_taken(L, form, case, Cout, 1, 0), _taken(L, form, case, Cout, 1, 1))
        got = {v: run(v) for v in VARIANTS}
    for v in VARIANTS:
        # (torch.equal is false for a NaN against itself: compare the bit patterns)
        assert torch.equal(got[v].view(torch.int32), ref[v].view(torch.int32)), (form, took, v)
        assert bool((got[v][:, Cout:] == GUARD).all()) and bool((got[v][npix:] == GUARD).all()), v
    for v in ('nan_in_M', 'nan_in_res'):
        assert bool(torch.isnan(ref[v][:npix, :Cout]).any()) and bool(torch.isnan(got[v][:npix, :Cout]).any())
    bound = 16 * 2.0 ** -24 * 67.0625 ** 2 * d['M'].abs().max().item()
    err = (got['plain'][:npix, :Cout].view(N, H, W, Cout).cpu().double() - d['Y64']).abs().max().item()
    print(f'{case} form {form} (takes {took}): max |Y - Y64| {err:.3e} (bound {bound:.3e})')
    assert err <= bound, (err, bound)


@pytest.mark.parametrize('form', list(FORMS))
@pytest.mark.parametrize('case', [(2, 12, 20, 64, 64), (2, 30, 54, 256, 256)])
def test_layer_under_each_form_equals_form0(gpu, case, form):
    """ops.conv2d_winograd(tile=6) -- transforms and GEMMs -- with ReLU in and out, scale, shift and a residual, and with nothing."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout = case
    g = torch.Generator().manual_seed(4000 + Cin)
    x = torch.randn(N, H, W, Cin, generator=g).to(gpu)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    kw = dict(scale=(1 + 0.1 * torch.randn(Cout, generator=g)).to(gpu), shift=(0.1 * torch.randn(Cout, generator=g)).to(gpu),
              res=torch.randn(N, H, W, Cout, generator=g).to(gpu), relu_in=True, relu_out=True)
    cfg = ops.wino_gemm_cfg(3, 512)
    with forced(0):
        ref = [ops.conv2d_winograd(x, w, cfg=cfg, tile=6, **kw), ops.conv2d_winograd(x, w, cfg=cfg, tile=6)]
    with forced(FORMS[form]):
        got = [ops.conv2d_winograd(x, w, cfg=cfg, tile=6, **kw), ops.conv2d_winograd(x, w, cfg=cfg, tile=6)]
    assert torch.equal(got[0], ref[0]) and torch.equal(got[1], ref[1])
