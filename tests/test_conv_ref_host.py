"""tests/conv_ref.py checked on the CPU: the epilogue against autograd, the 2e-5 condition of every case, the planted mask values
and the layout builder's guards."""
import pytest
import torch
from torch.nn import functional as F

import conv_ref
from conv_ref import BIG, GEOMS, GUARD, NAN, STRIDES, VARIANTS


@pytest.mark.parametrize('mask_after', [0, 1])
def test_epilogue_is_the_data_gradient_of_autograd(mask_after):
    """d/dx of conv(relu(x)) (+ a skip branch) equals the ``mask = x`` form of the epilogue over the flipped, transposed filters:
    mask_after = 0: the skip leaves from x itself (its gradient is added unmasked); 1: it leaves from relu(x) (masked with the sum)."""
    g = torch.Generator().manual_seed(3 + mask_after)
    x = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(4, 6, 3, 3, generator=g, dtype=torch.float64)
    gy = torch.randn(2, 4, 5, 7, generator=g, dtype=torch.float64)
    gs = torch.randn(2, 6, 5, 7, generator=g, dtype=torch.float64)
    with torch.no_grad():
        x.view(-1)[::5] = 0.0                       # the gradient of relu at 0 is 0: pins ``> 0``
    loss = (F.conv2d(torch.relu(x), w, padding=1) * gy).sum() + ((torch.relu(x) if mask_after else x) * gs).sum()
    loss.backward()
    wt = w.flip(2, 3).transpose(0, 1)
    conv = conv_ref.rows(F.conv2d(gy, wt, padding=1))
    got = conv_ref.epilogue(conv, None, None, conv_ref.rows(gs), 0, conv_ref.rows(x.detach()), mask_after, False)
    assert (got - conv_ref.rows(x.grad)).abs().max().item() < 1e-12


def test_epilogue_scale_shift_res_mod_and_relu():
    conv = torch.tensor([[1.0, -2.0], [3.0, 4.0], [-5.0, 6.0], [7.0, -8.0]], dtype=torch.float64)
    res = torch.tensor([[10.0, 20.0], [-30.0, -40.0]], dtype=torch.float64)
    got = conv_ref.epilogue(conv, torch.tensor([2.0, 3.0]), torch.tensor([1.0, -1.0]), res, 2, None, False, True)
    want = torch.tensor([[13.0, 13.0], [0.0, 0.0], [1.0, 37.0], [0.0, 0.0]], dtype=torch.float64)
    assert torch.equal(got, want)
    assert torch.isnan(conv_ref.epilogue(torch.tensor([[NAN]]), None, None, None, 0, None, False, True)).all()


@pytest.mark.parametrize('mode', [0, 1, 2])
def test_every_case_meets_the_bound(mode):
    """make_case refuses a case whose 8 x ratio is not below 2e-5: building every case the GPU tests use is the assertion."""
    worst = 0.0
    cases = conv_ref.case_list(mode)
    assert len(cases) == {0: 44, 1: 5, 2: 14}[mode]
    for geom, variant in cases:
        c = conv_ref.make_case(geom, variant, mode)
        assert 0 < c.bound < conv_ref.BOUND_CAP and c.ref.shape == (c.M, geom[4]) and c.ref.dtype == torch.float64
        worst = max(worst, c.ratio)
    for variant in ('none', 'full'):
        worst = max(worst, conv_ref.make_bank_case(variant=variant).ratio)
    if mode == 0:                       # the extra variant of the NaN launches (a mask and both ReLUs)
        for geom in (GEOMS[2], GEOMS[7], GEOMS[9]):
            worst = max(worst, conv_ref.make_case(geom, 'mask_relu').ratio)
    print(f'mode {mode}: worst float32 ratio {worst:.2e}')
    if mode == 1:
        assert all(g[3] % 64 == 0 for g, _ in cases) and (2, 6, 10, 160, 136, 1, 1) not in [g for g, _ in cases]


def test_pack_is_the_package_filter_layout():
    from vfloodnet_amd import weights
    w = torch.randn(5, 32, 3, 3)
    assert torch.equal(conv_ref.pack(w), weights.pack_conv_weight(w))


def test_korder_sum_and_reduced_products_agree_with_float64():
    g = torch.Generator().manual_seed(9)
    x, w = torch.randn(2, 32, 5, 6, generator=g), torch.randn(7, 32, 3, 3, generator=g) / 17
    for mode, tol in ((0, 1e-6), (1, 1e-6), (2, 1e-6)):
        ref = conv_ref.products(x, w, 2, 1, mode, torch.float64)
        assert conv_ref.rel(conv_ref.korder_sum(x, w, 2, mode), ref) < tol
        assert conv_ref.rel(conv_ref.products(x, w, 2, 1, mode, torch.float32), ref) < tol
    exact = conv_ref.products(x, w, 2, 1, 0, torch.float64)
    assert 1e-4 < conv_ref.rel(conv_ref.products(x, w, 2, 1, 1, torch.float64), exact) < 2e-2
    assert conv_ref.rel(conv_ref.products(x, w, 2, 1, 2, torch.float64), exact) < 1e-4


def test_mask_plants_the_values_that_pin_the_comparison():
    m = conv_ref.mask_tensor(70, 36, torch.Generator().manual_seed(1))
    flat = m.view(-1)
    signs = torch.signbit(flat[flat == 0])
    assert bool(signs.any()) and not bool(signs.all())                   # +0 and -0
    assert bool((flat == 1.1754944e-38).any()) and bool((flat == -1.1754944e-38).any())
    assert bool((m[35] <= 0).all()) and bool((m[69] > 0).all())
    assert not bool(((flat != 0) & (flat.abs() < 1.1754944e-38)).any())  # no subnormals


@pytest.mark.parametrize('strides', sorted(STRIDES))
@pytest.mark.parametrize('variant', ['none', 'full', 'mask_after'])
def test_layout_puts_its_guards_where_it_says(variant, strides):
    geom = GEOMS[2]
    c = conv_ref.make_case(geom, variant)
    L = conv_ref.Layout(c, strides, 'cpu')
    go, gr, gm = STRIDES[strides]
    Cin, Cout, M = geom[3], geom[4], c.M
    poison = BIG if variant == 'full' else NAN

    def is_poison(t, p):
        return bool(torch.isnan(t).all()) if p != p else bool((t == p).all())

    def guards(alloc, view, nrows, ncols, ld, off, p):
        assert alloc.shape == (nrows + 2 * GUARD, ld) and view.shape == (nrows, ncols) and view.stride() == (ld, 1)
        assert view.data_ptr() == alloc.data_ptr() + 4 * (GUARD * ld + off)
        outside = torch.ones_like(alloc, dtype=torch.bool)
        outside[GUARD:GUARD + nrows, off:off + ncols] = False
        assert is_poison(alloc[outside], p) and int(outside.sum()) == alloc.numel() - nrows * ncols
    guards(L.x_alloc, L.x, c.x.shape[0], Cin, Cin + 8, 4, poison)
    assert L.in_ld == Cin + 8 and torch.equal(L.x, c.x)
    guards(L.out_alloc, L.out, M, Cout, Cout + go, 4 if strides == 'wide' else 1, NAN)
    assert bool(torch.isnan(L.out_alloc).all()) and L.out_ld == Cout + go
    if c.res is not None:
        guards(L.res_alloc, L.res, M, Cout, Cout + gr, 4 if strides == 'wide' else 1, poison)
        assert torch.equal(L.res, c.res) and L.res_ld == Cout + gr
    if c.mask is not None:
        guards(L.mask_alloc, L.mask, M, Cout, Cout + gm, 8 if strides == 'wide' else 2, poison)
        assert torch.equal(conv_ref.bits(L.mask), conv_ref.bits(c.mask)) and L.mask_ld == Cout + gm
    if strides == 'wide':
        assert all(t.data_ptr() % 16 == 0 for t in (L.x, L.out, L.res, L.mask) if t is not None)
    else:
        assert L.out_ld % 4 and (L.res is None or L.res_ld % 4) and (L.mask is None or L.mask_ld % 4)
    # collect(): a result inside the bound, a write one column past Cout and a missing NaN each show
    L.out.copy_(c.ref.float())
    err, dirty, image = L.collect()
    assert err.item() < c.bound and dirty.item() == 0 and torch.equal(image, c.ref.float()) and bool(torch.isnan(L.out_alloc).all())
    L.out.copy_(c.ref.float())
    if strides == 'wide':                                   # (the slice ends at the row's end: one column past Cout is the next row's gutter)
        L.out_alloc[GUARD + 2, 0] = 1.0
    else:
        L.out_alloc[GUARD + 1, 1 + Cout] = 1.0
    assert L.collect()[1].item() == 1
    L.out.copy_(c.ref.float())
    L.out[3, 2] = NAN
    assert L.collect()[0].item() == float('inf')
