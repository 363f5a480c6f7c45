"""HIP implicit-GEMM conv vs torch CPU fp32 ``F.conv2d`` (the op's fp32 reference)."""
import pytest
import torch
from torch.nn import functional as F

from conv_ref import _reduced_reference

pytestmark = pytest.mark.gpu

# (N, H, W, Cin, Cout, k, stride, relu_in, relu_out, residual)
CASES = [
    (1, 12, 20, 64, 64, 1, 1, False, True, False),
    (2, 12, 20, 64, 256, 1, 1, False, False, True),
    (1, 13, 19, 128, 128, 3, 2, False, True, False),
    (2, 9, 14, 256, 256, 3, 1, True, False, True),
    (1, 16, 24, 256, 512, 1, 2, False, False, False),
    (2, 7, 11, 1024, 640, 3, 1, False, False, False),
    (2, 30, 40, 32, 32, 3, 1, True, False, True),
    (2, 10, 12, 256, 2, 3, 1, True, False, False),
    (1, 33, 47, 64, 96, 3, 1, False, True, True),
]


@pytest.mark.parametrize('case', CASES)
def test_conv_matches_torch_cpu(gpu, case):
    from vfloodnet_amd import ops, weights
    N, H, W, Cin, Cout, k, s, relu_in, relu_out, use_res = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = 1 + 0.1 * torch.randn(Cout, generator=g)
    shift = 0.1 * torch.randn(Cout, generator=g)
    xin = F.relu(x) if relu_in else x
    ref = F.conv2d(xin, w, stride=s, padding=k // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = torch.randn(ref.shape, generator=g) if use_res else None
    if use_res:
        ref = ref + res
    if relu_out:
        ref = F.relu(ref)
    scale_d, shift_d = scale.to(gpu), shift.to(gpu)      # descriptors hold raw pointers: keep the tensors alive
    xd = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    wp = ops.pad_rows(weights.pack_conv_weight(w)).to(gpu)
    resd = res.permute(0, 2, 3, 1).contiguous().to(gpu) if use_res else None
    for cfg, (bm_, bn_) in enumerate(ops.conv_cfg_tiles()):
        if wp.shape[0] < ((Cout + bn_ - 1) // bn_) * bn_:
            continue
        y = ops.conv2d_nhwc(xd, wp, Cout, k, k, s, k // 2, scale_d, shift_d, resd,
                            relu_in, relu_out, cfg=cfg)
        torch.cuda.synchronize()
        got = y.permute(0, 3, 1, 2).cpu()
        err = (got - ref).abs().max().item()
        assert err < 2e-4 * max(1.0, ref.abs().max().item()), f'cfg {cfg}: max err {err}'
    # split-K variants (partial slabs + fixed-order reduce)
    ws = torch.empty(8 * ref.numel(), device=gpu)
    y = torch.empty(N, ref.shape[2], ref.shape[3], Cout, device=gpu)
    d = ops.make_conv_desc(xd, wp, Cout, k, k, s, k // 2, y, scale_d, shift_d, resd, relu_in, relu_out)
    cnt = torch.zeros(4096, dtype=torch.int32, device=gpu)
    for ks in ops.valid_splits(d, 8)[1:]:
        outs = []
        for counters in (None, cnt if Cout % 64 == 0 else None):       # separate reduce launch / in-launch finish
            y.zero_()
            ops.set_splitk(d, ks, ws, counters=counters)
            for _ in range(2):                                          # twice: the counters must return to rest
                ops.conv2d_launch(d, 3)
            torch.cuda.synchronize()
            err = (y.permute(0, 3, 1, 2).cpu() - ref).abs().max().item()
            assert err < 2e-4 * max(1.0, ref.abs().max().item()), f'split {ks}: max err {err}'
            outs.append(y.clone())
        assert torch.equal(outs[0], outs[1]), 'in-launch finish must be bit-identical to the reduce launch'
        assert int(cnt.abs().sum()) == 0
    # tail split: only the tiles from an n-tile-aligned index on are cut along K
    tiles = ops.conv_cfg_tiles()
    bm, bn = tiles[3]
    n_t = (Cout + bn - 1) // bn
    m_t = (d.M + bm - 1) // bm
    for full_m in {1, m_t // 2, m_t - 1}:
        if 0 < full_m < m_t and len(ops.valid_splits(d, 4)) > 1:
            ks = ops.valid_splits(d, 4)[-1]
            y.zero_()
            ops.set_splitk(d, ks, ws, split_from=full_m * n_t, rows=d.M - full_m * bm)
            ops.conv2d_launch(d, 3)
            torch.cuda.synchronize()
            err = (y.permute(0, 3, 1, 2).cpu() - ref).abs().max().item()
            assert err < 2e-4 * max(1.0, ref.abs().max().item()), f'tail split from {full_m}: max err {err}'


BF16_CASES = [
    (1, 12, 20, 64, 64, 1, 1, False, True, False),
    (2, 12, 20, 64, 256, 1, 1, False, False, True),
    (1, 13, 19, 128, 128, 3, 2, False, True, False),
    (2, 9, 14, 256, 256, 3, 1, True, False, True),
    (2, 7, 11, 1024, 640, 3, 1, False, False, False),
    (1, 33, 47, 64, 96, 3, 1, False, True, True),
]


@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('case', BF16_CASES)
def test_conv_reduced_precision_matches_emulation(gpu, case, mode):
    """bf16 / bf16x3 kernels against an f64 evaluation of exactly the products they form (operands rounded /
    split on the host the same way, nearest-even): only the f32 summation order differs."""
    from vfloodnet_amd import ops, weights
    N, H, W, Cin, Cout, k, s, relu_in, relu_out, use_res = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    scale = 1 + 0.1 * torch.randn(Cout, generator=g)
    shift = 0.1 * torch.randn(Cout, generator=g)
    xin = F.relu(x) if relu_in else x
    ref = _reduced_reference(xin, w, s, k // 2, mode) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    exact = F.conv2d(xin, w, stride=s, padding=k // 2) * scale.view(1, -1, 1, 1) + shift.view(1, -1, 1, 1)
    res = torch.randn(ref.shape, generator=g) if use_res else None
    if use_res:
        ref = ref + res
        exact = exact + res
    if relu_out:
        ref = F.relu(ref)
        exact = F.relu(exact)
    scale_d, shift_d = scale.to(gpu), shift.to(gpu)
    xd = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    wp = ops.pad_rows(weights.pack_conv_weight(w)).to(gpu)
    resd = res.permute(0, 2, 3, 1).contiguous().to(gpu) if use_res else None
    tiles = ops.conv_cfg_tiles()
    tol = 2e-4 * max(1.0, ref.abs().max().item())
    for cfg in ops.conv_cfgs(mode):
        if wp.shape[0] < ((Cout + tiles[cfg][1] - 1) // tiles[cfg][1]) * tiles[cfg][1]:
            continue
        y = ops.conv2d_nhwc(xd, wp, Cout, k, k, s, k // 2, scale_d, shift_d, resd, relu_in, relu_out, cfg=cfg, mode=mode)
        torch.cuda.synchronize()
        got = y.permute(0, 3, 1, 2).cpu()
        err = (got - ref).abs().max().item()
        assert err < tol, f'cfg {cfg}: max err {err}'
    # filters converted on the host (vfn_conv_desc.w_packed): bit-identical to the on-the-fly conversion
    wlp = ops.pack_weights_lp(wp, mode)
    y2 = torch.empty_like(y)
    d2 = ops.make_conv_desc(xd, wp, Cout, k, k, s, k // 2, y2, scale_d, shift_d, resd, relu_in, relu_out)
    ops.use_packed_weights(d2, wlp)
    ops.conv2d_launch(d2, cfg, mode)
    torch.cuda.synchronize()
    assert torch.equal(y2, y), 'packed-weight path differs from the on-the-fly conversion'
    # distance from the exact f32 convolution: what the mode costs (bf16x3 ~2^-16 per product, bf16 ~2^-9)
    dev_exact = (got - exact).abs().max().item() / max(1.0, exact.abs().max().item())
    assert dev_exact < (2e-2 if mode == 1 else 1e-4), dev_exact
    ws = torch.empty(8 * ref.numel(), device=gpu)
    y = torch.empty(N, ref.shape[2], ref.shape[3], Cout, device=gpu)
    d = ops.make_conv_desc(xd, wp, Cout, k, k, s, k // 2, y, scale_d, shift_d, resd, relu_in, relu_out)
    for ks in ops.valid_splits(d, 8, mode=mode)[1:]:
        y.zero_()
        ops.set_splitk(d, ks, ws)
        ops.conv2d_launch(d, 3, mode=mode)
        torch.cuda.synchronize()
        err = (y.permute(0, 3, 1, 2).cpu() - ref).abs().max().item()
        assert err < tol, f'split {ks}: max err {err}'


@pytest.mark.parametrize('mode', [1, 2])
def test_reduced_precision_refuses_the_f32_only_configurations(gpu, mode):
    """A reduced-precision entry point launches exactly the configurations whose vfn_conv_cfg_modes bit it owns: every other id in
    0..61 (LDS-DMA staging, the f32-only tiles, the wave-autonomous and stream-K kernels) is refused before anything is launched.
    The tensors are valid for every tile, so a wrong dispatch would still be a well-formed launch."""
    from vfloodnet_amd import _lib, ops, weights
    g = torch.Generator().manual_seed(5)
    x = torch.randn(1, 12, 20, 64, generator=g).to(gpu)
    wp = ops.pad_rows(weights.pack_conv_weight(torch.randn(64, 64, 1, 1, generator=g) / 8)).to(gpu)
    y = torch.empty(1, 12, 20, 64, device=gpu)
    d = ops.make_conv_desc(x, wp, 64, 1, 1, 1, 0, y, None, None, None, False, True)
    tiles = ops.conv_cfg_tiles()
    assert len(tiles) == 62
    ran = 0
    for cfg, (bm, bn) in enumerate(tiles):
        if not _lib.lib().vfn_conv_cfg_modes(cfg) >> mode & 1:
            with pytest.raises(RuntimeError):
                ops.conv2d_launch(d, cfg, mode)
        elif wp.shape[0] >= ((64 + bn - 1) // bn) * bn:
            y.fill_(float('nan'))
            ops.conv2d_launch(d, cfg, mode)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(y).all()), cfg
            ran += 1
    assert ran == len(ops.conv_cfgs(mode)) == 27


@pytest.mark.parametrize('shape', [(2, 12, 20, 64, 128, 3, 1), (1, 13, 19, 128, 64, 3, 2), (2, 9, 14, 256, 256, 1, 1), (1, 24, 40, 32, 32, 3, 1)])
@pytest.mark.parametrize('relu', [False, True])
def test_split_bf16_activation_image_round_trip(gpu, shape, relu):
    """bf16x3 with the activations' split-bf16 image (vfn_conv_desc.out_lp / in_lp): a producer writes the image of (the ReLU
    of) its result from its epilogue -- with and without the f32 tensor, through the plain, the split-K and the in-workgroup
    split-K epilogues -- and a consumer stages it without conversion.  The image must hold exactly hi = bf16(y),
    lo = bf16(y - hi); the consumer must give the SAME BITS as the on-the-fly split of the f32 tensor (same operands, same
    order of MFMAs)."""
    from vfloodnet_amd import ops, weights
    from vfloodnet_amd._lib import ptr
    N, H, W, Cin, Cmid, k, s = shape
    g = torch.Generator().manual_seed(sum(shape) + relu)
    x = torch.randn(N, H, W, Cin, generator=g).to(gpu)
    w1 = torch.randn(Cmid, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5
    w2 = torch.randn(96, Cmid, 3, 3, generator=g) / (Cmid * 9) ** 0.5
    wp1 = ops.pad_rows(weights.pack_conv_weight(w1)).to(gpu)
    wp2 = ops.pad_rows(weights.pack_conv_weight(w2)).to(gpu)
    sc = (1 + 0.1 * torch.randn(Cmid, generator=g)).to(gpu)
    sh = (0.1 * torch.randn(Cmid, generator=g)).to(gpu)
    Ho, Wo = (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1
    res = torch.randn(N, Ho, Wo, Cmid, generator=g).to(gpu)
    # reference: f32 tensor y from the plain bf16x3 kernel, consumer with on-the-fly split (+ ReLU on the input)
    y = torch.empty(N, Ho, Wo, Cmid, device=gpu)
    d1 = ops.make_conv_desc(x, wp1, Cmid, k, k, s, k // 2, y, sc, sh, res, False, False)
    ops.conv2d_launch(d1, 3, 2)
    z_ref = torch.empty(N, Ho, Wo, 96, device=gpu)
    d2 = ops.make_conv_desc(y, wp2, 96, 3, 3, 1, 1, z_ref, None, None, None, relu, False)
    ops.conv2d_launch(d2, 3, 2)
    torch.cuda.synchronize()
    yr = torch.relu(y) if relu else y
    hi = yr.bfloat16()
    lo = (yr - hi.float()).bfloat16()
    want = torch.cat([hi.view(-1, Cmid // 32, 32), lo.view(-1, Cmid // 32, 32)], dim=2).reshape(N, Ho, Wo, Cmid * 2)
    ws = torch.empty(8 * y.numel(), device=gpu)
    for variant in ('plain', 'image_only', 'split_k', 'wk'):
        img = torch.zeros(N, Ho, Wo, Cmid, device=gpu)                       # the twin: same bytes as y
        y2 = torch.full_like(y, float('nan'))
        d = ops.make_conv_desc(x, wp1, Cmid, k, k, s, k // 2, y2, sc, sh, res, False, False)
        d.out_lp, d.out_lp_relu = ptr(img), int(relu)
        cfg = 3
        if variant == 'image_only':
            d.out = None
        elif variant == 'split_k':
            splits = ops.valid_splits(d, 8, mode=2)
            if len(splits) < 2:
                continue
            ops.set_splitk(d, splits[1], ws)
        elif variant == 'wk':
            cfg = 27                                                        # 64x64 tile, two K groups, deep prefetch
        ops.conv2d_launch(d, cfg, 2)
        torch.cuda.synchronize()
        got = img.view(torch.bfloat16)
        if variant == 'plain':
            assert torch.equal(y2, y)
            assert torch.equal(got, want), variant
        elif variant == 'image_only':
            assert torch.isnan(y2).all() and torch.equal(got, want)
        else:                                                               # another summation order: compare the values
            back = got.view(-1, Cmid // 32, 2, 32).float().sum(2).reshape(N, Ho, Wo, Cmid)
            assert (back - yr).abs().max() < 2e-4 * max(1.0, yr.abs().max().item()), variant
            continue
        z = torch.empty_like(z_ref)
        dc = ops.make_conv_desc(y, wp2, 96, 3, 3, 1, 1, z, None, None, None, False, False)
        dc.inp, dc.in_lp = ptr(img), 1
        for ccfg in (3, 10, 27, 36):
            z.zero_()
            ops.conv2d_launch(dc, ccfg, 2)
            zr = torch.empty_like(z_ref)
            dr = ops.make_conv_desc(y, wp2, 96, 3, 3, 1, 1, zr, None, None, None, relu, False)
            ops.conv2d_launch(dr, ccfg, 2)
            torch.cuda.synchronize()
            assert torch.equal(z, zr), (variant, ccfg)
    # refused: ReLU on an image input, an image from the f32 / bf16 entry points
    dbad = ops.make_conv_desc(y, wp2, 96, 3, 3, 1, 1, z_ref, None, None, None, True, False)
    dbad.in_lp = 1
    with pytest.raises(RuntimeError):
        ops.conv2d_launch(dbad, 3, 2)
    dbad.relu_in = 0
    with pytest.raises(RuntimeError):
        ops.conv2d_launch(dbad, 3, 0)


def test_streamk_hand_off_is_reproducible_under_load(gpu):
    """conv_streamk_kernel finishes cut tiles inside the launch (write-through partials, arrival counter, the last arriver adds
    the segments in K order).  Repeated launches next to a second stream that keeps the chip busy must give the SAME bits every
    time (whichever wave arrives last), agree with the LDS-tiled kernel, and leave the counters at rest."""
    from vfloodnet_amd import ops
    g = torch.Generator().manual_seed(5)
    cases = [(2, 30, 54, 256, 256, 3, 1), (1, 60, 108, 128, 128, 3, 1), (2, 30, 54, 1024, 256, 1, 1), (1, 33, 47, 64, 96, 3, 1)]
    sk_cfgs = [c for c in range(len(ops.conv_cfg_tiles())) if ops.conv_cfg_kind(c) == 2]
    assert len(sk_cfgs) >= 4
    side = torch.cuda.Stream(device=gpu)
    big_x = torch.randn(2, 120, 216, 256, generator=g).to(gpu)
    big_w = ops.pad_rows(torch.randn(256, 9 * 256, generator=g) * 0.02).to(gpu)
    for (N, H, W, Cin, Cout, k, s) in cases:
        x = torch.randn(N, H, W, Cin, generator=g).to(gpu)
        wp = ops.pad_rows(torch.randn(Cout, k * k * Cin, generator=g) / (Cin * k * k) ** 0.5).to(gpu)
        res = torch.randn(N, (H + 2 * (k // 2) - k) // s + 1, (W + 2 * (k // 2) - k) // s + 1, Cout, generator=g).to(gpu)
        ref = ops.conv2d_nhwc(x, wp, Cout, k, k, s, k // 2, None, None, res, True, True, cfg=3)
        ws, cnt = ops.streamk_scratch(gpu)
        for cfg in sk_cfgs:
            first = None
            for it in range(12):
                if it % 3 == 0:
                    with torch.cuda.stream(side):                      # uneven load beside the hand-offs
                        ops.conv2d_nhwc(big_x, big_w, 256, 3, 3, 1, 1, cfg=9)
                y = ops.conv2d_nhwc(x, wp, Cout, k, k, s, k // 2, None, None, res, True, True, cfg=cfg)
                if first is None:
                    first = y.clone()
                    err = (y - ref).abs().max().item()
                    assert err < 2e-4 * max(1.0, ref.abs().max().item()), (cfg, err)
                else:
                    assert torch.equal(y, first), f'cfg {cfg}: launch {it} differs from launch 0'
            torch.cuda.synchronize()
            assert int(cnt.abs().sum()) == 0, 'arrival counters must return to rest'


@pytest.mark.parametrize('case', [(2, 12, 20, 64, 64, True, True, True), (1, 13, 19, 128, 96, False, False, True), (2, 30, 54, 256, 256, True, False, True),
                                  (1, 33, 47, 64, 256, False, True, False), (2, 9, 14, 32, 32, True, False, True)])
def test_winograd_f4x4_matches_torch_cpu(gpu, case):
    """Winograd F(4x4, 3x3) around the matrix kernels (input transform -> 36 batched-filter GEMMs -> output transform + epilogue)
    against F.conv2d on the CPU, at the tolerance of every other configuration of the convolution; image sizes that are not
    multiples of 4, every epilogue piece, and three kernel families for the GEMMs (LDS-tiled, wave-autonomous, stream-K)."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout, relu_in, relu_out, use_res = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    scale = 1 + 0.1 * torch.randn(Cout, generator=g)
    shift = 0.1 * torch.randn(Cout, generator=g)
    xin = F.relu(x) if relu_in else x
    ref = F.conv2d(xin.double(), w.double(), padding=1) * scale.double().view(1, -1, 1, 1) + shift.double().view(1, -1, 1, 1)
    res = torch.randn(ref.shape, generator=g) if use_res else None
    if use_res:
        ref = ref + res.double()
    if relu_out:
        ref = F.relu(ref)
    xd = x.permute(0, 2, 3, 1).contiguous().to(gpu)
    resd = res.permute(0, 2, 3, 1).contiguous().to(gpu) if use_res else None
    sc, sh = scale.to(gpu), shift.to(gpu)
    tol = 2e-4 * max(1.0, ref.abs().max().item())
    base = None
    for cfg in (2, 3, 42, 56) + tuple(ops.wino_gemm_cfg(tc, wgs) for tc, wgs in ((0, 512), (1, 256), (2, 768), (3, 512), (5, 512), (7, 256))):
        # (from 1000 on: the PERSISTENT transform-domain GEMM of round 5, vfn_winograd_gemm_f32 -- every tile shape, both request depths)
        if cfg >= ops.WINO_GEMM_CFG0 and Cout < 128 and ops.WINO_GEMM_TILES[(cfg - ops.WINO_GEMM_CFG0) & 3][1] > 64:
            continue
        y = ops.conv2d_winograd(xd, w, sc, sh, resd, relu_in, relu_out, cfg=cfg)
        torch.cuda.synchronize()
        err = (y.permute(0, 3, 1, 2).cpu().double() - ref).abs().max().item()
        assert err < tol, (cfg, err, tol)
        if cfg == 3:
            base = y.clone()
        elif cfg >= ops.WINO_GEMM_CFG0:
            # the same products in the same order as the un-split LDS-tiled launch: bit-identical, whatever the tile shape
            assert torch.equal(y, base), (cfg, (y - base).abs().max().item())


def test_winograd_persistent_gemm_is_bit_identical_to_the_batched_launch(gpu):
    """vfn_winograd_gemm_f32 (a workgroup walks a list of (component, row tile, filter tile) units as ONE K loop) against the batched-filter
    launch of the convolution kernel on the C2 frame's shapes incl. KeyValue's 1024 -> 640 and a 128-channel bottleneck: bit-identical
    for every tile shape / request depth / workgroup count, ragged unit counts (units not a multiple of the grid) included."""
    from vfloodnet_amd import ops
    g = torch.Generator(device=gpu).manual_seed(11)
    for (ntile, C, Cout) in [(810, 256, 256), (224, 1024, 640), (405, 128, 128), (300, 64, 192)]:
        rows = (ntile + 255) // 256 * 256
        cp = (Cout + 255) // 256 * 256
        V = torch.randn(36 * rows, C, device=gpu, generator=g)
        U = torch.randn(36 * cp, C, device=gpu, generator=g) * 0.05
        ref = torch.empty(36 * rows, Cout, device=gpu)
        ops.conv2d_launch(ops.make_winograd_gemm_desc(V, U, ref, rows, C, Cout), 3, 0)
        for tc in range(8):
            for wgs in (128, 512, 640):
                out = torch.full((36 * rows, Cout), float('nan'), device=gpu)
                ops.conv2d_launch(ops.make_winograd_gemm_desc(V, U, out, rows, C, Cout), ops.wino_gemm_cfg(tc, wgs), 0)
                torch.cuda.synchronize()
                assert torch.equal(out, ref), (ntile, C, Cout, tc, wgs)
    with pytest.raises(RuntimeError):                      # rows per component must be a multiple of the tile height
        ops.winograd_gemm(V[:36 * 192], U, out[:36 * 192], 192, 64, 192, cfg=0)


@pytest.mark.parametrize('case', [(2, 30, 54, 256, 64, False, True, True, 0), (1, 37, 41, 64, 256, False, True, True, 0), (2, 24, 40, 128, 96, True, False, False, 0),
                                  (3, 16, 20, 512, 256, False, True, True, 320), (1, 9, 7, 32, 20, True, True, False, 0)])
def test_persistent_1x1_convolution_matches_the_tiled_kernel(gpu, case):
    """vfn_conv1x1_persistent_f32 (round 5: the trunk's thin-K 1x1 layers as one persistent GEMM with the epilogue applied from the
    accumulator registers) against the LDS-tiled kernel on the same descriptor -- the same products in the same order, so the
    results agree to the last bit of the epilogue's fused multiply-add -- and against F.conv2d in float64: ragged M, a filter count
    that is no multiple of the tile, ReLU on the input / output, a residual and a residual shared by the images of the batch."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout, relu_in, relu_out, use_res, res_mod = case
    g = torch.Generator().manual_seed(hash(case) & 0xFFFF)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, Cin, generator=g) / Cin ** 0.5
    scale, shift = 1 + 0.1 * torch.randn(Cout, generator=g), 0.1 * torch.randn(Cout, generator=g)
    M = N * H * W
    res = torch.randn(res_mod if res_mod else M, Cout, generator=g) if use_res else None
    xin = F.relu(x) if relu_in else x
    ref = xin.double().reshape(M, Cin) @ w.double().t() * scale.double() + shift.double()
    if use_res:
        ref = ref + (res.double()[torch.arange(M) % res_mod] if res_mod else res.double())
    if relu_out:
        ref = F.relu(ref)
    xd, wp = x.to(gpu), ops.pad_rows(w.to(gpu))
    sc, sh = scale.to(gpu), shift.to(gpu)
    resd = res.to(gpu) if use_res else None

    def run(cfg):
        out = torch.full((N, H, W, Cout), float('nan'), device=gpu)
        d = ops.make_conv_desc(xd, wp, Cout, 1, 1, 1, 0, out, sc, sh, resd, relu_in, relu_out)
        d.res_mod = res_mod
        ops.conv2d_launch(d, cfg, 0)
        torch.cuda.synchronize()
        return out.reshape(M, Cout)
    base = run(3 if Cout >= 64 else 5)
    tol = 2e-4 * max(1.0, ref.abs().max().item())
    assert (base.cpu().double() - ref).abs().max().item() < tol
    for tc in range(8):
        if ops.WINO_GEMM_TILES[tc & 3][1] > 64 and Cout < 64:
            continue
        for wgs in (128, 512):
            y = run(ops.pconv_cfg(tc, wgs))
            assert not torch.isnan(y).any(), (tc, wgs)
            assert (y.cpu().double() - ref).abs().max().item() < tol, (tc, wgs)
            assert (y - base).abs().max().item() <= 2e-6 * max(1.0, base.abs().max().item()), (tc, wgs, (y - base).abs().max().item())
    # what the kernel does not implement is refused, not mis-computed
    d = ops.make_conv_desc(xd, ops.pad_rows(torch.randn(Cout, 9 * Cin, device=gpu)), Cout, 3, 3, 1, 1, torch.empty(N, H, W, Cout, device=gpu), sc, sh, None, False, False)
    with pytest.raises(RuntimeError):
        ops.conv2d_launch(d, ops.pconv_cfg(3, 512), 0)


def test_winograd_layers_of_the_plain_bf16_mode(gpu):
    """Round 5: in the plain-bf16 mode (BASELINE configs C3 / C5) a Winograd layer writes V as bf16 from the input transform and multiplies
    it with bf16 filter banks in the persistent GEMM (f32 accumulate).  Pieces against what they claim: V is exactly the f32 transform
    rounded once (RNE); the GEMM equals the float64 product of exactly those bf16 operands up to the f32 summation order; and the whole
    layer stays within bf16's operand resolution of the float64 convolution."""
    from vfloodnet_amd import ops
    g = torch.Generator().manual_seed(5)
    N, H, W, Cin, Cout = 2, 30, 54, 256, 192
    x = torch.randn(N, H, W, Cin, generator=g).to(gpu)
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5)
    rows = ops.winograd_rows(N, H, W)
    Vf = torch.zeros(36 * rows, Cin, device=gpu)
    Vh = torch.zeros(36 * rows, Cin, device=gpu, dtype=torch.bfloat16)
    ops.winograd_input(x, Vf, rows, True)
    ops.winograd_input(x, Vh, rows, True)
    torch.cuda.synchronize()
    assert torch.equal(Vh, Vf.to(torch.bfloat16))
    U = ops.pack_winograd_weight_bf16(w).to(gpu)
    cp = U.shape[0] // 36
    ref = torch.einsum('xrc,xoc->xro', Vh.double().view(36, rows, Cin), U.double().view(36, cp, Cin)[:, :Cout]).reshape(36 * rows, Cout)
    for tc in range(8):
        for wgs in (256, 512):
            Mb = torch.full((36 * rows, Cout), float('nan'), device=gpu)
            ops.conv2d_launch(ops.make_winograd_gemm_desc(Vh, U, Mb, rows, Cin, Cout), ops.wino_gemm_cfg(tc, wgs), 1)
            torch.cuda.synchronize()
            err = (Mb.double() - ref).abs().max().item()
            assert err < 2e-4 * ref.abs().max().item(), (tc, wgs, err)
    out = torch.empty(N, H, W, Cout, device=gpu)
    ops.winograd_output(Mb, rows, out, N, H, W, Cout, None, None, None, 0, 0, False)
    full = torch.nn.functional.conv2d(torch.relu(x).permute(0, 3, 1, 2).double().cpu(), w.double(), padding=1).permute(0, 2, 3, 1)
    diff = (out.cpu().double() - full).abs()
    rel, rms = diff.max().item() / full.abs().max().item(), (diff.pow(2).mean().sqrt() / full.pow(2).mean().sqrt()).item()
    # 8-bit operands THROUGH the transforms: the inverse transform amplifies the operands' 2^-9 rounding by an order of magnitude -- worst
    # element ~5 % of the largest output, r.m.s. ~1 % (the direct bf16 kernel: ~0.3 %).  Asserted at what it is; what it means for the masks is
    # measured on trained weights (tests/test_configs_gpu.py, profiles/r05_bf16_trained_margins.json: min mIoU 0.9996 with and without it)
    print(f'bf16 Winograd layer vs float64: max {rel:.4f} of the largest output, r.m.s. {rms:.4f}')
    assert rel < 0.1 and rms < 0.03, (rel, rms)
