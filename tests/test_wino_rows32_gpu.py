"""32-row tiles of the persistent transform-domain GEMM (csrc/conv_winograd.hip: wino_gemm_kernel<32, 128, 1, 4, PD>, <32, 64, 1, 2, PD>;
configuration ids from ops.WINO_GEMM32_CFG0): an F(6x6, 3x3) layer whose rows are padded to 32 equals the same layer on 64-padded rows
through a 64-row tile bit for bit -- the same k-order, one fmaf chain per element -- and the ids keep their meaning."""
import itertools
import json

import pytest
import torch

from golden_util import load, state_dict, t, close_logits

# (N, H, W) -> F(6x6) tiles: 90 (the 1/16-resolution map of two 480x854 images: rows 96 / 128), 65 (ragged edges both ways: 96 / 128),
# 97 (128 either way: a 32-row tile and a 64-row tile on the same rows), 33 (64 either way)
GEOMS = {90: (2, 30, 54), 65: (1, 27, 75), 97: (1, 6, 580), 33: (1, 16, 64)}
CHANNELS = list(itertools.product((32, 96), (48, 160)))                   # (Cin, Cout)


def test_geometries():
    from vfloodnet_amd import ops
    assert {k: ops.winograd6_tiles(*g) for k, g in GEOMS.items()} == {k: k for k in GEOMS}
    assert {k: ops.winograd6_rows(*g) for k, g in GEOMS.items()} == {90: 128, 65: 128, 97: 128, 33: 64}


def _layer(gpu, x, U, w_cout, rows, cfg, scale, shift, res):
    """input transform -> GEMMs -> output transform on buffers of exactly ``rows`` rows per component, NaN before the launches."""
    from vfloodnet_amd import ops
    N, H, W, cin = x.shape
    V = torch.full((64 * rows, cin), float('nan'), device=gpu)
    Mb = torch.full((64 * rows, w_cout), float('nan'), device=gpu)
    out = torch.full((N, H, W, w_cout), float('nan'), device=gpu)
    ops.winograd_input(x, V, rows, True, tile=6)
    d = ops.make_winograd_gemm_desc(V, U, Mb, rows, cin, w_cout, 64)
    ops.conv2d_launch(d, cfg, 0)
    ops.winograd_output(Mb, rows, out, N, H, W, w_cout, scale, shift, res, w_cout, 0, True, tile=6)
    torch.cuda.synchronize()
    return out, Mb.view(64, rows, w_cout)


@pytest.mark.gpu
@pytest.mark.parametrize('tiles', sorted(GEOMS))
def test_layer_through_32_row_tiles_equals_64_row_tiles(gpu, tiles):
    from vfloodnet_amd import ops
    N, H, W = GEOMS[tiles]
    rows32, rows64 = (tiles + 31) // 32 * 32, ops.winograd6_rows(N, H, W)
    n = 0
    for cin, cout in CHANNELS:
        g = torch.Generator().manual_seed(3200 + tiles + cin + cout)
        x = torch.randn(N, H, W, cin, generator=g).to(gpu)
        w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
        scale, shift = (1 + 0.1 * torch.randn(cout, generator=g)).to(gpu), (0.1 * torch.randn(cout, generator=g)).to(gpu)
        res = torch.randn(N, H, W, cout, generator=g).to(gpu)
        U = ops.pack_winograd6_weight(w).to(gpu)
        base, Mb64 = _layer(gpu, x, U, cout, rows64, ops.wino_gemm_cfg(3, 512), scale, shift, res)
        assert not torch.isnan(base).any() and not torch.isnan(Mb64[:, :tiles]).any()
        cfgs = [c for c in ops.wino_gemm_cfg_options(rows32, cout) if ops.is_wino_gemm32_cfg(c)]
        assert len(cfgs) == (12 if cout >= 128 else 6)
        for cfg in cfgs:
            y, Mb32 = _layer(gpu, x, U, cout, rows32, cfg, scale, shift, res)
            assert torch.equal(Mb32[:, :tiles], Mb64[:, :tiles]), (tiles, cin, cout, cfg)
            assert bool((Mb32[:, tiles:] == 0).all()), (tiles, cin, cout, cfg)            # (pad rows: zero operands)
            assert torch.equal(y, base), (tiles, cin, cout, cfg)
            n += 1
        # the wide tile on a filter count below its width: the entry point runs it (cout_pad covers the tile), the options never offer it
        if cout < 128:
            y, _ = _layer(gpu, x, U, cout, rows32, ops.wino_gemm32_cfg(4, 256), scale, shift, res)
            assert torch.equal(y, base)
    assert n == 2 * (12 + 6)


@pytest.mark.gpu
def test_rows_that_no_32_row_tile_divides_are_refused(gpu):
    from vfloodnet_amd import ops
    V, U, Mb = torch.zeros(64 * 48, 32, device=gpu), torch.zeros(64 * 256, 32, device=gpu), torch.zeros(64 * 48, 64, device=gpu)
    with pytest.raises(RuntimeError):
        ops.winograd_gemm(V, U, Mb, 48, 32, 64, cfg=8, comps=64)
    for bad in (10, 11, 14, 15, 16):                        # tile indices 2 and 3 of the 32-row range do not exist
        with pytest.raises(RuntimeError):
            ops.winograd_gemm(V, U, Mb, 32, 32, 64, cfg=bad, comps=64)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=gpu, dtype=dt)
    d = ops.make_winograd_gemm_desc(z(36 * 64, 64, dt=torch.bfloat16), z(36 * 256, 64, dt=torch.bfloat16), z(36 * 64, 64), 64, 64, 64, 36)
    with pytest.raises(RuntimeError):
        ops.conv2d_launch(d, ops.wino_gemm32_cfg(1, 256), 1)          # the bf16 form has no 32-row tile


@pytest.mark.gpu
def test_plan_with_32_row_padding_equals_the_64_row_plan(gpu, monkeypatch):
    """The 96x160 sample with every F(6x6) layer whose rows shrink on 32-padded rows (VFN_WINO_ROWS32=2: the 1/16 and 1/8 maps, 4 and 16
    tiles -> 32 rows instead of 64, sharing one V buffer with the 1/4 maps' 64 rows) and with none (=0): the same logits bit for bit,
    and tests/test_golden_gpu.py::test_blocks' tolerance."""
    from vfloodnet_amd import AFB_URR, FeatureBank, engine as E, ops
    monkeypatch.setattr(E, '_WINOGRAD', '2')
    monkeypatch.setattr(E, '_WINOGRAD_F6', '2')
    scores, n32 = {}, {}
    for switch in ('0', '2'):
        monkeypatch.setattr(E, '_WINO_ROWS32', switch)
        model = AFB_URR(gpu, update_bank=True).to(gpu).eval()
        model.load_state_dict(state_dict(), strict=True)
        g = load('blocks_96x160.npz')
        frames, m0 = t(g['frames']).to(gpu), t(g['mask'])
        oh = torch.stack([1 - m0, m0], 0).unsqueeze(0).to(gpu)
        k, v = model.memorize(frames[0:1], oh)
        fb = FeatureBank(2, 250000, gpu)
        fb.init_bank(k, v)
        score, _ = model.segment(frames[1:2], fb)
        ok, dl, dp = close_logits(score.cpu(), t(g['score']), 1e-3)
        assert ok, (switch, dl, dp)
        scores[switch] = score.clone()
        plan = model.engine().last_query[0]
        n32[switch] = sum(1 for lst in plan.all_lists() for l in lst if l.fn is ops.conv2d_launch and ops.is_wino_gemm32_cfg(l.args[1]))
    assert n32['0'] == 0 and n32['2'] >= 10, n32
    assert torch.equal(scores['0'], scores['2'])


def test_ids():
    """Existing ids name what tests/test_host_logic.py says; the new range decodes to the 32-row tiles; a 32-row tile is offered only
    for rows that are a multiple of 32, never to the heuristics; no shipped table names one for a shape whose rows are not."""
    from vfloodnet_amd import engine, ops
    assert ops.pconv_cfg(5, 512) == 2000 + 5 + 8 * 4 and ops.conv_cfg_name(ops.pconv_cfg(5, 512)) == 'wino_gemm_kernel<64, 128, 2, 4, 2, true, false>'
    assert ops.conv_cfg_name(ops.wino_gemm_cfg(2, 768), 1) == 'wino_gemm_kernel<128, 64, 4, 2, 1, false, true>'
    assert [ops.conv_cfg_name(ops.wino_gemm_cfg(tc, 256)) for tc in (0, 1, 7)] == [
        'wino_gemm_kernel<128, 128, 4, 2, 1, false, false>', 'wino_gemm_kernel<64, 128, 2, 4, 1, false, false>', 'wino_gemm_kernel<64, 64, 2, 2, 2, false, false>']
    assert ops.WINO_GEMM_CFG0 + 7 + 8 * 6 < ops.WINO_GEMM32_CFG0 and ops.WINO_GEMM32_CFG0 + 7 + 8 * 6 < ops.PCONV_CFG0
    assert ops.conv_cfg_name(ops.wino_gemm32_cfg(0, 512)) == 'wino_gemm_kernel<32, 128, 1, 4, 1, false, false>'
    assert ops.conv_cfg_name(ops.wino_gemm32_cfg(5, 768)) == 'wino_gemm_kernel<32, 64, 1, 2, 2, false, false>'
    assert ops.persistent_cfg_info(ops.wino_gemm32_cfg(4, 768)) == (32, 128, 1, 4, 2, 768)
    assert ops.persistent_cfg_info(1051) == (64, 64, 2, 2, 1, 768) and ops.persistent_cfg_info(2037) == (64, 128, 2, 4, 2, 512)
    assert not ops.is_wino_gemm32_cfg(1055) and not ops.is_wino_gemm32_cfg(2000) and ops.is_wino_gemm32_cfg(1500)
    for rows in (16, 32, 48, 64, 90, 96, 100, 128, 160, 256):
        opts = ops.wino_gemm_cfg_options(rows, 256)
        assert any(ops.is_wino_gemm32_cfg(c) for c in opts) == (rows % 32 == 0), rows
        assert all(rows % ops.persistent_cfg_info(c)[0] == 0 for c in opts), rows
        assert not any(ops.is_wino_gemm32_cfg(c) for c in ops.wino_gemm_cfg_options(rows, 256, rows32=False))
    assert not any(ops.persistent_cfg_info(c)[1] > 64 for c in ops.wino_gemm_cfg_options(96, 48))
    for path in engine._TABLE_PATHS:
        for k, v in json.load(open(path)).items():
            assert not any(ops.is_wino_gemm32_cfg(c) for c in v[0::3]), (path, k, v)
    for k, v in json.load(open(engine._TUNED_WINO6_PATH)).items():
        M = int(k.split(',')[0])
        assert M % 64 == 0 and len(v) == 3 and v[0] >= ops.WINO_GEMM_CFG0 and v[0] < ops.PCONV_CFG0, (k, v)
        assert (M // 64) % ops.persistent_cfg_info(v[0])[0] == 0, (k, v)
        if ops.is_wino_gemm32_cfg(v[0]):
            assert (M // 64) % 32 == 0 and (M // 64) % 64 != 0, (k, v)        # (a shape of 64-padded rows keeps a 64- or 128-row tile)
