"""The implicit-GEMM convolution one tile configuration at a time against float64 (tests/conv_ref.py): all 62 configurations behind
vfn_conv2d_nhwc_f32 / _bf16 / _bf16x3 -- conv_igemm_kernel, conv_igemm_wk_kernel, conv_igemm_dma_kernel, conv_direct_kernel,
conv_streamk_kernel, splitk_reduce_kernel and the in-launch finishes -- driven through the descriptors on tensors this file lays
out itself: every tensor a channel slice of a wider allocation with guard rows, gutters poisoned (NaN, or +1e30 under a ReLU), the
output allocation, the split-K slabs and their tail NaN before every launch.  After every launch: every output element within
8 x the float32 error of the reference itself (never wider than 2e-5 of max|ref|), every byte around the output unchanged, the
arrival counters at rest.

Measured on an MI355X (CONVMARGIN lines; errors in units of max|ref|, worst over the launches of the row):

    path           family    launches   ratio      bound      worst err  err / bound
    f32 unsplit    igemm       1672     4.60e-07   3.68e-06   5.52e-07   0.150
    f32 unsplit    wk          1056     3.56e-07   2.85e-06   4.66e-07   0.164
    f32 unsplit    dma          616     4.60e-07   3.68e-06   5.52e-07   0.150
    f32 unsplit    direct      1584     4.60e-07   3.68e-06   6.45e-07   0.176
    f32 unsplit    streamk      616     1.82e-07   1.46e-06   2.17e-07   0.149
    split-K        igemm       1175     3.56e-07   2.85e-06   4.66e-07   0.164
    split-K        dma          535     3.56e-07   2.85e-06   4.66e-07   0.164
    split-K        direct       600     2.68e-07   2.14e-06   2.16e-07   0.101
    k_rot          igemm        490     5.82e-07   4.65e-06   7.39e-07   0.159
    k_rot          wk           288     5.07e-07   4.06e-06   5.44e-07   0.134
    k_rot          dma          210     5.07e-07   4.06e-06   5.44e-07   0.134
    w_batch_rows   igemm         76     3.46e-07   2.77e-06   2.48e-07   0.090
    w_batch_rows   wk            48     3.46e-07   2.77e-06   2.48e-07   0.090
    w_batch_rows   dma           28     3.46e-07   2.77e-06   2.48e-07   0.090
    w_batch_rows   direct        72     1.58e-07   1.26e-06   1.80e-07   0.142
    w_batch_rows   streamk       28     1.58e-07   1.26e-06   1.80e-07   0.142
    bf16           igemm        269     2.00e-07   1.60e-06   2.17e-07   0.136
    bf16           wk           180     2.00e-07   1.60e-06   2.17e-07   0.136
    bf16x3         igemm        411     2.35e-07   1.88e-06   1.84e-07   0.098
    bf16x3         wk           288     2.35e-07   1.88e-06   1.84e-07   0.098
    bf16x3 out_lp  igemm+wk       3     7.58e-07   6.06e-06   3.43e-07   0.057
    NaN input      igemm        438     1.53e-07   1.23e-06   2.06e-07   0.168
    NaN input      wk           216     1.53e-07   1.23e-06   2.06e-07   0.168
    NaN input      dma          192     1.53e-07   1.23e-06   2.06e-07   0.168
    NaN input      direct       396     3.12e-07   2.50e-06   4.09e-07   0.164
    NaN input      streamk      126     1.53e-07   1.23e-06   1.14e-07   0.093
    copies (bits)  igemm        684     1.53e-07   1.23e-06   2.06e-07   0.168
    copies (bits)  wk           432     1.53e-07   1.23e-06   2.06e-07   0.168
    copies (bits)  dma          252     1.53e-07   1.23e-06   2.06e-07   0.168
    copies (bits)  direct       648     3.12e-07   2.50e-06   4.09e-07   0.164
    copies (bits)  streamk      216     1.53e-07   1.23e-06   1.14e-07   0.093

(igemm = conv_igemm_kernel, wk = conv_igemm_wk_kernel, dma = conv_igemm_dma_kernel, direct = conv_direct_kernel, streamk =
conv_streamk_kernel; the split-K rows include splitk_reduce_kernel and the in-launch finish.  The row shown is the launch closest to
its bound; ratios over all cases run from 6.0e-8, the floor of one float32 rounding, to 1.06e-6.  The NaN rows include the
'mask_relu' launches, which take the pointer form of the wide epilogue with relu_out on.)

Wall time of the file on an MI355X: 5.5 s for the 29 tests, about 14 500 checked launches."""
import ctypes as C
import functools

import pytest
import torch

import conv_ref
from conv_ref import GEOMS, GUARD, NAN, STRIDES

pytestmark = pytest.mark.gpu

OK, ERR_ARG = 0, 1
FN = ('vfn_conv2d_nhwc_f32', 'vfn_conv2d_nhwc_bf16', 'vfn_conv2d_nhwc_bf16x3')
ONE_BY_ONE = [g for g in GEOMS if g[5] == 1]
SPLIT_GEOMS = [GEOMS[2], GEOMS[5], GEOMS[7]]
NAN_AT = {GEOMS[2]: (1, 2, 3, 17), GEOMS[7]: (0, 4, 4, 40), GEOMS[9]: (0, 20, 25, 100)}


def _cdiv(a, b):
    return (a + b - 1) // b


def _gname(geom):
    return 'x'.join(str(v) for v in geom)


def _launch(d, cfg, mode=0):
    from vfloodnet_amd import _lib
    return getattr(_lib.lib(), FN[mode])(C.byref(d), int(cfg), _lib.stream())


@functools.lru_cache(maxsize=None)
def _families():
    """Kernel family of every configuration id, from the instantiation names."""
    from vfloodnet_amd import ops
    out = []
    for name in ops.conv_cfg_names():
        out.append('wk' if name.startswith('conv_igemm_wk') else 'dma' if name.startswith('conv_igemm_dma') else
                   'igemm' if name.startswith('conv_igemm_kernel') else 'direct' if name.startswith('conv_direct') else 'streamk')
        assert out[-1] != 'streamk' or name.startswith('conv_streamk'), name
    assert len(out) == 62
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _splitk_cfgs():
    """One register-staged, one LDS-DMA and one wave-autonomous configuration per tile height (the narrowest tile of that height, so
    that Cout = 64 is a whole number of filter tiles wherever a configuration allows it)."""
    from vfloodnet_amd import ops
    tiles, fam, pick = ops.conv_cfg_tiles(), _families(), {}
    for cfg, (bm, bn) in enumerate(tiles):
        if fam[cfg] in ('igemm', 'dma', 'direct'):
            key = (fam[cfg], bm)
            if key not in pick or bn < tiles[pick[key]][1]:
                pick[key] = cfg
    assert sorted(pick) == [('direct', 32), ('direct', 64), ('direct', 128), ('direct', 256), ('dma', 64), ('dma', 128), ('dma', 256),
                            ('igemm', 32), ('igemm', 64), ('igemm', 128), ('igemm', 256)]
    return tuple(sorted(pick.values()))


def _pick(family, bm, bn, wk=None, tpb=None):
    """The first configuration id of a kernel family with that tile (and K groups / K tiles per barrier, where given)."""
    from vfloodnet_amd import ops
    for cfg, tile in enumerate(ops.conv_cfg_tiles()):
        if (_families()[cfg] == family and tile == (bm, bn) and (wk is None or ops.conv_cfg_wk(cfg) == wk) and
                (tpb is None or ops.conv_cfg_tpb(cfg) == tpb)):
            return cfg
    raise AssertionError(f'no {family} configuration with a {bm} x {bn} tile (wk {wk}, tpb {tpb})')


_wcache = {}


def _weights(gpu, case):
    from vfloodnet_amd import ops
    key = (case.geom, case.variant)
    if key not in _wcache:
        _wcache[key] = ops.pad_rows(case.wp).to(gpu)
    return _wcache[key]


class Run:
    """One case on the device in one stride set (conv_ref.Layout) and the descriptor that points at it."""

    def __init__(self, gpu, case, strides):
        self.case, self.gpu = case, gpu
        self.L = conv_ref.Layout(case, strides, gpu)
        self.wp = _weights(gpu, case)

    def desc(self):
        from vfloodnet_amd import ops
        from vfloodnet_amd._lib import ptr
        c, L, fl = self.case, self.L, self.case.flags
        N, H, W, Cin, Cout, k, s = c.geom
        d = ops.make_conv_desc(L.x, self.wp, Cout, k, k, s, k // 2, L.out, L.scale, L.shift, L.res, fl['relu_in'], fl['relu_out'],
                               cin=Cin, in_ld=L.in_ld, out_ld=L.out_ld, res_ld=L.res_ld, N=N, H=H, W=W)
        assert d.M == c.M and d.k_rot == 0
        d.res_mod = c.res_mod
        if L.mask is not None:
            d.mask, d.mask_ld, d.mask_after = ptr(L.mask), L.mask_ld, int(fl['mask_after'])
        return d


class Ledger:
    """Device-side results of many launches, read back once: (label, bound, error, flags that must be zero)."""

    def __init__(self):
        self.rows = []

    def add(self, label, case, err, *zero):
        z = torch.stack([t.double().reshape(()) for t in zero]).sum() if zero else torch.zeros((), dtype=torch.float64, device=err.device)
        self.rows.append((label, case.bound, case.ratio, err.reshape(()), z))

    def close(self, family, path, name):
        if not self.rows:
            return
        torch.cuda.synchronize()
        errs = torch.stack([r[3] for r in self.rows]).cpu().tolist()
        zero = torch.stack([r[4] for r in self.rows]).cpu().tolist()
        bad = [(r[0], f'err {e:.3e}', f'bound {r[1]:.3e}', f'flags {z:g}') for r, e, z in zip(self.rows, errs, zero) if not e < r[1] or z != 0]
        i = max(range(len(errs)), key=lambda j: errs[j] / self.rows[j][1] if errs[j] == errs[j] else float('inf'))
        print(f'CONVMARGIN {family} {path} {name} launches {len(errs)} ratio {self.rows[i][2]:.2e} bound {self.rows[i][1]:.2e} '
              f'err {errs[i]:.2e} ({errs[i] / self.rows[i][1]:.3f} of the bound)')
        self.rows = []
        assert not bad, (family, path, name, len(bad), bad[:6])


def _ledgers():
    return {f: Ledger() for f in ('igemm', 'wk', 'dma', 'direct', 'streamk')}


def _close(ledgers, path, name):
    for fam, lg in ledgers.items():
        lg.close(fam, path, name)


def _differs(a, b):
    return (conv_ref.bits(a) != conv_ref.bits(b)).any()


def _untouched(image):
    return (~torch.isnan(image)).any()


# ------------------------------------------------------------------------------------------------------------- tile counts
def test_geometries_reach_the_xcd_remap_and_the_stream_k_hand_off(gpu):
    """Every configuration of kind 0 and 1 has a launch with 16 or more whole tiles whose count is no multiple of 8 (the remap of
    workgroups to XCD runs: bijective for any count, and only such a count has runs of two lengths); at least one stream-K
    configuration has more (tile, K tile) units than waves, and not a multiple (waves with uq and uq + 1 units, tiles cut between
    waves).  W comes from the device's CU count."""
    from vfloodnet_amd import ops
    tiles = ops.conv_cfg_tiles()
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    qualifies = []
    for cfg, (bm, bn) in enumerate(tiles):
        counts = [_cdiv(conv_ref.make_case(g, 'none').M, bm) * _cdiv(g[4], bn) for g in GEOMS]
        if ops.conv_cfg_kind(cfg) < 2:
            assert any(t >= 16 and t % 8 for t in counts), (cfg, bm, bn, counts)
            continue
        wps = int(ops.conv_cfg_name(cfg).split(',')[-1])                    # "conv_streamk_kernel<TM, TN, waves per SIMD"
        W = cus * wps * 4
        units = [t * g[5] * g[5] * (g[3] // 32) for t, g in zip(counts, GEOMS)]
        qualifies += [(cfg, u, W) for u in units if u > W and u % W]
    assert qualifies, (cus, 'no stream-K launch with more units than waves')
    print(f'stream-K launches with U > W, U % W != 0: {qualifies}')


# ------------------------------------------------------------------------------------------------------------- f32, every id
@pytest.mark.parametrize('geom', GEOMS, ids=_gname)
def test_f32_every_configuration(gpu, geom):
    """All 62 ids x every epilogue variant that applies x both stride sets.  The f32 entry point refuses none of these launches: a
    refusal (or any other status) fails."""
    from vfloodnet_amd import ops
    fam = _families()
    ws, cnt = ops.streamk_scratch(gpu)
    for variant in conv_ref.VARIANTS:
        if not conv_ref.applies(geom, variant):
            continue
        case = conv_ref.make_case(geom, variant)
        for strides in sorted(STRIDES):
            R, led = Run(gpu, case, strides), _ledgers()
            for cfg in range(62):
                d = R.desc()
                if ops.conv_cfg_kind(cfg) == 2:
                    ops.set_streamk(d, ws, cnt)
                assert _launch(d, cfg) == OK, (cfg, variant, strides)
                err, dirty, _ = R.L.collect()
                led[fam[cfg]].add((cfg, variant, strides), case, err, dirty)
            led['streamk'].add(('counters', variant, strides), case, torch.zeros((), dtype=torch.float64, device=gpu), cnt.abs().sum())
            _close(led, f'{variant}/{strides}', _gname(geom))


# ------------------------------------------------------------------------------------------------------------- split-K
@pytest.mark.parametrize('geom', SPLIT_GEOMS, ids=_gname)
def test_split_k_every_slice_count_and_tail(gpu, geom):
    """Every ksplit from 2 to nk_all that check_desc accepts -- one-tile slices, shorter than the register prefetch, included --
    through the C entry point, cut from tile 0 and from every m-tile boundary (tail split), all five epilogue variants (the reduce
    kernel and the in-launch finish have their own copies of the epilogue): the separate reduce launch, and on the LDS-tiled
    configurations with whole filter tiles the in-launch finish, bit-equal to it.  A ksplit with an empty slice is refused."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout, k, s = geom
    tiles, fam = ops.conv_cfg_tiles(), _families()
    nk_all = k * k * (Cin // 32)
    cnt = torch.zeros(4096, dtype=torch.int32, device=gpu)
    finishes = 0
    for variant in conv_ref.VARIANTS:
        case = conv_ref.make_case(geom, variant)
        R, led = Run(gpu, case, 'wide'), _ledgers()
        P = torch.empty(nk_all * case.M * Cout + 64, device=gpu)
        for cfg in _splitk_cfgs():
            bm, bn = tiles[cfg]
            n_t, m_t = _cdiv(Cout, bn), _cdiv(case.M, bm)
            for ks in range(2, nk_all + 1):
                if _cdiv(nk_all, ks) * (ks - 1) >= nk_all:                       # an empty last slice
                    if variant == 'none':
                        d = ops.set_splitk(R.desc(), ks, P)
                        assert _launch(d, cfg) == ERR_ARG, (cfg, ks)
                        err, dirty, image = R.L.collect()
                        led[fam[cfg]].add((cfg, ks, 'refused'), case, torch.zeros_like(err), dirty, _untouched(image))
                    continue
                for full_m in range(m_t):
                    rows_ = case.M - full_m * bm
                    images = []
                    for counters in (None, cnt) if (fam[cfg] != 'direct' and Cout % bn == 0) else (None,):
                        P.fill_(NAN)
                        d = ops.set_splitk(R.desc(), ks, P, split_from=full_m * n_t, rows=rows_, counters=counters)
                        assert _launch(d, cfg) == OK, (cfg, ks, full_m, variant)
                        err, dirty, image = R.L.collect()
                        past = (~torch.isnan(P[ks * rows_ * Cout:])).any()       # nothing behind the slabs was written
                        led[fam[cfg]].add((cfg, ks, full_m, variant, 'finish' if counters is not None else 'reduce'), case, err, dirty, past)
                        images.append(image)
                    if len(images) == 2:
                        finishes += 1
                        led[fam[cfg]].add((cfg, ks, full_m, variant, 'finish != reduce'), case, torch.zeros_like(err), _differs(*images))
        led['igemm'].add(('counters', variant), case, torch.zeros((), dtype=torch.float64, device=gpu), cnt.abs().sum())
        _close(led, f'splitk/{variant}', _gname(geom))
    assert (finishes > 0) == (geom == GEOMS[7])


# ------------------------------------------------------------------------------------------------------------- k_rot
@pytest.mark.parametrize('geom', ONE_BY_ONE, ids=_gname)
def test_k_rotation(gpu, geom):
    """vfn_conv_desc.k_rot = 1 on the 1x1 geometries through every LDS-tiled configuration against float64, and with split-K on the
    register-staged 64 x 64 tile.  Where a workgroup has at most one K tile there is nothing to rotate: the bits of k_rot = 0, on
    the one-tile geometries and on the split whose slices are one tile each.  conv_igemm_dma_kernel does not read k_rot: its
    launches must give the bits of k_rot = 0 on every geometry."""
    from vfloodnet_amd import ops
    N, H, W, Cin, Cout, k, s = geom
    fam, nk_all = _families(), Cin // 32
    cfg64 = _pick('igemm', 64, 64)
    for variant in ('none', 'full'):
        case = conv_ref.make_case(geom, variant)
        R, led = Run(gpu, case, 'wide'), _ledgers()
        for cfg in range(62):
            if ops.conv_cfg_kind(cfg) != 0:
                continue
            images = []
            for rot in (0, 1):
                d = R.desc()
                d.k_rot = rot
                assert _launch(d, cfg) == OK, (cfg, rot)
                err, dirty, image = R.L.collect()
                led[fam[cfg]].add((cfg, variant, 'k_rot', rot), case, err, dirty)
                images.append(image)
            if nk_all == 1 or fam[cfg] == 'dma':
                led[fam[cfg]].add((cfg, variant, 'bits of k_rot = 0'), case, torch.zeros_like(err), _differs(*images))
        P = torch.empty(nk_all * case.M * Cout + 64, device=gpu)
        for ks in range(2, nk_all + 1):
            if _cdiv(nk_all, ks) * (ks - 1) >= nk_all:
                continue
            images = []
            for rot in (0, 1):
                P.fill_(NAN)
                d = ops.set_splitk(R.desc(), ks, P)
                d.k_rot = rot
                assert _launch(d, cfg64) == OK, (ks, rot)
                err, dirty, image = R.L.collect()
                led['igemm'].add((cfg64, variant, 'k_rot split', ks, rot), case, err, dirty, (~torch.isnan(P[ks * case.M * Cout:])).any())
                images.append(image)
            if ks == nk_all:
                led['igemm'].add((cfg64, variant, 'one-tile slices: bits of k_rot = 0'), case, torch.zeros_like(err), _differs(*images))
        _close(led, f'k_rot/{variant}', _gname(geom))


# ------------------------------------------------------------------------------------------------------------- batched filters
def test_batched_filters_every_configuration(gpu):
    """vfn_conv_desc.w_batch_rows: three banks with different filters, 256 rows each, Cin 64, Cout 40, against a float64 einsum per
    bank, through every configuration of the three kinds (all accept a 256-row bank: every tile height divides it)."""
    from vfloodnet_amd import ops
    fam = _families()
    ws, cnt = ops.streamk_scratch(gpu)
    for variant in ('none', 'full'):
        case = conv_ref.make_bank_case(variant=variant)
        wdev = torch.zeros(case.banks, 256, case.cin)
        wdev[:, :case.cout] = case.w
        wdev = wdev.reshape(-1, case.cin).to(gpu)
        for strides in sorted(STRIDES):
            L, led = conv_ref.Layout(case, strides, gpu), _ledgers()
            for cfg in range(62):
                d = _bank_desc(case, L, wdev)
                if ops.conv_cfg_kind(cfg) == 2:
                    ops.set_streamk(d, ws, cnt)
                assert _launch(d, cfg) == OK, (cfg, variant, strides)
                err, dirty, _ = L.collect()
                led[fam[cfg]].add((cfg, variant, strides), case, err, dirty)
            led['streamk'].add(('counters',), case, torch.zeros((), dtype=torch.float64, device=gpu), cnt.abs().sum())
            _close(led, f'w_batch_rows/{variant}/{strides}', f'{case.banks}x{case.rows_per_bank}x{case.cin}x{case.cout}')


def _bank_desc(case, L, wdev):
    from vfloodnet_amd import ops
    fl = case.flags
    d = ops.make_conv_desc(L.x, wdev, case.cout, 1, 1, 1, 0, L.out, L.scale, L.shift, L.res, fl['relu_in'], fl['relu_out'],
                           cin=case.cin, in_ld=L.in_ld, out_ld=L.out_ld, res_ld=L.res_ld, N=1, H=1, W=case.M)
    d.cout_pad, d.w_batch_rows = 256, case.rows_per_bank
    return d


# ------------------------------------------------------------------------------------------------------------- bf16, bf16x3
@pytest.mark.parametrize('mode', [1, 2])
def test_reduced_precision_every_configuration(gpu, mode):
    """bf16 and bf16x3 against the float64 evaluation of exactly the products they form: exactly 27 configurations accept the mode;
    each runs on every geometry its K tile divides (and refuses the others, and the entry point refuses the other 35 ids), variants
    'full' and 'resmod' on the 16-byte stride set and 'full' on the odd one, filters converted on the fly and on the host
    (w_packed): bit-equal.  Split-K on the 64 x 64 tile includes one-tile slices."""
    from vfloodnet_amd import ops
    fam, kt = _families(), 64 if mode == 1 else 32
    cfgs = ops.conv_cfgs(mode)
    assert len(cfgs) == 27
    cfg64 = _pick('igemm', 64, 64)
    ran = set()
    for geom in GEOMS:
        N, H, W, Cin, Cout, k, s = geom
        for variant in ('full', 'resmod'):
            if not conv_ref.applies(geom, variant):
                continue
            fits = Cin % kt == 0
            case = conv_ref.make_case(geom, variant, mode if fits else 0)
            for strides in ('wide', 'odd') if variant == 'full' else ('wide',):
                R, led = Run(gpu, case, strides), _ledgers()
                wlp = ops.pack_weights_lp(R.wp, mode) if fits else None
                for cfg in range(62):
                    if cfg in cfgs and fits:
                        d = R.desc()
                        assert _launch(d, cfg, mode) == OK, (cfg, geom, variant, strides)
                        err, dirty, image = R.L.collect()
                        d2 = ops.use_packed_weights(R.desc(), wlp)
                        assert _launch(d2, cfg, mode) == OK, (cfg, geom, variant, strides, 'packed')
                        err2, dirty2, image2 = R.L.collect()
                        led[fam[cfg]].add((cfg, variant, strides), case, torch.maximum(err, err2), dirty, dirty2, _differs(image, image2))
                        ran.add(cfg)
                    elif strides == 'wide' and variant == 'full':       # Cin no multiple of the K tile, or an id of another mode
                        assert _launch(R.desc(), cfg, mode) == ERR_ARG, (cfg, geom)
                        err, dirty, image = R.L.collect()
                        led[fam[cfg]].add((cfg, 'refused'), case, torch.zeros_like(err), dirty, _untouched(image))
                if fits and variant == 'full' and strides == 'wide' and geom in (GEOMS[2], GEOMS[7]):
                    nk_all = k * k * (Cin // kt)
                    P = torch.empty(nk_all * case.M * Cout + 64, device=gpu)
                    for ks in range(2, nk_all + 1):
                        if _cdiv(nk_all, ks) * (ks - 1) >= nk_all:
                            continue
                        P.fill_(NAN)
                        assert _launch(ops.set_splitk(R.desc(), ks, P), cfg64, mode) == OK, (geom, ks)
                        err, dirty, _ = R.L.collect()
                        led['igemm'].add((cfg64, 'split', ks), case, err, dirty, (~torch.isnan(P[ks * case.M * Cout:])).any())
                _close(led, f'mode{mode}/{variant}/{strides}', _gname(geom))
    assert ran == set(cfgs)


def test_bf16x3_image_output_with_a_gutter(gpu):
    """bf16x3 with vfn_conv_desc.out_lp at out_ld = Cout + 32: the image is exactly hi = bf16(y), lo = bf16(y - hi) of the f32
    result of the same launch, y is within the bound, and the gutter and guard bytes of the image's allocation are unchanged."""
    from vfloodnet_amd import ops
    from vfloodnet_amd._lib import ptr
    geom = GEOMS[7]
    Cout = geom[4]
    case = conv_ref.make_case(geom, 'resmod', 2)
    R, led = Run(gpu, case, 'wide'), Ledger()
    ld = Cout + 32
    for cfg in (_pick('igemm', 64, 64), _pick('wk', 64, 64, wk=2, tpb=1), _pick('wk', 64, 64, wk=1, tpb=2)):
        y_alloc = torch.full((case.M + 2 * GUARD, ld), NAN, device=gpu)
        img_alloc = torch.full((case.M + 2 * GUARD, ld), -777.0, device=gpu)
        y, img = y_alloc[GUARD:GUARD + case.M, :Cout], img_alloc[GUARD:GUARD + case.M, :Cout]
        d = R.desc()
        d.out, d.out_ld, d.out_lp, d.out_lp_relu = ptr(y), ld, ptr(img), 0
        assert _launch(d, cfg, 2) == OK, cfg
        yc = y.contiguous()
        hi = yc.bfloat16()
        lo = (yc - hi.float()).bfloat16()
        want = torch.cat([hi.view(-1, Cout // 32, 32), lo.view(-1, Cout // 32, 32)], dim=2).reshape(case.M, Cout * 2)
        wrong = (img.contiguous().view(torch.int16) != want.view(torch.int16)).any()
        err = (yc.double() - R.L.ref).abs().max() / case.maxref
        y.fill_(NAN)
        img.fill_(-777.0)
        dirty = (~torch.isnan(y_alloc)).any().double() + (img_alloc != -777.0).any().double()
        led.add((cfg, 'out_lp'), case, err, wrong, dirty)
    led.close('igemm+wk', 'mode2/out_lp', _gname(geom))


# ------------------------------------------------------------------------------------------------------------- refusals
def test_every_rule_refuses_before_anything_is_launched(gpu):
    """One descriptor per rule of check_desc and of the entry points, breaking only that rule: VFN_ERR_ARG and an untouched output
    allocation.  Every descriptor would still be a well-formed launch if its rule were missing (all reads and writes stay inside
    the allocations), so a lost rule fails the status assertion and nothing else."""
    from vfloodnet_amd import ops
    from vfloodnet_amd._lib import ptr
    fam, tiles = _families(), ops.conv_cfg_tiles()
    ws, sk_cnt = ops.streamk_scratch(gpu)
    cnt = torch.zeros(4096, dtype=torch.int32, device=gpu)
    direct64, c64, c128, cwk = _pick('direct', 64, 64), _pick('igemm', 64, 64), _pick('igemm', 128, 128), _pick('wk', 64, 64, wk=2)
    sk = next(c for c in range(62) if fam[c] == 'streamk')
    base = Run(gpu, conv_ref.make_case(GEOMS[7], 'none'), 'wide')          # 2 x 8 x 8, 64 -> 64, 3x3: 18 K tiles, M = 128
    masked = Run(gpu, conv_ref.make_case(GEOMS[7], 'mask'), 'wide')
    wide = Run(gpu, conv_ref.make_case(GEOMS[5], 'none'), 'wide')          # Cout = 136: three 64-filter tiles
    one = Run(gpu, conv_ref.make_case(GEOMS[0], 'none'), 'wide')           # one unit: stream-K touches neither workspace nor counters
    bank_case = conv_ref.make_bank_case(variant='none')
    bankL = conv_ref.Layout(bank_case, 'wide', gpu)
    wbank = torch.zeros(bank_case.banks * 256, bank_case.cin, device=gpu)
    P = torch.full((18 * 2 * 128 * 136,), NAN, device=gpu)
    M, Cin = base.case.M, GEOMS[7][3]
    x96 = torch.zeros(M + 2 * GUARD, 96, device=gpu)                        # an input whose pixel stride the image form accepts

    def set_(d, **kw):
        for k_, v in kw.items():
            setattr(d, k_, v)
        return d

    def lp_relu():
        d = set_(base.desc(), inp=ptr(x96[GUARD:]), in_ld=96, in_lp=1, relu_in=1)
        return d
    n_t = _cdiv(136, 64)
    tiles_wide = _cdiv(wide.case.M, 64) * n_t
    rules = [
        ('Cin % kt', base, set_(base.desc(), Cin=48), c64, 0),
        ('in_ld % 4', base, set_(base.desc(), in_ld=70), c64, 0),
        ('M <= 0', base, set_(base.desc(), M=0), c64, 0),
        ('cout_pad below the tile multiple', base, set_(base.desc(), cout_pad=64), c128, 0),
        ('w_batch_rows no tile multiple', bankL, set_(_bank_desc(bank_case, bankL, wbank), cout_pad=64, w_batch_rows=96), c64, 0),
        ('w_batch_rows with 3x3', base, set_(base.desc(), cout_pad=128, w_batch_rows=64), c64, 0),
        ('empty K slice', base, ops.set_splitk(base.desc(), 7, P), c64, 0),
        ('ksplit with Cout % 4', base, set_(ops.set_splitk(base.desc(), 2, P), Cout=62), c64, 0),
        ('split_from no multiple of n_tiles', wide, ops.set_splitk(wide.desc(), 2, P, split_from=1), c64, 0),
        ('split_from past the tile count', wide, ops.set_splitk(wide.desc(), 2, P, split_from=tiles_wide + n_t), c64, 0),
        ('tile_counters with Cout % bn', wide, ops.set_splitk(wide.desc(), 2, P, counters=cnt), c64, 0),
        ('tile_counters on kind 1', base, ops.set_splitk(base.desc(), 2, P, counters=cnt), direct64, 0),
        ('ksplit on a wk configuration', base, ops.set_splitk(base.desc(), 2, P), cwk, 0),
        ('ksplit on a stream-K configuration', base, set_(ops.set_streamk(base.desc(), ws, sk_cnt), ksplit=2), sk, 0),
        ('stream-K without workspace', one, one.desc(), sk, 0),
        ('mask_ld % 4 with ksplit', masked, set_(ops.set_splitk(masked.desc(), 2, P), mask_ld=masked.L.mask_ld + 1), c64, 0),
        ('in_lp with relu_in', base, lp_relu(), c64, 2),
    ]
    assert len(rules) == 17 and Cin == 64
    led = Ledger()
    for name, run, d, cfg, mode in rules:
        assert _launch(d, cfg, mode) == ERR_ARG, name
        L = run.L if isinstance(run, Run) else run
        err, dirty, image = L.collect()
        led.add(name, base.case, torch.zeros_like(err), dirty, _untouched(image))
    led.add('counters', base.case, torch.zeros((), dtype=torch.float64, device=gpu), cnt.abs().sum(), sk_cnt.abs().sum())
    led.close('entry', 'refusals', 'rules')
    # each of these is the well-formed launch its rule's descriptor departs from: accepted
    for name, run, d, cfg in [('split', base, ops.set_splitk(base.desc(), 2, P), c64), ('tail', wide, ops.set_splitk(wide.desc(), 2, P, split_from=n_t, rows=wide.case.M - 64), c64),
                              ('stream-K', one, ops.set_streamk(one.desc(), ws, sk_cnt), sk)]:
        assert _launch(d, cfg) == OK, name
        err, dirty, _ = run.L.collect()
        led.add(name, run.case, err, dirty)
    led.close('entry', 'accepted', 'rules')


# ------------------------------------------------------------------------------------------------------------- NaN in, NaN out
@pytest.mark.parametrize('geom', sorted(NAN_AT), ids=_gname)
def test_a_nan_in_the_input_reaches_exactly_the_outputs_that_see_it(gpu, geom):
    """One input element is NaN.  Exactly the outputs the float64 reference makes NaN -- F.conv2d(relu(x)) through the epilogue:
    every output whose window covers the element, but those a mask zeroes -- are NaN, and every other output is within the bound.
    (common.h: a ReLU must keep a NaN, or a diverging training run is kept alive silently.)  Which launch reaches which copy of
    the ReLU, through every configuration:
      'none' / 'full' (ReLU in and out both off / both on), 16-byte strides: the staging floor of every kernel; relu_out of the
          branch-free buffer form of the LDS-tiled kernels and of the wide forms of conv_direct / conv_streamk;
      the same on odd strides: relu_out of the dword forms;
      'mask_relu' (mask + both ReLUs), 16-byte strides: a mask keeps the LDS-tiled kernels off the buffer form, so this is relu_out
          of the POINTER form of the wide epilogue; on odd strides the dword forms under a mask;
      split-K of all three variants: relu_out of splitk_reduce_kernel and of the in-launch finish."""
    from vfloodnet_amd import ops
    fam, tiles = _families(), ops.conv_cfg_tiles()
    N, H, W, Cin, Cout, k, s = geom
    ws, cnt = ops.streamk_scratch(gpu)
    fcnt = torch.zeros(4096, dtype=torch.int32, device=gpu)
    for variant in ('none', 'full', 'mask_relu'):
        case = conv_ref.make_case(geom, variant, 0, NAN_AT[geom])
        n_nan = int(torch.isnan(case.ref).sum())
        if variant == 'mask_relu':                   # (the mask is randn: it zeroes about half of them, never all or none of 36+)
            assert 0 < n_nan < Cout * k * k and bool((case.mask[torch.isnan(case.ref)] > 0).all())
        else:
            assert n_nan == Cout * k * k and n_nan < case.ref.numel()
        for strides in sorted(STRIDES):
            R, led = Run(gpu, case, strides), _ledgers()
            assert bool(torch.isnan(R.L.x).sum() == 1)
            for cfg in range(62):
                d = R.desc()
                if ops.conv_cfg_kind(cfg) == 2:
                    ops.set_streamk(d, ws, cnt)
                assert _launch(d, cfg) == OK, (cfg, variant, strides)
                err, dirty, _ = R.L.collect()
                led[fam[cfg]].add((cfg, variant, strides), case, err, dirty)
            if strides == 'wide' and Cout % 4 == 0:
                nk_all = k * k * (Cin // 32)
                P = torch.empty(nk_all * case.M * Cout + 64, device=gpu)
                for cfg in _splitk_cfgs():
                    for ks in (2, nk_all):
                        for counters in (None, fcnt) if (fam[cfg] != 'direct' and Cout % tiles[cfg][1] == 0) else (None,):
                            P.fill_(NAN)
                            assert _launch(ops.set_splitk(R.desc(), ks, P, counters=counters), cfg) == OK, (cfg, ks)
                            err, dirty, _ = R.L.collect()
                            led[fam[cfg]].add((cfg, variant, 'split', ks, counters is not None), case, err, dirty)
            led['streamk'].add(('counters',), case, torch.zeros((), dtype=torch.float64, device=gpu), cnt.abs().sum(), fcnt.abs().sum())
            _close(led, f'nan/{variant}/{strides}', _gname(geom))


@pytest.mark.parametrize('geom', [GEOMS[2], GEOMS[7]], ids=_gname)
def test_every_epilogue_copy_gives_the_bits_of_the_wide_buffer_path(gpu, geom):
    """Holds the copies of the epilogue to one another on finite inputs: the dword form (odd strides) of every configuration writes
    the bits its wide form writes (16-byte strides: the branch-free buffer form of the LDS-tiled kernels without a mask, their
    pointer form under one), for the five variants and for 'mask_relu'.  This compares copies inside one build: both sides share
    the staging code, and conv_direct / conv_streamk have no form that predates the NaN-keeping ReLU, so it does not show that a
    finite result kept its bits across that change -- vfn_relu_nan returns fmaxf's value for every number by construction, and
    vfn_floor_nan differs from fmaxf only in keeping -0 under a floor of 0, which cannot change a sum that starts at +0."""
    fam = _families()
    from vfloodnet_amd import ops
    ws, cnt = ops.streamk_scratch(gpu)
    for variant in conv_ref.VARIANTS + ('mask_relu',):
        case = conv_ref.make_case(geom, variant)
        runs, led = [Run(gpu, case, st) for st in ('wide', 'odd')], _ledgers()
        for cfg in range(62):
            images = []
            for R in runs:
                d = R.desc()
                if ops.conv_cfg_kind(cfg) == 2:
                    ops.set_streamk(d, ws, cnt)
                assert _launch(d, cfg) == OK, (cfg, variant)
                err, dirty, image = R.L.collect()
                images.append(image)
                led[fam[cfg]].add((cfg, variant), case, err, dirty)
            led[fam[cfg]].add((cfg, variant, 'dword != wide'), case, torch.zeros_like(err), _differs(*images))
        _close(led, f'bits/{variant}', _gname(geom))
