"""The entry points of ``csrc/encoder_train.hip`` (include/vfn_encoder_train.h) one by one against ``tests/encoder_train_ref.py``
in float64.

Every buffer sits inside a larger allocation that holds NaN: in front of it, behind it and in the columns C .. ld-1 of every
row.  The poison must survive outside the written region and no NaN may reach a result, so a stray access is a failed
assertion.  Every launch is made twice: equal bits.

The error rule is the one of tests/test_image_train_kernels_gpu.py: the same formula evaluated in float32 on the CPU lies
``e32 / |ref|max`` from the float64 result; a kernel may be 8 x the largest such ratio over its case list away from float64, in
units of the case's ``|ref|max``."""
import functools
import zlib

import pytest
import torch

import encoder_train_ref as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
FACTOR = 8.0
VFN_ERR_ARG = 1
GUARD = 2                                                       # rows of NaN in front of and behind every matrix
# (N, H, W, C, k, stride, Ho, Wo; Ho = None: H // stride): the smallest shapes at which the index arithmetic can go wrong
DW_SHAPES = [(1, 1, 1, 4, 5, 1, None, None),                    # the filter is all padding
             (2, 2, 3, 8, 3, 1, None, None),                    # small map, stride 1
             (1, 5, 7, 12, 5, 1, None, None),                   # odd map, stride 1
             (1, 4, 6, 12, 3, 2, None, None),                   # pad 0 before, 1 after
             (2, 6, 4, 36, 5, 2, None, None),                   # pad 1 before, 2 after
             (1, 5, 7, 4, 3, 2, 2, 3),                          # Ho = H // 2 on an odd map
             (1, 6, 8, 4, 3, 2, 2, 3),                          # the last input row and column receive no gradient
             (1, 2, 2, 2688, 5, 1, None, None),                 # width; a 5 x 5 filter on a 2 x 2 map
             (3, 32, 32, 8, 3, 2, None, None)]                  # 3072 input rows: crosses chunk boundaries


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _lib():
    from vfloodnet_amd import _lib
    return _lib


def _pad_before(k, s):
    from vfloodnet_amd.linknet import _same_pad_before
    return _same_pad_before(k, s)


class Buf:
    """A [rows, C] matrix with leading dimension ld inside a NaN allocation; ``data`` None: an output, NaN throughout."""

    def __init__(self, dev, rows, C, ld=None, data=None, dtype=torch.float32):
        ld = C if ld is None else ld
        full = torch.full((GUARD + rows + GUARD, ld), NAN, dtype=dtype)
        if data is not None:
            full[GUARD:GUARD + rows, :C] = data.reshape(rows, C).to(dtype)
        self.full, self.rows, self.C, self.ld = full.to(dev), rows, C, ld

    @property
    def ptr(self):
        return _lib().ptr(self.full[GUARD:])

    def value(self):
        return self.full[GUARD:GUARD + self.rows, :self.C].cpu()

    def poison_kept(self):
        m = torch.ones_like(self.full, dtype=torch.bool)
        m[GUARD:GUARD + self.rows, :self.C] = False
        return bool(torch.isnan(self.full[m]).all())

    def untouched(self):
        return bool(torch.isnan(self.full).all())


def _dist(got, ref64, scale):
    d = (got.double() - ref64).abs().max().item()
    return float('inf') if d != d else d / scale


def _hold(name, rows):
    """rows: (case, quantity, float32 distance, kernel distance), both in units of the quantity's scale."""
    bound, worst = {}, {}
    for case, q, e32, e in rows:
        bound[q] = max(bound.get(q, 0.0), e32)
        if e >= worst.get(q, (-1.0, None))[0]:
            worst[q] = (e, case)
    for q in bound:
        print(f'{name} {q}: float32 ratio {bound[q]:.3e}  bound {FACTOR * bound[q]:.3e}  kernel error {worst[q][0]:.3e} at {worst[q][1]}')
    for q in bound:
        assert worst[q][0] <= FACTOR * bound[q], (name, q, worst[q][1], f'error {worst[q][0]:.3e}', f'bound {FACTOR * bound[q]:.3e}')


def _twice(launch, outs):
    """Runs ``launch`` twice into fresh outputs; -> the first run's values after the bit comparison and the poison checks."""
    first = launch()
    torch.cuda.synchronize()
    second = launch()
    torch.cuda.synchronize()
    vals = []
    for a, b in zip(first, second):
        va, vb = a.value(), b.value()
        assert not torch.isnan(va).any() and a.poison_kept() and b.poison_kept()
        assert torch.equal(va, vb)
        vals.append(va)
    return vals


# ------------------------------------------------------------------------------------------------------- element-wise
MAT_CASES = [(1, 1, 4, 8), (2, 5, 12, 16), (3, 7, 36, 40), (1, 3, 2688, 2692), (2, 1500, 8, 12)]      # (B, M, C, ld)


@functools.lru_cache(maxsize=None)
def _mats(case):
    B, M, C, ld = case
    g = _gen('mats', case)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=1.5 * r(B, M, C), g=r(B, M, C), res=r(B, M, C), scale=1 + 0.2 * r(C), shift=0.3 * r(C), gate=torch.rand(B, C, generator=g),
                dpool=r(B, C))


def test_affine_and_scale_rows(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for case in MAT_CASES:
        B, M, C, ld = case
        t = _mats(case)
        xb, rb = Buf(gpu, B * M, C, ld, t['x']), Buf(gpu, B * M, C, ld + 4, t['res'])
        sc, sh, gt = Buf(gpu, 1, C, data=t['scale']), Buf(gpu, 1, C, data=t['shift']), Buf(gpu, B, C, data=t['gate'])
        for act in (0, 1):
            for res in (None, rb):
                def launch():
                    y = Buf(gpu, B * M, C, ld + 8)
                    assert lib.vfn_et_affine_f32(xb.ptr, sc.ptr, sh.ptr, res.ptr if res else None, y.ptr, B * M, C, ld, ld + 4, ld + 8, act,
                                                 L.stream()) == 0
                    return [y]
                got, = _twice(launch, 1)
                f = lambda d: R.affine(t['x'].to(d), t['scale'].to(d), t['shift'].to(d), t['res'].to(d) if res else None, bool(act)).reshape(B * M, C)
                ref = f(torch.float64)
                rows.append((case + (act, bool(res)), 'affine', _dist(f(torch.float32), ref, ref.abs().max().item()), _dist(got, ref, ref.abs().max().item())))

        def launch():
            y = Buf(gpu, B * M, C, ld + 8)
            assert lib.vfn_et_scale_rows_f32(xb.ptr, gt.ptr, y.ptr, B, M, C, ld, ld + 8, L.stream()) == 0
            return [y]
        got, = _twice(launch, 1)
        ref = R.scale_rows(t['x'].double(), t['gate'].double()).reshape(B * M, C)
        rows.append((case, 'scale_rows', _dist(R.scale_rows(t['x'], t['gate']).reshape(B * M, C), ref, ref.abs().max().item()),
                     _dist(got, ref, ref.abs().max().item())))
        assert xb.poison_kept() and rb.poison_kept()
    _hold('element-wise', rows)


def test_swish_backward(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for case in MAT_CASES:
        B, M, C, ld = case
        t = _mats(case)
        gb, xb = Buf(gpu, B * M, C, ld, t['g']), Buf(gpu, B * M, C, ld + 4, t['x'])
        sc, sh = Buf(gpu, 1, C, data=t['scale']), Buf(gpu, 1, C, data=t['shift'])
        gt, dp = Buf(gpu, B, C, data=t['gate']), Buf(gpu, B, C, data=t['dpool'])
        for gated in (False, True):
            def launch():
                y = Buf(gpu, B * M, C, ld + 8)
                assert lib.vfn_et_swish_bwd_f32(gb.ptr, gt.ptr if gated else None, dp.ptr if gated else None, 1.0 / M, xb.ptr, sc.ptr, sh.ptr,
                                                y.ptr, B, M, C, ld, ld + 4, ld + 8, L.stream()) == 0
                return [y]
            got, = _twice(launch, 1)
            f = lambda d: R.swish_bwd(t['g'].to(d), t['x'].to(d), t['scale'].to(d), t['shift'].to(d), t['gate'].to(d) if gated else None,
                                      t['dpool'].to(d) if gated else None, 1.0 / M).reshape(B * M, C)
            ref = f(torch.float64)
            rows.append((case + (gated,), 'swish_bwd', _dist(f(torch.float32), ref, ref.abs().max().item()), _dist(got, ref, ref.abs().max().item())))
    _hold('swish backward', rows)


# -------------------------------------------------------------------------------------------------------- column sums
def test_column_sums(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for case in MAT_CASES + [(1, 3001, 8, 8), (3, 700, 68, 72)]:
        B, M, C, ld = case
        t = _mats(case)
        gb, ab = Buf(gpu, B * M, C, ld, t['g']), Buf(gpu, B * M, C, ld + 4, t['x'])
        for with_a in (True, False):
            def launch():
                part = Buf(gpu, 1, L.ET_MAX_BLOCKS * 2 * C, dtype=torch.float64)
                s0, s1 = Buf(gpu, B, C), Buf(gpu, B, C)
                assert lib.vfn_et_colsums_f32(gb.ptr, ab.ptr if with_a else None, B, M, C, ld, ld + 4, part.ptr, s0.ptr, s1.ptr if with_a else None,
                                              L.stream()) == 0
                assert part.poison_kept() and (with_a or s1.untouched())
                return [s0, s1] if with_a else [s0]
            got = _twice(launch, 2)
            ref = R.colsums(t['g'].double(), t['x'].double() if with_a else None)
            r32 = R.colsums(t['g'], t['x'] if with_a else None)
            for i, q in enumerate(('sum_g', 'sum_ga')[:len(got)]):
                scale = ref[2 + i].max().item()                  # sums of signed numbers: the summands' magnitudes are the scale
                rows.append((case, q, _dist(r32[i], ref[i], scale), _dist(got[i], ref[i], scale)))
    _hold('column sums', rows)


# -------------------------------------------------------------------------------------------------- squeeze-excite backward
SE_CASES = [(1, 4, 1, 4), (3, 4, 1, 8), (1, 1632, 68, 1632), (3, 1632, 68, 1664), (3, 144, 6, 160)]      # (B, C, sq, Cpad)


def test_squeeze_excite_backward(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for case in SE_CASES:
        B, C, sq, Cpad = case
        g = _gen('se', case)
        r = lambda *s: torch.randn(*s, generator=g)
        hw = 49
        t = dict(sum_px=hw * 0.5 * r(B, C), dgate=r(B, C), w1=r(sq, C) / C ** 0.5, b1=0.2 * r(sq), w2=r(C, sq) / sq ** 0.5, b2=0.2 * r(C))
        pad = lambda v: torch.cat([v, torch.zeros(B, Cpad - C)], 1)
        spx, dg = Buf(gpu, B, Cpad, data=pad(t['sum_px'])), Buf(gpu, B, Cpad, data=pad(t['dgate']))
        w1, b1, w2, b2 = Buf(gpu, sq, C, data=t['w1']), Buf(gpu, 1, sq, data=t['b1']), Buf(gpu, C, sq, data=t['w2']), Buf(gpu, 1, C, data=t['b2'])

        def launch():
            tmp = Buf(gpu, B, Cpad + 2 * sq)
            outs = [Buf(gpu, B, Cpad), Buf(gpu, sq, C), Buf(gpu, 1, sq), Buf(gpu, C, sq), Buf(gpu, 1, C)]
            assert lib.vfn_et_se_bwd_f32(spx.ptr, 1.0 / hw, dg.ptr, w1.ptr, b1.ptr, w2.ptr, b2.ptr, tmp.ptr, *(o.ptr for o in outs), B, C, sq, Cpad,
                                         L.stream()) == 0
            assert tmp.poison_kept()
            return outs
        got = _twice(launch, 5)
        f = lambda d: R.se_bwd(*(t[k].to(d) if k != 'inv' else 1.0 / hw for k in ('sum_px', 'inv', 'dgate', 'w1', 'b1', 'w2', 'b2')))
        ref, r32 = f(torch.float64), f(torch.float32)
        assert not got[0][:, C:].any()                           # padded channels: 0
        for v, q in zip(got, ('dpool', 'dw1', 'db1', 'dw2', 'db2')):
            want = ref[q].reshape(v.shape[0], -1)
            v = v[:, :want.shape[1]]
            rows.append((case, q, _dist(r32[q].reshape(want.shape), want, want.abs().max().item()), _dist(v, want, want.abs().max().item())))
    _hold('squeeze-excite backward', rows)


# --------------------------------------------------------------------------------------------------------- depthwise
@functools.lru_cache(maxsize=None)
def _dw(case):
    N, H, W, C, k, s, Ho, Wo = case
    Ho, Wo = (H // s if Ho is None else Ho), (W // s if Wo is None else Wo)
    g = _gen('dw', case)
    r = lambda *sh: torch.randn(*sh, generator=g)
    return dict(x=1.5 * r(N, H, W, C), g=r(N, Ho, Wo, C), w=r(k * k, C) / k, scale=1 + 0.2 * r(C), shift=0.3 * r(C), Ho=Ho, Wo=Wo,
                pb=_pad_before(k, s))


def test_depthwise_forward_data_and_weight_gradient(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for case in DW_SHAPES:
        N, H, W, C, k, s = case[:6]
        t = _dw(case)
        Ho, Wo, pb = t['Ho'], t['Wo'], t['pb']
        Mi, Mo, ld = N * H * W, N * Ho * Wo, C + 4
        xb, gb, wb = Buf(gpu, Mi, C, ld, t['x']), Buf(gpu, Mo, C, ld + 4, t['g']), Buf(gpu, k * k, C, data=t['w'])
        sc, sh = Buf(gpu, 1, C, data=t['scale']), Buf(gpu, 1, C, data=t['shift'])
        for act in (0, 1):
            def launch():
                out, gx, dw = Buf(gpu, Mo, C, ld + 8), Buf(gpu, Mi, C, ld + 8), Buf(gpu, k * k, C)
                part = Buf(gpu, 1, L.ET_MAX_BLOCKS * k * k * C if Mi > 64 else k * k * C, dtype=torch.float64)
                assert lib.vfn_et_dwconv_f32(xb.ptr, wb.ptr, sc.ptr, sh.ptr, out.ptr, N, H, W, C, ld, ld + 8, k, s, pb, Ho, Wo, act, L.stream()) == 0
                assert lib.vfn_et_dw_dgrad_f32(gb.ptr, wb.ptr, xb.ptr if act else None, gx.ptr, N, H, W, C, ld + 4, ld, ld + 8, k, s, pb, Ho, Wo, act,
                                               L.stream()) == 0
                assert lib.vfn_et_dw_wgrad_f32(gb.ptr, xb.ptr, part.ptr, dw.ptr, N, H, W, C, ld + 4, ld, k, s, pb, Ho, Wo, act, L.stream()) == 0
                assert part.poison_kept()
                return [out, gx, dw]
            got = _twice(launch, 3)

            def f(d):
                x, g, w = t['x'].to(d), t['g'].to(d), t['w'].to(d)
                out = R.affine(R.dw_forward(R.swish(x) if act else x, w, k, s, pb, Ho, Wo), t['scale'].to(d), t['shift'].to(d))
                dw, mag = R.dw_wgrad(g, x, k, s, pb, act=bool(act))
                return out.reshape(Mo, C), R.dw_dgrad(g, w, H, W, k, s, pb, y=x if act else None).reshape(Mi, C), dw, mag
            ref, r32 = f(torch.float64), f(torch.float32)
            for i, q in enumerate(('forward', 'dgrad', 'wgrad')):
                scale = max(ref[i].abs().max().item(), 1e-30) if q != 'wgrad' else max(ref[3].max().item(), 1e-30)
                rows.append((case + (act,), q, _dist(r32[i], ref[i], scale), _dist(got[i], ref[i], scale)))
        assert xb.poison_kept() and gb.poison_kept()
    _hold('depthwise', rows)


# -------------------------------------------------------------------------------------------------------------- stem
STEM_CASES = [(1, 2, 2, 48, 52), (2, 6, 10, 64, 64), (1, 5, 7, 48, 48), (3, 64, 32, 64, 68)]      # (N, H, W, Cp, ld); the last: 1536 rows


def test_stem_forward_and_weight_gradient(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    pb = _pad_before(3, 2)
    for case in STEM_CASES:
        N, H, W, Cp, ld = case
        Ho, Wo = (H + 1) // 2, (W + 1) // 2
        M = N * Ho * Wo
        g = _gen('stem', case)
        r = lambda *s: torch.randn(*s, generator=g)
        x, w, gr, scale, shift = r(N, 3, H, W), r(48, 3, 3, 3) / 5, r(N, Ho, Wo, 48), 1 + 0.2 * r(48), 0.3 * r(48)
        xb, wb, gb = Buf(gpu, 1, x.numel(), data=x), Buf(gpu, 1, 1296, data=w), Buf(gpu, M, 48, ld, gr)
        sc, sh = Buf(gpu, 1, 48, data=scale), Buf(gpu, 1, 48, data=shift)

        def launch():
            out, dw, part = Buf(gpu, M, Cp, ld), Buf(gpu, 1, 1296), Buf(gpu, 1, L.ET_MAX_BLOCKS * 1296, dtype=torch.float64)
            assert lib.vfn_et_stem_f32(xb.ptr, wb.ptr, sc.ptr, sh.ptr, out.ptr, N, H, W, Ho, Wo, Cp, ld, pb, L.stream()) == 0
            assert lib.vfn_et_stem_wgrad_f32(gb.ptr, xb.ptr, part.ptr, dw.ptr, N, H, W, Ho, Wo, ld, pb, L.stream()) == 0
            assert part.poison_kept()
            return [out, dw]
        out, dw = _twice(launch, 2)
        assert not out[:, 48:].any()
        f = lambda d: (R.stem_forward(x.to(d), w.to(d), scale.to(d), shift.to(d), Ho, Wo, pb).reshape(M, 48),) + R.stem_wgrad(gr.to(d), x.to(d), pb)
        ref, r32 = f(torch.float64), f(torch.float32)
        rows.append((case, 'forward', _dist(r32[0], ref[0], ref[0].abs().max().item()), _dist(out[:, :48], ref[0], ref[0].abs().max().item())))
        scale_w = ref[2].max().item()
        rows.append((case, 'wgrad', _dist(r32[1], ref[1], scale_w), _dist(dw.reshape(48, 3, 3, 3), ref[1], scale_w)))
    _hold('stem', rows)


# ------------------------------------------------------------------------------------------------------------ refusals
def test_bad_arguments_launch_nothing(gpu):
    L, lib = _lib(), _lib().lib()
    S = L.stream()
    N, H, W, C, k, s = 2, 6, 4, 8, 5, 2
    Ho, Wo, pb = 3, 2, 1
    Mi, Mo = N * H * W, N * Ho * Wo
    r = lambda *sh: torch.randn(*sh)
    x, g, w, v = Buf(gpu, Mi, C, data=r(Mi, C)), Buf(gpu, Mo, C, data=r(Mo, C)), Buf(gpu, k * k, C, data=r(k * k, C)), Buf(gpu, 1, C, data=r(C))
    gate = Buf(gpu, N, C, data=r(N, C))
    img, gs = Buf(gpu, 1, N * 3 * H * W, data=r(N * 3 * H * W)), Buf(gpu, Mo, 48, data=r(Mo, 48))
    out, part = Buf(gpu, Mi, 64), Buf(gpu, 1, 4096, dtype=torch.float64)
    o, p = out.ptr, part.ptr
    bad = R.refusals(lib, x.ptr, g.ptr, w.ptr, v.ptr, gate.ptr, img.ptr, gs.ptr, o, p, S)
    assert len(bad) > 80
    torch.cuda.synchronize()
    assert all(st == VFN_ERR_ARG for _, _, st in bad), [b for b in bad if b[2] != VFN_ERR_ARG]
    assert out.untouched() and part.untouched()                  # nothing was launched
    assert x.poison_kept() and g.poison_kept()
    # the same pointers with good sizes do run
    assert lib.vfn_et_dw_wgrad_f32(g.ptr, x.ptr, p, o, N, H, W, C, C, C, k, s, pb, Ho, Wo, 1, S) == 0
    torch.cuda.synchronize()
    assert not out.untouched()
