"""The entry points of ``csrc/encoder_bn_train.hip`` (include/vfn_encoder_bn_train.h) one by one against the float64 formulas of
``tests/encoder_bn_train_ref.py``.

The rules are tests/test_encoder_train_kernels_gpu.py's: every buffer sits inside a larger allocation that holds NaN, strided
(ld > C), the poison must survive outside the written region and no NaN may reach a result; every launch is made twice: equal
bits; a kernel may be 8 x the float32 CPU formula's largest distance from float64 over the case list away from float64, in units
of the case's ``|ref|max``.

Shapes: M in {2, 63, 64, 65, 1025} (the smallest batch, one chunk and its edges, seventeen chunks), C in {4, 32, 2688} (one quad,
a partial column tile, the widest layer: 42 column tiles), B in {1, 3} with a dropped image."""
import functools

import pytest
import torch

import encoder_bn_train_ref as B
from test_encoder_train_kernels_gpu import Buf, _dist, _gen, _hold, _lib, _twice, VFN_ERR_ARG

pytestmark = pytest.mark.gpu

MS, CS = (2, 63, 64, 65, 1025), (4, 32, 2688)
EPS, MOM = B.BN_EPS_ENC, B.BN_MOMENTUM_ENC


@functools.lru_cache(maxsize=None)
def _stats_case(M, C):
    """z [M][C]: column 0 constant, column 1 with mean 1e4 and unit spread, the others with means and spreads of order one."""
    g = _gen('bn stats', M, C)
    r = lambda *s: torch.randn(*s, generator=g)
    z = r(M, C) * (0.5 + torch.rand(C, generator=g)) + 2 * r(C)
    z[:, 0] = 7.25
    z[:, 1] = 1e4 + r(M)
    return dict(z=z, gamma=1 + 0.2 * r(C), rm=0.3 * r(C), rv=0.5 + torch.rand(C, generator=g))


def test_batch_statistics(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for M in MS:
        for C in CS:
            t = _stats_case(M, C)
            ld, c_run = C + 4, C - 1
            zb, gb = Buf(gpu, M, C, ld, t['z']), Buf(gpu, 1, C, data=t['gamma'])

            def launch(track=True):
                part = Buf(gpu, 1, L.ET_MAX_BLOCKS * 2 * C, dtype=torch.float64)
                outs = [Buf(gpu, 1, C) for _ in range(3)]
                rm, rv = Buf(gpu, 1, c_run, data=t['rm'][:c_run]), Buf(gpu, 1, c_run, data=t['rv'][:c_run])
                assert lib.vfn_et_bn_stats_f32(zb.ptr, M, C, ld, gb.ptr, EPS, MOM, part.ptr, *(o.ptr for o in outs), rm.ptr if track else None,
                                               rv.ptr if track else None, c_run, L.stream()) == 0
                assert part.poison_kept()
                return outs + [rm, rv]
            rstd, nshift, fold, rm, rv = _twice(launch, 5)
            untracked = _twice(lambda: launch(False), 5)
            assert torch.equal(untracked[3][0], t['rm'][:c_run]) and torch.equal(untracked[4][0], t['rv'][:c_run])     # null: nothing moves
            assert all(torch.equal(a, b) for a, b in zip(untracked[:3], (rstd, nshift, fold)))
            f = lambda d: B.bn_stats(t['z'].to(d), t['gamma'].to(d), EPS, MOM, t['rm'].to(d), t['rv'].to(d))
            ref, r32 = f(torch.float64), f(torch.float32)
            # a constant column: variance 0 exactly
            rs0 = (1 / torch.sqrt(torch.tensor(EPS, dtype=torch.float64)))
            assert ref['var'][0] == 0 and rstd[0, 0] == rs0.float() and nshift[0, 0] == (-7.25 * rs0).float()
            assert rv[0, 0] == ((1 - MOM) * t['rv'][0].double()).float()
            rest = list(range(2, C))                             # (column 0 is held exactly above)
            for q, got, n in (('rstd', rstd, C), ('nshift', nshift, C), ('fold', fold, C), ('running_mean', rm, c_run), ('running_var', rv, c_run)):
                for cols, tag in (([c for c in rest if c < n], ''), ([1], ' (mean 1e4)')):
                    want = ref[q][cols]
                    scale = max(want.abs().max().item(), 1e-30)
                    rows.append(((M, C), q + tag, _dist(r32[q][cols], want, scale), _dist(got[0][cols], want, scale)))
            assert zb.poison_kept()
    _hold('batch statistics', rows)


@functools.lru_cache(maxsize=None)
def _mat_case(Bn, M, C):
    g = _gen('bn mats', Bn, M, C)
    r = lambda *s: torch.randn(*s, generator=g)
    keep = torch.full((Bn,), 1 / 0.9)
    keep[Bn // 2] = 0.0 if Bn > 1 else 1.25
    return dict(z=2 * r(Bn, M, C) + 1, g=r(Bn, M, C), res=r(Bn, M, C), rstd=0.5 + torch.rand(C, generator=g), nshift=r(C), gamma=1 + 0.2 * r(C),
                beta=0.3 * r(C), dbeta=3 * r(C), dgamma=3 * r(C), keep=keep)


def test_normalisation(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for Bn in (1, 3):
        for M in MS:
            for C in CS:
                t = _mat_case(Bn, M, C)
                R_, ld = Bn * M, C + 4
                rb, kb = Buf(gpu, R_, C, ld + 4, t['res']), Buf(gpu, 1, Bn, data=t['keep'])
                v = {k: Buf(gpu, 1, C, data=t[k]) for k in ('rstd', 'nshift', 'gamma', 'beta')}
                for act, keep, res, inplace in ((1, True, True, False), (0, False, False, True), (0, True, True, True), (1, False, True, False)):
                    def launch():
                        zb = Buf(gpu, R_, C, ld, t['z'])
                        xh, y = (zb if inplace else Buf(gpu, R_, C, ld)), Buf(gpu, R_, C, ld + 8)
                        assert lib.vfn_et_bn_norm_f32(zb.ptr, v['rstd'].ptr, v['nshift'].ptr, v['gamma'].ptr, v['beta'].ptr, kb.ptr if keep else None,
                                                      rb.ptr if res else None, xh.ptr, y.ptr, Bn, M, C, ld, ld + 4, ld, ld + 8, act, L.stream()) == 0
                        if not inplace:
                            torch.cuda.synchronize()
                            assert torch.equal(zb.value(), t['z'].reshape(R_, C)) and zb.poison_kept()
                        return [xh, y]
                    xh, y = _twice(launch, 2)
                    f = lambda d: B.bn_norm(t['z'].to(d), t['rstd'].to(d), t['nshift'].to(d), t['gamma'].to(d), t['beta'].to(d),
                                            t['keep'].to(d) if keep else None, t['res'].to(d) if res else None, bool(act))
                    ref, r32 = f(torch.float64), f(torch.float32)
                    for q, got, i in (('xh', xh, 0), ('y', y, 1)):
                        want = ref[i].reshape(R_, C)
                        rows.append(((Bn, M, C, act, keep, res, inplace), q, _dist(r32[i].reshape(R_, C), want, want.abs().max().item()),
                                     _dist(got, want, want.abs().max().item())))
                    if keep and res and Bn > 1:                     # the dropped image's branch contributes nothing
                        b0 = Bn // 2
                        assert torch.equal(y[b0 * M:(b0 + 1) * M], t['res'][b0])
                assert rb.poison_kept()
    _hold('normalisation', rows)


def test_sums_and_centring(gpu):
    L, lib = _lib(), _lib().lib()
    rows = []
    for Bn in (1, 3):
        for M in MS:
            for C in CS:
                t = _mat_case(Bn, M, C)
                R_, ld = Bn * M, C + 4
                xb, kb = Buf(gpu, R_, C, ld + 4, t['z']), Buf(gpu, 1, Bn, data=t['keep'])
                db, dg = Buf(gpu, 1, C, data=t['dbeta']), Buf(gpu, 1, C, data=t['dgamma'])
                for keep, inplace in ((True, False), (False, True), (False, False)):
                    def launch():
                        gb = Buf(gpu, R_, C, ld, t['g'])
                        gp = gb if inplace else Buf(gpu, R_, C, ld)
                        assert lib.vfn_et_bn_center_f32(gb.ptr, xb.ptr, kb.ptr if keep else None, db.ptr, dg.ptr, gp.ptr, Bn, M, C, ld, ld + 4, ld,
                                                        L.stream()) == 0
                        if not inplace:
                            torch.cuda.synchronize()
                            assert torch.equal(gb.value(), t['g'].reshape(R_, C)) and gb.poison_kept()     # a residual block's pass-through
                        return [gp]
                    got, = _twice(launch, 1)
                    f = lambda d: B.bn_center(t['g'].to(d), t['z'].to(d), t['dbeta'].to(d), t['dgamma'].to(d), t['keep'].to(d) if keep else None)
                    want = f(torch.float64).reshape(R_, C)
                    rows.append(((Bn, M, C, keep, inplace), 'center', _dist(f(torch.float32).reshape(R_, C), want, want.abs().max().item()),
                                 _dist(got, want, want.abs().max().item())))
                assert xb.poison_kept()
            # the per-image sums under the scale (parameter-sized: once per B and C)
        for C in CS:
            t = _mat_case(Bn, 2, C)
            sg, sga = 50 * t['g'][:, 0], 50 * t['g'][:, 1]
            sgb, sgab, kb = Buf(gpu, Bn, C, data=sg), Buf(gpu, Bn, C, data=sga), Buf(gpu, 1, Bn, data=t['keep'])
            for keep in (True, False):
                def launch():
                    o = [Buf(gpu, 1, C), Buf(gpu, 1, C)]
                    assert lib.vfn_et_bn_sums_f32(sgb.ptr, sgab.ptr, kb.ptr if keep else None, o[0].ptr, o[1].ptr, Bn, C, L.stream()) == 0
                    return o
                got = _twice(launch, 2)
                f = lambda d: B.bn_sums(sg.to(d), sga.to(d), t['keep'].to(d) if keep else None)
                ref, r32 = f(torch.float64), f(torch.float32)
                for i, q in enumerate(('dbeta', 'dgamma')):
                    scale = (sg if i == 0 else sga).abs().sum(0).max().item()
                    rows.append(((Bn, C, keep), q, max(_dist(r32[i], ref[i], scale), 2.0 ** -25), _dist(got[i][0], ref[i], scale)))
    _hold('sums and centring', rows)


def test_one_batchnorm_forward_and_backward_chained(gpu):
    """The launches of one BatchNorm under drop-connect as the trainer chains them -- statistics, normalisation in place, per-image
    column sums, the sums under the scale, the centring out of place -- against ``F.batch_norm(training=True)`` under autograd in
    float64: y, dbeta, dgamma and g_z = fold g'.  The yardstick is the chain of formulas in float32."""
    import torch.nn.functional as F
    L, lib = _lib(), _lib().lib()
    Bn, M, C, ld = 3, 65, 36, 40
    t = _mat_case(Bn, M, C)
    R_ = Bn * M
    zb, gb, kb = Buf(gpu, R_, C, ld, t['z']), Buf(gpu, R_, C, ld, t['g']), Buf(gpu, 1, Bn, data=t['keep'])
    gam, bet = Buf(gpu, 1, C, data=t['gamma']), Buf(gpu, 1, C, data=t['beta'])
    part = Buf(gpu, 1, L.ET_MAX_BLOCKS * 2 * C, dtype=torch.float64)
    rstd, nshift, fold, dbeta, dgamma = (Buf(gpu, 1, C) for _ in range(5))
    sg, sga, y, gp = Buf(gpu, Bn, C), Buf(gpu, Bn, C), Buf(gpu, R_, C, ld), Buf(gpu, R_, C, ld)
    S = L.stream()
    assert lib.vfn_et_bn_stats_f32(zb.ptr, R_, C, ld, gam.ptr, EPS, MOM, part.ptr, rstd.ptr, nshift.ptr, fold.ptr, None, None, 0, S) == 0
    assert lib.vfn_et_bn_norm_f32(zb.ptr, rstd.ptr, nshift.ptr, gam.ptr, bet.ptr, kb.ptr, None, zb.ptr, y.ptr, Bn, M, C, ld, ld, ld, ld, 0, S) == 0
    assert lib.vfn_et_colsums_f32(gb.ptr, zb.ptr, Bn, M, C, ld, ld, part.ptr, sg.ptr, sga.ptr, S) == 0
    assert lib.vfn_et_bn_sums_f32(sg.ptr, sga.ptr, kb.ptr, dbeta.ptr, dgamma.ptr, Bn, C, S) == 0
    assert lib.vfn_et_bn_center_f32(gb.ptr, zb.ptr, kb.ptr, dbeta.ptr, dgamma.ptr, gp.ptr, Bn, M, C, ld, ld, ld, S) == 0
    torch.cuda.synchronize()

    def autograd(d):
        z, gamma, beta = (t[k].to(d).requires_grad_(True) for k in ('z', 'gamma', 'beta'))
        out = F.batch_norm(z.reshape(-1, C), None, None, gamma, beta, True, MOM, EPS).reshape(Bn, M, C) * t['keep'].to(d)[:, None, None]
        return (out.detach().reshape(R_, C),) + tuple(v.detach() for v in torch.autograd.grad(out, (beta, gamma, z), t['g'].to(d)))

    def formulas(d):                                              # the yardstick: the same chain of formulas in float32
        z, g_, keep = t['z'].to(d), t['g'].to(d), t['keep'].to(d)
        st = B.bn_stats(z.reshape(-1, C), t['gamma'].to(d), EPS, MOM)
        xh, out = B.bn_norm(z, st['rstd'], st['nshift'], t['gamma'].to(d), t['beta'].to(d), keep)
        db_, dg_, gc = B.bn_backward(g_, xh, keep)
        return out.reshape(R_, C), db_, dg_, st['fold'] * gc
    ref, r32 = autograd(torch.float64), formulas(torch.float32)
    assert all((a.reshape(b.shape) - b).abs().max() <= 1e-11 * b.abs().max() for a, b in zip(formulas(torch.float64), ref))
    got = (y.value(), dbeta.value()[0], dgamma.value()[0], (fold.value() * gp.value()))
    rows = []
    for q, g_, want, w32 in zip(('y', 'dbeta', 'dgamma', 'g_z'), got, ref, r32):
        want = want.reshape(g_.shape)
        scale = want.abs().max().item()
        rows.append(('chain', q, _dist(w32.reshape(g_.shape), want, scale), _dist(g_, want, scale)))
    assert all(b.poison_kept() for b in (zb, gb, y, gp, sg, sga, dbeta, dgamma))
    _hold('one BatchNorm chained', rows)


def test_bad_arguments_launch_nothing(gpu):
    L, lib = _lib(), _lib().lib()
    S = L.stream()
    r = lambda *sh: torch.randn(*sh)
    x, v, k = Buf(gpu, 12, 12, data=r(12, 12)), Buf(gpu, 1, 8, data=r(8)), Buf(gpu, 1, 2, data=torch.tensor([0.0, 1.25]))
    out, part = Buf(gpu, 12, 12), Buf(gpu, 1, 4096, dtype=torch.float64)
    bad = B.refusals(lib, x.ptr, v.ptr, k.ptr, out.ptr, part.ptr, S)
    assert len(bad) > 55
    torch.cuda.synchronize()
    assert all(st == VFN_ERR_ARG for _, _, st in bad), [b for b in bad if b[2] != VFN_ERR_ARG]
    assert out.untouched() and part.untouched()                  # nothing was launched
    assert x.poison_kept() and v.poison_kept()
    # the same pointers with good sizes do run
    assert lib.vfn_et_bn_center_f32(x.ptr, x.ptr, k.ptr, v.ptr, v.ptr, out.ptr, 2, 6, 8, 12, 12, 12, S) == 0
    torch.cuda.synchronize()
    assert not out.untouched()
