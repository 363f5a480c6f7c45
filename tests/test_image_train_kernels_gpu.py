"""The five kernels of ``csrc/image_train.hip`` (include/vfn_image_train.h) one by one against ``tests/linknet_train_ref.py`` in
float64.

Every output buffer holds NaN before the launch; input columns beyond C and rows beyond M hold NaN as well.

The error rule is the one of tests/test_linknet_kernels_gpu.py with the tensor's own scale: the same formula evaluated in
float32 on the CPU lies ``e32 / |ref|max`` from the float64 result (the ratio); a kernel may be 8 x the largest ratio over its
case list away from float64, in units of the case's ``|ref|max`` -- not ``max(1, .)``: these gradients are of order 1e-4 and a
unit floor would make the test vacuous.  Cancelling sums (dbeta, the head's g_b) are nearly zero by construction; their
error is measured in units of the float64 sum of the summands' magnitudes instead."""
import functools
import zlib

import pytest
import torch

import linknet_train_ref as R

pytestmark = pytest.mark.gpu

NAN = float('nan')
FACTOR = 8.0
VFN_ERR_ARG = 1
SHAPES = [(2, 32, 32, 32), (8, 128, 128, 112), (30, 32, 64, 32), (4097, 64, 64, 64), (86528, 32, 32, 32)]     # (M, C, ld, real channels)
GUARD = 3                                                      # rows of NaN behind row M - 1


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) & 0x7FFFFFFF)


def _lib():
    from vfloodnet_amd import _lib
    return _lib


def _padded(t, M, ld):
    """[M, C] -> [M + GUARD, ld] with NaN wherever the kernel has no business reading."""
    out = torch.full((M + GUARD, ld), NAN)
    out[:M, :t.shape[1]] = t
    return out


def _nan(*shape, dtype=torch.float32, dev=None):
    return torch.full(shape, NAN, dtype=dtype, device=dev)


def _dist(got, ref64, scale):
    d = (got.double().cpu() - ref64).abs().max().item()
    return float('inf') if d != d else d / scale


def _hold(name, rows):
    """rows: (case, quantity, float32 distance, kernel distance), both in units of the quantity's scale."""
    bound = {}
    for case, q, e32, _ in rows:
        bound[q] = max(bound.get(q, 0.0), e32)
    worst = {}
    for case, q, _, e in rows:
        if e >= worst.get(q, (-1.0, None))[0]:
            worst[q] = (e, case)
    for q in bound:
        print(f'{name} {q}: float32 ratio {bound[q]:.3e}  bound {FACTOR * bound[q]:.3e}  kernel error {worst[q][0]:.3e} at {worst[q][1]}')
    for q in bound:
        assert worst[q][0] <= FACTOR * bound[q], (name, q, worst[q][1], f'error {worst[q][0]:.3e}', f'bound {FACTOR * bound[q]:.3e}')


# ---------------------------------------------------------------------------------------------------------------- inputs
STAT_CASES = [s + ('plain',) for s in SHAPES] + [(4097, 64, 64, 64, 'offset'), (30, 32, 64, 32, 'constant')]


@functools.lru_cache(maxsize=None)
def _layer(case):
    """x [M, C] f32 with zeros in the padded channels, gamma, beta (zeros in the padding), running statistics."""
    M, C, ld, real, kind = case
    g = _gen('layer', case)
    x = torch.zeros(M, C)
    x[:, :real] = 1.5 * torch.randn(M, real, generator=g) + 0.5 * torch.randn(real, generator=g)
    if kind == 'offset':                                       # channel means 1e3, standard deviation 1e-2
        x[:, :real] = 1e3 * (1 + 0.1 * torch.rand(real, generator=g)) + 1e-2 * torch.randn(M, real, generator=g)
    if kind == 'constant':
        x[:, 3] = 0.75                                         # variance exactly 0
    gamma, beta = torch.zeros(C), torch.zeros(C)
    gamma[:real] = 1 + 0.1 * torch.randn(real, generator=g)
    beta[:real] = 0.1 * torch.randn(real, generator=g)
    rm, rv = torch.zeros(C), torch.zeros(C)
    rm[:real], rv[:real] = 0.2 * torch.randn(real, generator=g), 0.5 + torch.rand(real, generator=g)
    return x, gamma, beta, rm, rv


def _launch_stats(dev, case, M=None):
    L = _lib()
    x, gamma, beta, rm, rv = _layer(case)
    Mx, C, ld = x.shape[0], case[1], case[2]
    M = Mx if M is None else M
    xd = _padded(x, Mx, ld).to(dev)
    out = {k: _nan(C, dev=dev) for k in ('scale', 'shift', 'mean', 'rstd')}
    out['running_mean'], out['running_var'] = rm.to(dev), rv.to(dev)
    part = _nan(L.LNT_MAX_BLOCKS * 2 * C, dtype=torch.float64, dev=dev)
    gd, bd = gamma.to(dev), beta.to(dev)                       # (named: a temporary would be freed before the launch)
    st = L.lib().vfn_lnt_bn_stats_f32(L.ptr(xd), M, C, ld, L.ptr(gd), L.ptr(bd), R.BN_EPS, R.BN_MOMENTUM, L.ptr(part),
                                      L.ptr(out['scale']), L.ptr(out['shift']), L.ptr(out['mean']), L.ptr(out['rstd']),
                                      L.ptr(out['running_mean']), L.ptr(out['running_var']), L.stream())
    torch.cuda.synchronize()
    return st, out


STAT_KEYS = ('mean', 'rstd', 'scale', 'shift', 'running_mean', 'running_var')


def test_statistics(gpu):
    rows = []
    for case in STAT_CASES:
        x, gamma, beta, rm, rv = _layer(case)
        ref = R.bn_stats(x.double(), gamma.double(), beta.double(), rm.double(), rv.double())
        r32 = R.bn_stats(x, gamma, beta, rm, rv)
        st, got = _launch_stats(gpu, case)
        assert st == 0, case
        st2, again = _launch_stats(gpu, case)
        for k in STAT_KEYS:
            assert torch.equal(got[k].view(torch.int32), again[k].view(torch.int32)), (case, k)      # equal inputs, equal bits
            scale = ref[k].abs().max().item()
            rows.append((case, k, _dist(r32[k], ref[k], scale), _dist(got[k], ref[k], scale)))
        real = case[3]
        for k in ('mean', 'scale', 'shift', 'running_mean'):                # padded channels: x = 0, gamma = beta = 0
            assert (got[k][real:] == 0).all(), (case, k)
        if case[4] == 'constant':
            assert got['mean'][3].item() == 0.75 and abs(got['rstd'][3].item() - R.BN_EPS ** -0.5) <= 1e-4 * R.BN_EPS ** -0.5
    _hold('bn_stats', rows)


def test_statistics_of_one_row_are_refused(gpu):
    st, out = _launch_stats(gpu, SHAPES[0] + ('plain',), M=1)
    assert st == VFN_ERR_ARG
    for k in ('scale', 'shift', 'mean', 'rstd'):
        assert torch.isnan(out[k]).all()                                    # nothing was launched
    rm, rv = _layer(SHAPES[0] + ('plain',))[3:]
    assert torch.equal(out['running_mean'].cpu(), rm) and torch.equal(out['running_var'].cpu(), rv)


@functools.lru_cache(maxsize=None)
def _bwd_inputs(shape):
    """The layer's x with the f32 statistics the kernels are handed, a gradient, and exact zeros planted in y: channel 0 has
    scale 0.5 and shift -1, and every third row holds x = 2 there, so fma(x, scale, shift) == 0 and the mask must be off."""
    case = shape + ('plain',)
    x, gamma, beta, rm, rv = _layer(case)
    x = x.clone()
    s = {k: v.float() for k, v in R.bn_stats(x.double(), gamma.double(), beta.double(), rm.double(), rv.double()).items()}
    s['scale'][0], s['shift'][0] = 0.5, -1.0
    x[::3, 0] = 2.0
    g = torch.zeros_like(x)
    g[:, :shape[3]] = 1e-4 * torch.randn(x.shape[0], shape[3], generator=_gen('g', shape))
    return x, g, s


def _bwd_ref(shape, dt):
    x, g, s = _bwd_inputs(shape)
    x, g = x.to(dt), g.to(dt)
    s = {k: v.to(dt) for k, v in s.items()}
    out = {}
    for relu in (True, False):
        dg, db, adg, adb = R.bn_bwd_reduce(g, x, s['scale'], s['shift'], s['mean'], s['rstd'], relu)
        out[relu] = dict(dgamma=dg, dbeta=db, abs_dgamma=adg, abs_dbeta=adb, y=R.bn_apply(x, s['scale'], s['shift'], relu))
    return out


def test_apply(gpu):
    L = _lib()
    rows = []
    for shape in SHAPES:
        M, C, ld, real = shape
        x, g, s = _bwd_inputs(shape)
        ref, r32 = _bwd_ref(shape, torch.float64), _bwd_ref(shape, torch.float32)
        xd, sc, sh = _padded(x, M, ld).to(gpu), s['scale'].to(gpu), s['shift'].to(gpu)
        for relu in (True, False):
            y = _nan(M + GUARD, ld, dev=gpu)
            assert L.lib().vfn_lnt_bn_apply_f32(L.ptr(xd), L.ptr(sc), L.ptr(sh), L.ptr(y), M, C, ld, ld, int(relu), L.stream()) == 0
            torch.cuda.synchronize()
            assert torch.isnan(y[M:]).all() and torch.isnan(y[:M, C:]).all()                 # nothing written outside [M, C]
            scale = ref[relu]['y'].abs().max().item()
            rows.append(((shape, relu), 'y', _dist(r32[relu]['y'], ref[relu]['y'], scale), _dist(y[:M, :C], ref[relu]['y'], scale)))
            if relu:
                assert (y[:M:3, 0] == 0).all() and (y[:M, real:C] == 0).all()                  # planted zeros, padded channels
    _hold('bn_apply', rows)


def _launch_bwd(dev, shape, relu):
    L = _lib()
    M, C, ld, real = shape
    x, g, s = _bwd_inputs(shape)
    xd, gd = _padded(x, M, ld).to(dev), _padded(g, M, ld).to(dev)
    sd = {k: s[k].to(dev) for k in ('scale', 'shift', 'mean', 'rstd')}
    dg, db = _nan(C, dev=dev), _nan(C, dev=dev)
    part = _nan(L.LNT_MAX_BLOCKS * 2 * C, dtype=torch.float64, dev=dev)
    assert L.lib().vfn_lnt_bn_bwd_reduce_f32(L.ptr(gd), L.ptr(xd), L.ptr(sd['scale']), L.ptr(sd['shift']), L.ptr(sd['mean']), L.ptr(sd['rstd']),
                                             M, C, ld, ld, int(relu), L.ptr(part), L.ptr(dg), L.ptr(db), L.stream()) == 0
    gx = _nan(M + GUARD, ld, dev=dev)
    assert L.lib().vfn_lnt_bn_bwd_apply_f32(L.ptr(gd), L.ptr(xd), L.ptr(sd['scale']), L.ptr(sd['shift']), L.ptr(sd['mean']), L.ptr(sd['rstd']),
                                            L.ptr(dg), L.ptr(db), L.ptr(gx), M, C, ld, ld, ld, int(relu), L.stream()) == 0
    torch.cuda.synchronize()
    return dg, db, gx


def test_backward_reduce_and_apply(gpu):
    rows_r, rows_a = [], []
    for shape in SHAPES:
        M, C, ld, real = shape
        x, g, s = _bwd_inputs(shape)
        ref, r32 = _bwd_ref(shape, torch.float64), _bwd_ref(shape, torch.float32)
        for relu in (True, False):
            dg, db, gx = _launch_bwd(gpu, shape, relu)
            dg2, db2, _ = _launch_bwd(gpu, shape, relu)
            assert torch.equal(dg.view(torch.int32), dg2.view(torch.int32)) and torch.equal(db.view(torch.int32), db2.view(torch.int32))
            case = (shape, relu)
            rf, rs = ref[relu], r32[relu]
            for k in ('dgamma', 'dbeta'):                       # dbeta cancels (zero-mean g): in units of the sum of its summands' magnitudes
                scale = rf['abs_dbeta'].max().item() if k == 'dbeta' else rf[k].abs().max().item()
                rows_r.append((case, k, _dist(rs[k], rf[k], scale), _dist(dg if k == 'dgamma' else db, rf[k], scale)))
            assert (dg[real:] == 0).all() and (db[real:] == 0).all()
            # the apply kernel read the KERNEL's dgamma / dbeta: its reference does the same
            args = lambda dt: (g.to(dt), x.to(dt), *(s[k].to(dt) for k in ('scale', 'shift', 'mean', 'rstd')), dg.cpu().to(dt), db.cpu().to(dt), relu)
            want, w32 = R.bn_bwd_apply(*args(torch.float64)), R.bn_bwd_apply(*args(torch.float32))
            scale = want.abs().max().item()
            rows_a.append((case, 'gx', _dist(w32, want, scale), _dist(gx[:M, :C], want, scale)))
            assert torch.isnan(gx[M:]).all() and torch.isnan(gx[:M, C:]).all() and (gx[:M, real:C] == 0).all()
    _hold('bn_bwd_reduce', rows_r)
    _hold('bn_bwd_apply', rows_a)


# ------------------------------------------------------------------------------------------------------------------ head
HEAD_CASES = [(2, 32), (30, 64), (4097, 32), (86528, 32)]      # (M, ld)


@functools.lru_cache(maxsize=None)
def _head_inputs(case):
    M, ld = case
    g = _gen('head', case)
    x = torch.relu(torch.randn(M, 32, generator=g))             # a ReLU output: exact zeros
    w = 0.3 * torch.randn(32, generator=g)
    pr = torch.sigmoid(x @ w + 0.1)
    gt = (torch.rand(M, generator=g) > 0.6).float()
    sums = torch.stack(R.dice_sums(pr.double(), gt.double()))
    return x, w, pr, gt, sums


def _launch_head(dev, case):
    L = _lib()
    M, ld = case
    x, w, pr, gt, sums = _head_inputs(case)
    guard = lambda v: torch.cat([v, torch.full((GUARD,), NAN)]).to(dev)
    gx, gw, gb = _nan(M + GUARD, 32, dev=dev), _nan(32, dev=dev), _nan(1, dev=dev)
    part = _nan(L.LNT_MAX_BLOCKS * 36, dtype=torch.float64, dev=dev)
    sums5 = torch.cat([sums, torch.full((2,), NAN, dtype=torch.float64)]).to(dev)
    xd, wd, prd, gtd = _padded(x, M, ld).to(dev), w.to(dev), guard(pr), guard(gt)      # (named: alive until the launch has run)
    assert L.lib().vfn_lnt_head_bwd_f32(L.ptr(xd), L.ptr(wd), L.ptr(prd), L.ptr(gtd), L.ptr(sums5), M, ld,
                                        L.ptr(part), L.ptr(gx), L.ptr(gw), L.ptr(gb), L.stream()) == 0
    torch.cuda.synchronize()
    return gx, gw, gb


def test_head_backward(gpu):
    rows = []
    for case in HEAD_CASES:
        M, ld = case
        x, w, pr, gt, sums = _head_inputs(case)
        rx, rw, rb, rabs = R.head_bwd(x.double(), w.double(), pr.double(), gt.double(), tuple(sums))
        fx, fw, fb, _ = R.head_bwd(x, w, pr, gt, tuple(sums.float()))
        gx, gw, gb = _launch_head(gpu, case)
        gx2, gw2, gb2 = _launch_head(gpu, case)
        assert torch.equal(gw.view(torch.int32), gw2.view(torch.int32)) and torch.equal(gb.view(torch.int32), gb2.view(torch.int32))
        assert torch.isnan(gx[M:]).all()
        sx = rx.abs().max().item()
        rows.append((case, 'g_x', _dist(fx, rx, sx), _dist(gx[:M], rx, sx)))
        sw = rw.abs().max().item()
        rows.append((case, 'g_w', _dist(fw, rw, sw), _dist(gw, rw, sw)))
        rows.append((case, 'g_b', _dist(fb.reshape(1), rb.reshape(1), rabs.item()), _dist(gb, rb.reshape(1), rabs.item())))
    _hold('head_bwd', rows)


def test_arguments_are_checked(gpu):
    L = _lib()
    t = torch.zeros(64, 32, device=gpu)
    v = torch.zeros(32, device=gpu)
    part = torch.zeros(L.LNT_MAX_BLOCKS * 2 * 32, dtype=torch.float64, device=gpu)
    p, s, lib = L.ptr, L.stream(), L.lib()
    assert lib.vfn_lnt_bn_apply_f32(p(t), p(v), p(v), p(t), 64, 30, 32, 32, 1, s) == VFN_ERR_ARG              # C % 4
    assert lib.vfn_lnt_bn_apply_f32(p(t), p(v), p(v), p(t), 64, 32, 30, 32, 1, s) == VFN_ERR_ARG              # ld < C
    assert lib.vfn_lnt_bn_apply_f32(p(t), p(v), p(v), None, 64, 32, 32, 32, 1, s) == VFN_ERR_ARG
    assert lib.vfn_lnt_bn_apply_f32(p(t), p(v), p(v), p(t), 0, 32, 32, 32, 1, s) == VFN_ERR_ARG
    assert lib.vfn_lnt_bn_bwd_reduce_f32(p(t), p(t), p(v), p(v), p(v), p(v), 64, 32, 32, 34, 1, p(part), p(v), p(v), s) == VFN_ERR_ARG   # ld % 4
    assert lib.vfn_lnt_bn_bwd_apply_f32(p(t), p(t), p(v), p(v), p(v), p(v), p(v), p(v), p(t), 64, 2048, 2048, 2048, 2048, 1, s) == VFN_ERR_ARG
    assert lib.vfn_lnt_head_bwd_f32(p(t), p(v), p(v), p(v), None, 64, 32, p(part), p(t), p(v), p(v), s) == VFN_ERR_ARG
    torch.cuda.synchronize()
    assert (t == 0).all()
