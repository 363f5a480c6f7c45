"""vfn_memread_desc.nsplit_tail: the last query tile of the f32 stored-scores apply kernel in its own number of bank slices, its
dead 32-column groups skipped.  Scan, scan finish, apply and finish driven through the descriptors on the poisoned banks of
tests/test_bank_kernels_gpu.py (NaN past bank_len, NaN in o_part, a sentinel in out), against the float64 reference and the
derived f32 bound of tests/bank_ref.py.  HW 148 / 168 / 212 give a last tile of 1 / 2 / 3 live groups, 256 none; object 0 of the
short bank has 2 chunks, fewer than the 3 tail slices of two of the pairs."""
import ctypes as C
import functools

import pytest
import torch

import bank_ref
from bank_ref import CH, DK, DV, QT
from test_bank_kernels_gpu import NAN, SENTINEL, _Bank, _bits

pytestmark = pytest.mark.gpu

HWS = [148, 168, 212, 256]
LENS = [(65, 200), (1000, 777)]
PAIRS = [(3, 3), (4, 3), (5, 2), (2, 1)]
NSPLIT_SCAN = 3
POISON = _bits(torch.full((1,), NAN))[0].item()


@functools.lru_cache(maxsize=None)
def _inputs(lens, hw):
    g = torch.Generator().manual_seed(sum(lens) + hw)
    q = 2.0 * torch.randn(hw, DK, generator=g)
    keys = [torch.randn(n, DK, generator=g) for n in lens]
    vals = [torch.randn(n, DV, generator=g) for n in lens]
    qv = torch.randn(hw, DV, generator=g)
    new = torch.zeros(len(lens), hw, DK + DV)
    return q, keys, vals, qv, new


@functools.lru_cache(maxsize=None)
def _ref(lens, hw, obj):
    q, keys, vals, _, _ = _inputs(lens, hw)
    return bank_ref.memread(keys[obj], vals[obj], q, 0)


def _statistics(gpu, lens, hw):
    """The bank, the stored scores and (m, l) of the frame."""
    q, keys, vals, qv, new = _inputs(lens, hw)
    b = _Bank(gpu, lens, hw, keys, vals, q, qv, new)
    scores = b.scores_buffer()
    part = b.scan(0, 0, False, NSPLIT_SCAN, scores)
    ml = b.finish_stats(part, NSPLIT_SCAN)
    return b, scores, ml


def _read(b, scores, ml, nsplit, nsplit_tail, ld_out=DV):
    """apply + finish with the given slices.  Returns o_part, the hit counters of the apply, out.  The finish runs without the
    counters (no info bump); the counters are put back to zero here."""
    o_part = torch.full((b.o, nsplit, b.hw, DV), NAN, device=b.gpu)
    out = torch.full((b.o, b.hw, ld_out), SENTINEL, device=b.gpu)
    m = b.memread_desc(0, False, nsplit, ml, o_part, out, scores, cnt=True)
    m.nsplit_tail = nsplit_tail
    b.call('vfn_memread_apply', C.byref(m))
    torch.cuda.synchronize()
    cnt = b.cnt.clone()
    b.cnt.zero_()
    m = b.memread_desc(0, False, nsplit, ml, o_part, out, scores, cnt=False)
    m.nsplit_tail = nsplit_tail
    b.call('vfn_memread_finish', C.byref(m))
    torch.cuda.synchronize()
    return o_part, cnt, out


def _empty_from(n, slices):
    """First slice of `slices` that gets no chunk of an n-entry bank (chunk_range of memory_read.hip)."""
    nchunks = (n + CH - 1) // CH
    per = (nchunks + slices - 1) // slices
    return (nchunks + per - 1) // per


@pytest.mark.parametrize('pair', PAIRS, ids=lambda p: f's{p[0]}t{p[1]}')
@pytest.mark.parametrize('lens', LENS, ids=lambda l: f'b{l[0]}_{l[1]}')
@pytest.mark.parametrize('hw', HWS)
def test_tail_slices(gpu, hw, lens, pair):
    nsplit, tail = pair
    b, scores, ml = _statistics(gpu, lens, hw)
    o_u, cnt_u, out_u = _read(b, scores, ml, nsplit, 0)
    o_t, cnt_t, out_t = _read(b, scores, ml, nsplit, tail, ld_out=DV + 8)
    refs = [_ref(lens, hw, i) for i in range(b.o)]
    assert not bool(torch.isnan(o_u).any())
    for i in range(b.o):                                               # the uniform launch is the kernel the suite already holds
        assert bank_ref.check_hits(cnt_u[i].cpu(), refs[i]) == []
    assert torch.equal(cnt_t, cnt_u)                                   # hit counts do not depend on the slicing
    assert bool((out_t[..., DV:] == SENTINEL).all())                   # nothing past the read-out's 512 columns
    out_t = out_t[..., :DV].contiguous()
    assert bool(torch.isfinite(out_t).all())
    last_q0 = (hw - 1) // QT * QT
    if tail == nsplit:
        # the same slices, dead column groups skipped: every bit as the uniform launch
        assert torch.equal(_bits(o_t), _bits(o_u))
        assert torch.equal(_bits(out_t), _bits(out_u))
        return
    for i in range(b.o):
        v = bank_ref.check_out(out_t[i].cpu(), refs[i], 0)
        for crit, worst in v.parts.items():
            print(f'TAILMARGIN hw{hw} lens{lens} pair{pair} obj{i} {crit} {worst:.4f}')
        assert v == [], v
    assert torch.equal(_bits(o_t[:, :, :last_q0]), _bits(o_u[:, :, :last_q0]))         # the full tiles: same slices, same bits
    assert bool((_bits(o_t[:, tail:, last_q0:]) == POISON).all())     # slabs the last tile does not own: never written
    assert not bool(torch.isnan(o_t[:, :tail, last_q0:]).any())
    for i, n in enumerate(lens):
        assert bool((o_t[i, _empty_from(n, tail):tail, last_q0:] == 0).all())           # empty slices write zeros
        assert bool((o_t[i, _empty_from(n, nsplit):, :last_q0] == 0).all())


def test_refusals(gpu):
    lens, hw = LENS[0], 212
    b, scores, ml = _statistics(gpu, lens, hw)
    b.image()
    o_part = torch.full((b.o, 4, hw, DV), NAN, device=gpu)
    out = torch.full((b.o, hw, DV), SENTINEL, device=gpu)

    def status(entry, precision, image, with_scores, nsplit_tail):
        m = b.memread_desc(precision, image, 4, ml, o_part, out, scores if with_scores else None, cnt=False)
        m.nsplit_tail = nsplit_tail
        return getattr(b.lib, entry)(C.byref(m), b.L.stream())

    assert status('vfn_memread_apply', 1, True, False, 3) != 0         # reduced precision
    assert status('vfn_memread_apply', 2, True, False, 3) != 0
    assert status('vfn_memread_apply', 1, False, False, 3) != 0
    assert status('vfn_memread_apply', 0, False, False, 3) != 0        # f32 without stored scores
    assert status('vfn_memread_apply', 0, False, True, -1) != 0
    assert status('vfn_memread_apply', 0, False, True, 5) != 0         # more than nsplit
    assert status('vfn_memread_finish', 0, False, True, -1) != 0
    assert status('vfn_memread_finish', 0, False, True, 5) != 0
    torch.cuda.synchronize()
    assert bool((_bits(o_part) == POISON).all()) and bool((out == SENTINEL).all())     # a refused call launches nothing
    assert status('vfn_memread_apply', 0, False, True, 3) == 0
    assert status('vfn_memread_finish', 2, True, False, 3) == 0        # the finish only sums slabs: any precision
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
