"""The feature-bank kernels one by one against float64 (tests/bank_ref.py): row norms, the split-bf16 image, the statistics
scan and its finish, the stored score tiles, the cosine match (scan and certified), the apply kernels and the read's finish --
every precision and every kernel the launchers can pick, driven through the ctypes descriptors on banks this file lays out
itself: ragged lengths (most bank slices of the short object are empty), more slices than chunks, a one-entry bank, and NaN in
every row past bank_len of every slab the package allocates uninitialised, in all scratch, and a sentinel in the output.  A
NaN or a sentinel that reaches a result is a read of a dead row or a missed write."""
import ctypes as C
import functools

import pytest
import torch

import bank_ref
from bank_ref import CASES, CH, DK, DV, QT, SCALE, THRES, U

pytestmark = pytest.mark.gpu

NAN = float('nan')
SENTINEL = -777.0
LD = DK + DV

# (obj, higher row, lower row, query column, factor): the higher row becomes a bit copy of the lower one and the query column
# factor x that row, so both are the column's best match and the lower index must win
DUPS = {'A': [(0, 700, 3, 5, 0.7), (1, 64, 0, 7, 1.3)], 'B': [(0, 64, 1, 5, 0.7)], 'C': [(0, 199, 64, 2, 0.7)],
        'D': [(1, 128, 0, 4, 0.7)], 'E': [(0, 128, 2, 5, 0.7), (2, 6, 0, 3, 0.7)]}

# name, precision, kept split image, scores stored by the scan, VFN_SCAN_PIPE
SCAN_PATHS = [('f32', 0, False, False, None), ('f32_scores', 0, False, True, None), ('bf16x3', 2, False, False, None),
              ('bf16x3_image', 2, True, False, None), ('bf16', 1, False, False, None), ('bf16_image_pipe', 1, True, False, None),
              ('bf16_image_nopipe', 1, True, False, '0')]
# name, precision, kept split image, scores stored by the scan, VFN_APPLY_PIPE
APPLY_PATHS = [('f32_wide', 0, False, False, None), ('f32_scores', 0, False, True, None), ('bf16x3', 2, False, False, None),
               ('bf16x3_image', 2, True, False, None), ('bf16', 1, False, False, None), ('bf16_image_pipe', 1, True, False, None),
               ('bf16_image_nopipe', 1, True, False, '0')]


def _ids(paths):
    return [p[0] for p in paths]


def _bits(t):
    return t.contiguous().view(torch.int32)


def _report(test, path, case, obj, what, worst):
    print(f'BANKMARGIN {test} {path} {case} obj{obj} {what} {worst:.4f}')


@functools.lru_cache(maxsize=None)
def _inputs(case, dups):
    """The CPU inputs of a case (computed once, never changed)."""
    c = bank_ref.make_case(case)
    if dups:
        c['keys'] = [k.clone() for k in c['keys']]
        c['new'] = c['new'].clone()
        for obj, hi, lo, col, f in DUPS[case]:
            c['keys'][obj][hi] = c['keys'][obj][lo]
            c['new'][obj, col, :DK] = f * c['keys'][obj][lo]
    return c


@functools.lru_cache(maxsize=None)
def _memread_ref(case, obj, precision):
    c = _inputs(case, False)
    return bank_ref.memread(c['keys'][obj], c['vals'][obj], c['q'], precision)


class _Bank:
    """Slabs of one case on the device, laid out and poisoned by the test: rows >= bank_len hold NaN in keys, values, info and
    the norms; counters and images zero-initialised as the package allocates them (feature_bank.py:126,172-175)."""

    def __init__(self, gpu, lens, hw, keys, vals, q, qv, new):
        from vfloodnet_amd import _lib
        self.L, self.lib = _lib, _lib.lib()
        self.gpu, self.lens, self.hw, self.o = gpu, list(lens), hw, len(lens)
        o, cap = self.o, (max(lens) + 65 + 63) // 64 * 64
        self.cap = cap
        self.kbuf = torch.full((o, cap, DK), NAN, device=gpu)
        self.vbuf = torch.full((o, cap, DV), NAN, device=gpu)
        self.ibuf = torch.full((o, cap, 2), NAN, device=gpu)
        for i, n in enumerate(lens):
            self.kbuf[i, :n] = keys[i].to(gpu)
            self.vbuf[i, :n] = vals[i].to(gpu)
            self.ibuf[i, :n, 0] = 3.0
            self.ibuf[i, :n, 1] = 0.25 + 0.125 * (torch.arange(n, device=gpu) % 29).float()
        self.len_dev = torch.tensor(lens, dtype=torch.int32, device=gpu)
        self.knorm = torch.full((o, cap), NAN, device=gpu)
        self.kinv = torch.full((o, cap), NAN, device=gpu)
        self.vnorm = torch.full((o, cap), NAN, device=gpu)
        self.cnt = torch.zeros(o, cap, dtype=torch.int32, device=gpu)
        self.klp = torch.zeros(o * cap * DK * 2 + CH * DK * 2, dtype=torch.int16, device=gpu)
        self.vlp = torch.zeros(o * cap * DV * 2 + CH * DV * 2, dtype=torch.int16, device=gpu)
        self.kvq = torch.cat([q, qv], dim=1).contiguous().to(gpu)                       # [HW][640]: query key | query value
        self.new = new.contiguous().to(gpu)                                             # [obj][HW][640]
        self.work = torch.zeros(4, dtype=torch.int32, device=gpu)

    def call(self, name, *args):
        self.L.check(getattr(self.lib, name)(*args, self.L.stream()), name)

    def norms(self):
        p = self.L.ptr
        self.call('vfn_row_norms', p(self.kbuf), self.cap * DK, DK, DK, p(self.len_dev), 0, self.o, p(self.knorm), p(self.kinv), self.cap)
        self.call('vfn_row_norms', p(self.vbuf), self.cap * DV, DV, DV, p(self.len_dev), 0, self.o, p(self.vnorm), None, self.cap)

    def bank_desc(self):
        p, bd = self.L.ptr, self.L.BankDesc()
        bd.bank_k, bd.bank_v, bd.info = p(self.kbuf), p(self.vbuf), p(self.ibuf)
        bd.bank_len, bd.bank_len_rw = p(self.len_dev), p(self.len_dev)
        bd.stride_k, bd.stride_v, bd.stride_info, bd.stride_n = self.cap * DK, self.cap * DV, self.cap * 2, self.cap
        bd.HW, bd.obj_n, bd.cap = self.hw, self.o, self.cap
        return bd

    def image(self):
        bd = self.bank_desc()
        self.call('vfn_bank_refresh_lp', C.byref(bd), self.L.ptr(self.klp), self.L.ptr(self.vlp), 1)

    def scores_buffer(self):
        stride = (self.cap // CH) * ((self.hw + QT - 1) // QT) * CH * QT
        return torch.full((self.o, stride), NAN, device=self.gpu)

    def scan(self, mode, precision, image, nsplit, scores=None, expect_ok=True):
        """vfn_bank_scan: mode 0 over the frame's queries, mode 1 over the new features with the row scales.  Returns part."""
        p, d = self.L.ptr, self.L.BankScanDesc()
        part = torch.full((self.o, nsplit, self.hw, 2), NAN, device=self.gpu)
        d.bank_k, d.bank_len, d.part = p(self.kbuf), p(self.len_dev), p(part)
        d.stride_k = self.cap * DK
        if mode == 0:
            d.q, d.stride_q, d.q_per_obj, d.scale = p(self.kvq), 0, 0, SCALE
        else:
            d.q, d.stride_q, d.q_per_obj, d.scale = p(self.new), self.hw * LD, 1, 1.0
            d.rowscale, d.stride_rs = p(self.kinv), self.cap
        d.ldq, d.HW, d.obj_n, d.nsplit, d.mode, d.precision = LD, self.hw, self.o, nsplit, mode, precision
        d.work_counter = p(self.work)
        if image:
            d.bank_k_lp = p(self.klp)
        if scores is not None:
            d.scores, d.stride_scores = p(scores), scores.shape[1]
        status = self.lib.vfn_bank_scan(C.byref(d), self.L.stream())
        if not expect_ok:
            return status
        self.L.check(status, 'vfn_bank_scan')
        return part

    def finish_stats(self, part, nsplit):
        ml = torch.full((self.o, self.hw, 2), NAN, device=self.gpu)
        self.call('vfn_bank_scan_finish', self.L.ptr(part), nsplit, self.hw, self.o, 0, self.L.ptr(ml), None, None, None)
        return ml

    def finish_match(self, part, nsplit, colscale):
        idx = torch.full((self.o, self.hw), -1, dtype=torch.int32, device=self.gpu)
        corr = torch.full((self.o, self.hw), NAN, device=self.gpu)
        self.call('vfn_bank_scan_finish', self.L.ptr(part), nsplit, self.hw, self.o, 1, None, self.L.ptr(idx), self.L.ptr(corr),
                  self.L.ptr(colscale))
        return idx, corr

    def new_norms(self):
        """||new key||, its inverse [obj][HW]."""
        p = self.L.ptr
        nrm = torch.full((self.o, self.hw), NAN, device=self.gpu)
        inv = torch.full((self.o, self.hw), NAN, device=self.gpu)
        self.call('vfn_row_norms', p(self.new), self.hw * LD, LD, DK, None, self.hw, self.o, p(nrm), p(inv), self.hw)
        return nrm, inv

    def memread_desc(self, precision, image, nsplit, ml, o_part, out, scores=None, cnt=True, qv=False):
        p, m = self.L.ptr, self.L.MemReadDesc()
        m.q = p(self.kvq)
        m.qv = C.c_void_p(self.kvq.data_ptr() + DK * 4) if qv else None
        m.bank_k, m.bank_v, m.bank_len, m.ml, m.o_part = p(self.kbuf), p(self.vbuf), p(self.len_dev), p(ml), p(o_part)
        m.cnt = p(self.cnt) if cnt else None
        m.info, m.out = p(self.ibuf), p(out)
        m.stride_k, m.stride_v, m.stride_cnt, m.stride_info = self.cap * DK, self.cap * DV, self.cap, self.cap * 2
        m.scale, m.thres = SCALE, THRES
        m.ldq, m.ldqv, m.ld_out, m.HW, m.obj_n, m.nsplit = LD, LD, out.shape[-1], self.hw, self.o, nsplit
        m.precision = precision
        if image:
            m.bank_k_lp, m.bank_v_lp = p(self.klp), p(self.vlp)
        if scores is not None:
            m.scores, m.stride_scores = p(scores), scores.shape[1]
        return m


def _bank(gpu, case, dups=False):
    c = _inputs(case, dups)
    return _Bank(gpu, c['lens'], c['hw'], c['keys'], c['vals'], c['q'], c['qv'], c['new']), c


def _dead_rows_untouched(buf, lens):
    """Rows >= length of a NaN-poisoned [obj][cap]... slab still hold the poison, bit for bit."""
    poison = _bits(torch.full((1,), NAN))[0].item()
    return all(bool((_bits(buf[i, n:]) == poison).all()) for i, n in enumerate(lens))


# ---------------------------------------------------------------------------------------------------------------- norms, image
@pytest.mark.parametrize('case', sorted(CASES))
def test_row_norms(gpu, case):
    """vfn_row_norms on the bank (device lengths; rows >= length keep their poison) and on the key / value halves of a new-feature
    tensor (ld 640, one all-zero row: inverse 1e12), within (dim / 2 + 2) u of the f64 norm."""
    b, c = _bank(gpu, case)
    b.new[0, 1, :DK] = 0.0
    b.norms()
    nk, ik = b.new_norms()
    p = b.L.ptr
    nv = torch.full((b.o, b.hw), NAN, device=gpu)
    b.call('vfn_row_norms', C.c_void_p(b.new.data_ptr() + DK * 4), b.hw * LD, LD, DV, None, b.hw, b.o, p(nv), None, b.hw)
    torch.cuda.synchronize()

    def close(got, x, dim, what, obj):
        ref = bank_ref.row_norms(x)
        v = bank_ref.Violations()
        v.note((got.double().cpu() - ref).abs(), (dim / 2 + 2) * U * ref, what)
        _report('row_norms', what, case, obj, 'norm', v.worst)
        assert v == [], v

    new = b.new.cpu()
    for i, n in enumerate(b.lens):
        close(b.knorm[i, :n], c['keys'][i], DK, 'bank_keys', i)
        close(b.vnorm[i, :n], c['vals'][i], DV, 'bank_values', i)
        close(nk[i], new[i, :, :DK], DK, 'new_keys', i)
        close(nv[i], new[i, :, DK:], DV, 'new_values', i)
        for nrm, inv in ((b.knorm[i, :n], b.kinv[i, :n]), (nk[i], ik[i])):
            want = 1.0 / nrm.double().clamp_min(1e-12)
            assert bool(((inv.double() - want).abs() <= 2 * U * want).all())
    assert float(nk[0, 1]) == 0.0 and float(ik[0, 1]) == float(torch.tensor(1e12, dtype=torch.float32))
    for buf in (b.knorm, b.kinv, b.vnorm):
        assert _dead_rows_untouched(buf, b.lens)


@pytest.mark.parametrize('case', sorted(CASES))
def test_split_image_is_the_host_split(gpu, case):
    """vfn_bank_refresh_lp / _keys (all_rows = 1) against torch's bf16 conversion, bit for bit over the live blocks: ties to even
    (low 16 bits exactly 0x8000 under an even and under an odd bf16), +-0; rows past the length inside the last block are 0, and
    nothing past the last live block is written."""
    b, c = _bank(gpu, case)
    g = torch.Generator().manual_seed(17)
    keys, vals = [k.clone() for k in c['keys']], [v.clone() for v in c['vals']]
    for i, n in enumerate(b.lens):
        for t, dim in ((keys[i], DK), (vals[i], DV)):
            r = n - 1                                                    # the last live row: next to the dead ones
            bits = _bits(torch.randn(32, generator=g))
            bits = (bits & ~0xffff) | 0x8000
            bits[::2] &= ~0x10000                                        # even bf16 above the tie ...
            bits[1::2] |= 0x10000                                        # ... and odd
            t[r, :32] = bits.view(torch.float32)
            t[r, 32:36] = torch.tensor([0.0, -0.0, 0.0, -0.0])
        b.kbuf[i, :n] = keys[i].to(gpu)
        b.vbuf[i, :n] = vals[i].to(gpu)
    b.image()
    konly = torch.zeros_like(b.klp)
    bd = b.bank_desc()
    b.call('vfn_bank_refresh_lp_keys', C.byref(bd), b.L.ptr(konly), 1)
    torch.cuda.synchronize()
    for img in (b.klp, konly):
        assert int(img[b.o * b.cap * DK * 2:].abs().sum()) == 0          # the one-chunk tail
    kimg = [x[:b.o * b.cap * DK * 2].view(b.o, b.cap, 2 * DK).cpu() for x in (b.klp, konly)]
    vimg = b.vlp[:b.o * b.cap * DV * 2].view(b.o, b.cap // 8, 2, DV, 8).cpu()
    assert int(b.vlp[b.o * b.cap * DV * 2:].abs().sum()) == 0
    for i, n in enumerate(b.lens):
        kref, vref = bank_ref.split_image_keys(keys[i]), bank_ref.split_image_values(vals[i])
        nblk = (n + 7) // 8
        for k in kimg:
            assert torch.equal(k[i, :n], kref)
            assert int(k[i, n:].abs().sum()) == 0                        # dead rows were never split: NaN would show as 0x7fc0
        assert torch.equal(vimg[i, :nblk], vref)
        assert int(vimg[i, nblk:].abs().sum()) == 0


# ---------------------------------------------------------------------------------------------------------------- scans
@pytest.mark.parametrize('path', SCAN_PATHS, ids=_ids(SCAN_PATHS))
@pytest.mark.parametrize('case', sorted(CASES))
def test_scan_statistics(gpu, case, path, monkeypatch):
    """vfn_bank_scan (mode 0) + vfn_bank_scan_finish: (m, l) per query within the derived bounds of the f64 statistics; every
    slice partial written (empty slices included); the stored raw scores decoded from their tile layout."""
    name, precision, image, stored, pipe = path
    if pipe is not None:
        monkeypatch.setenv('VFN_SCAN_PIPE', pipe)
    nsplit = CASES[case][2]
    b, c = _bank(gpu, case)
    if image:
        b.image()
    scores = b.scores_buffer() if stored else None
    part = b.scan(0, precision, image, nsplit, scores)
    ml = b.finish_stats(part, nsplit)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part).any())
    assert not bool(torch.isnan(ml).any())
    ml = ml.cpu()
    for i in range(b.o):
        ref = _memread_ref(case, i, precision)
        v = bank_ref.check_stats(ml[i, :, 0], ml[i, :, 1], ref)
        _report('scan_statistics', name, case, i, 'stats', v.worst)
        assert v == [], v
        if stored:
            v = bank_ref.check_scores_tiles(scores[i].cpu(), ref)
            _report('scan_statistics', name, case, i, 'score_tiles', v.worst)
            assert v == [], v


def _match_refs(b, c, precision, nrm_new_inv):
    kinv, cs = b.kinv.cpu(), nrm_new_inv.cpu()
    return [bank_ref.match(c['keys'][i], kinv[i, :n].contiguous(), c['new'][i, :, :DK].contiguous(), cs[i].contiguous(), precision)
            for i, n in enumerate(b.lens)]


def _check_duplicates(case, idx, corr, refs, precision):
    cols = {}
    for obj, hi, lo, col, f in DUPS[case]:
        ref = refs[obj]
        assert int(idx[obj, col]) == lo, (obj, hi, lo, int(idx[obj, col]))
        cosine = float(ref.S[lo, col] * ref.colscale[col])                # the f64 cosine of the operand form, f32 scales
        bound = float((ref.E[lo, col] + 2 * U * abs(ref.S[lo, col])) * ref.colscale[col])
        assert abs(float(corr[obj, col]) - 1.0) <= bound + abs(cosine - 1.0)
        if precision == 0:                                                # exact products: 1 up to the two f32 scales
            assert abs(cosine - 1.0) <= (DK + 6) * U
        cols[obj] = col
    return cols


@pytest.mark.parametrize('path', SCAN_PATHS, ids=_ids(SCAN_PATHS))
@pytest.mark.parametrize('case', sorted(CASES))
def test_scan_match(gpu, case, path, monkeypatch):
    """vfn_bank_scan (mode 1, one query set per object) + vfn_bank_scan_finish against the f64 cosines: the chosen entry within 2E
    of the maximum, corr within its bound, and the lowest index among bit-identical rows -- within a chunk, across chunks and
    across bank slices.  (Stored scores exist in mode 0 only: the launcher must refuse them here.)"""
    name, precision, image, stored, pipe = path
    if pipe is not None:
        monkeypatch.setenv('VFN_SCAN_PIPE', pipe)
    nsplit = CASES[case][2]
    b, c = _bank(gpu, case, dups=True)
    b.norms()
    if stored:
        assert b.scan(1, precision, image, nsplit, b.scores_buffer(), expect_ok=False) != 0
        return
    if image:
        b.image()
    _, colscale = b.new_norms()
    part = b.scan(1, precision, image, nsplit)
    idx, corr = b.finish_match(part, nsplit, colscale)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(part[..., 0]).any())
    idx, corr = idx.cpu(), corr.cpu()
    refs = _match_refs(b, c, precision, colscale)
    for i in range(b.o):
        v = bank_ref.check_match(idx[i], corr[i], refs[i])
        _report('scan_match', name, case, i, 'match', v.worst)
        assert v == [], v
    _check_duplicates(case, idx, corr, refs, precision)


@pytest.mark.parametrize('case', ['A', 'B', 'E'])
def test_certified_match(gpu, case):
    """vfn_bank_match_certified (bf16x3 scores, certification, exact rescoring, f32 scan of the open columns) gives f32 results:
    held to the precision-0 reference, duplicates included (equal best scores cannot be certified and take the f32 path)."""
    nsplit = CASES[case][2]
    b, c = _bank(gpu, case, dups=True)
    b.norms()
    bd = b.bank_desc()
    b.call('vfn_bank_refresh_lp_keys', C.byref(bd), b.L.ptr(b.klp), 1)
    qnorm, colscale = b.new_norms()
    p, o, hw, nfb = b.L.ptr, b.o, b.hw, 3
    part_x3 = torch.full((o, nsplit, hw, 4), NAN, device=gpu)
    part_f32 = torch.full((o, nfb, hw, 2), NAN, device=gpu)
    ulist = torch.full((o, hw), -1, dtype=torch.int32, device=gpu)
    ucount = torch.zeros(o, dtype=torch.int32, device=gpu)
    utotal = torch.zeros(o, dtype=torch.int32, device=gpu)
    idx = torch.full((o, hw), -1, dtype=torch.int32, device=gpu)
    corr = torch.full((o, hw), NAN, device=gpu)
    md = b.L.BankMatchDesc()
    md.q, md.bank_k, md.bank_k_lp, md.bank_len = p(b.new), p(b.kbuf), p(b.klp), p(b.len_dev)
    md.rowscale, md.qnorm, md.colscale = p(b.kinv), p(qnorm), p(colscale)
    md.part_x3, md.part_f32, md.ulist = p(part_x3), p(part_f32), p(ulist)
    md.ucount, md.utotal, md.work_counter = p(ucount), p(utotal), p(b.work)
    md.match_idx, md.match_corr = p(idx), p(corr)
    md.stride_q, md.stride_k, md.stride_rs = hw * LD, b.cap * DK, b.cap
    md.ldq, md.HW, md.obj_n, md.nsplit, md.nsplit_fb = LD, hw, o, nsplit, nfb
    b.call('vfn_bank_match_certified', C.byref(md))
    torch.cuda.synchronize()
    idx, corr, ucount = idx.cpu(), corr.cpu(), ucount.cpu()
    refs = _match_refs(b, c, 0, colscale)
    for i in range(o):
        v = bank_ref.check_match(idx[i], corr[i], refs[i])
        _report('certified_match', 'certified', case, i, 'match', v.worst)
        assert v == [], v
        assert 0 <= int(ucount[i]) <= hw and int(utotal[i]) == int(ucount[i])
    for obj, col in _check_duplicates(case, idx, corr, refs, 0).items():
        assert col in ulist[obj, :int(ucount[obj])].cpu().tolist()      # a tie for the best score is never certified


# ---------------------------------------------------------------------------------------------------------------- apply, finish
def _read(b, path, nsplit_scan, nsplit, monkeypatch, cnt=True):
    """scan + finish -> apply.  Returns (descriptor-independent pieces) ml, o_part, scores, counters after the apply."""
    name, precision, image, stored, pipe = path
    if pipe is not None:
        monkeypatch.setenv('VFN_APPLY_PIPE', pipe)
    scores = b.scores_buffer() if stored else None
    part = b.scan(0, precision, image, nsplit_scan, scores)
    ml = b.finish_stats(part, nsplit_scan)
    o_part = torch.full((b.o, nsplit, b.hw, DV), NAN, device=b.gpu)
    out = torch.full((b.o, b.hw, DV), SENTINEL, device=b.gpu)
    m = b.memread_desc(precision, image, nsplit, ml, o_part, out, scores, cnt=cnt)
    b.call('vfn_memread_apply', C.byref(m))
    torch.cuda.synchronize()
    return ml, o_part, scores, out, m


def _finish(b, precision, image, nsplit, ml, o_part, scores, ld_out, cnt, qv):
    out = torch.full((b.o, b.hw, ld_out), SENTINEL, device=b.gpu)
    m = b.memread_desc(precision, image, nsplit, ml, o_part, out, scores, cnt=cnt, qv=qv)
    b.call('vfn_memread_finish', C.byref(m))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize('path', APPLY_PATHS, ids=_ids(APPLY_PATHS))
@pytest.mark.parametrize('case', sorted(CASES))
def test_apply_and_finish(gpu, case, path, monkeypatch):
    """vfn_bank_scan + finish -> vfn_memread_apply -> vfn_memread_finish per apply kernel: hit counts between `sure` and `sure +
    maybe`, the read-out within the hard f32 bound (precision 0) and the project's tolerances, the info bump from the kernel's own
    count, dead rows and column 0 of info untouched, the counters at rest, and the three call shapes of the finish."""
    name, precision, image, stored, _ = path
    _, hw, nsplit_scan, nsplit = CASES[case]
    b, c = _bank(gpu, case)
    if image:
        b.image()
    info0 = b.ibuf.clone()
    ml, o_part, scores, _, _ = _read(b, path, nsplit_scan, nsplit, monkeypatch)
    assert not bool(torch.isnan(o_part).any())                         # every slice wrote its partial, empty slices zeros
    cnt = b.cnt.cpu()
    refs = [_memread_ref(case, i, precision) for i in range(b.o)]
    for i in range(b.o):
        v = bank_ref.check_hits(cnt[i], refs[i])
        assert v == [], v

    def check_read_out(out, what):
        assert bool(torch.isfinite(out).all())
        for i in range(b.o):
            v = bank_ref.check_out(out[i, :, :DV].cpu(), refs[i], precision)
            for crit, worst in v.parts.items():
                _report('apply_and_finish', name, case, i, f'{what}_{crit}', worst)
            assert v == [], v

    # as the engine calls it: no query values, ld_out 512
    out = _finish(b, precision, image, nsplit, ml, o_part, scores, DV, True, False)
    check_read_out(out, 'out')
    assert int(b.cnt.abs().sum()) == 0
    info1 = b.ibuf.cpu()
    info0c = info0.cpu()
    assert torch.equal(_bits(info1[..., 0]), _bits(info0c[..., 0]))
    for i, n in enumerate(b.lens):
        want = info0c[i, :n, 1].double() + torch.log(cnt[i, :n].double() + 1)
        tol = 4 * U * torch.maximum(want.abs(), torch.ones_like(want))
        assert bool(((info1[i, :n, 1].double() - want).abs() <= tol).all())
        assert torch.equal(_bits(info1[i, n:]), _bits(info0c[i, n:]))
    if name == APPLY_PATHS[0][0]:
        wide = _finish(b, precision, image, nsplit, ml, o_part, scores, DV + 8, False, False)
        assert torch.equal(wide[..., :DV], out) and bool((wide[..., DV:] == SENTINEL).all())

    # with the query values: columns 512..1023 are the query values, 1024.. untouched
    cat = _finish(b, precision, image, nsplit, ml, o_part, scores, 2 * DV + 8, False, True)
    assert torch.equal(cat[..., :DV], out)
    assert torch.equal(_bits(cat[..., DV:2 * DV]), _bits(b.kvq[None, :, DK:].expand(b.o, -1, -1)))
    assert bool((cat[..., 2 * DV:] == SENTINEL).all())
    assert torch.equal(_bits(b.ibuf.cpu()), _bits(info1))

    # without counters (update_bank = False): the same read-out, info and the counters untouched
    _, o_part2, _, _, _ = _read(b, path, nsplit_scan, nsplit, monkeypatch, cnt=False)
    out2 = _finish(b, precision, image, nsplit, ml, o_part2, scores, DV, False, False)
    check_read_out(out2, 'out_nocnt')
    assert int(b.cnt.abs().sum()) == 0
    assert torch.equal(_bits(b.ibuf.cpu()), _bits(info1))


def test_uniform_attention(gpu, monkeypatch):
    """All-zero keys: every score is exactly 0 in every precision, so m = 0, l = B, p = 1 / B.  lens 512 / 72 / 1100, HW 33, integer
    values V[b][c] = ((5b + 3c) mod 17) - 8.  Hit counts are exactly 33 (1 / 512, 1 / 72 > 1e-3) or 0 (1 / 1100 < 1e-3).  Object 0:
    p = 2^-9 and every partial sum is a multiple of 2^-9 below 2^12, exactly representable, so the read-out is sum V / 512 bit for
    bit on every path, whatever the order.  Objects 1 and 2: within check_out's hard bound of the column means.  Plain bf16
    multiplies by bf16(1 / B) by design, 2^-9 relative from 1 / B and far above an f32 bound, so that path is held to the same
    hard bound around the means weighted with bf16(1 / B) (what it must compute), and to the bound plus 2^-9 of the |V|-mass
    around the exact means.  A dropped, doubled or dead row moves a channel by at least 1 / B, orders of magnitude more."""
    lens, hw, nsplit_scan, nsplit = [512, 72, 1100], 33, 3, 4
    g = torch.Generator().manual_seed(sum(lens) + hw)
    q = 2.0 * torch.randn(hw, DK, generator=g)
    qv = torch.randn(hw, DV, generator=g)
    keys = [torch.zeros(n, DK) for n in lens]
    vals = [((5 * torch.arange(n)[:, None] + 3 * torch.arange(DV)[None, :]) % 17 - 8).float() for n in lens]
    new = torch.zeros(len(lens), hw, LD)
    for path in APPLY_PATHS:
        name, precision, image, stored, _ = path
        b = _Bank(gpu, lens, hw, keys, vals, q, qv, new)
        if image:
            b.image()
        with monkeypatch.context() as mp:
            ml, o_part, scores, _, _ = _read(b, path, nsplit_scan, nsplit, mp)
            ml = ml.cpu()
            cnt = b.cnt.cpu()
            out = _finish(b, precision, image, nsplit, ml.to(gpu), o_part, scores, DV, True, False).cpu()
        assert bool(torch.isfinite(out).all()), name
        for i, n in enumerate(lens):
            assert bool((ml[i, :, 0] == 0).all()) and bool((ml[i, :, 1] == n).all()), (name, i)
            assert bool((cnt[i, :n] == (hw if n < 1000 else 0)).all()) and bool((cnt[i, n:] == 0).all()), (name, i)
            ref = bank_ref.memread(keys[i], vals[i], q, 0)
            mean = vals[i].double().sum(dim=0) / n
            assert (ref.out - mean[None, :]).abs().max() <= 1e-12
            if i == 0:
                assert torch.equal(out[i], mean.float()[None, :].expand(hw, -1)), name
                continue
            hard = (ref.rho.max(dim=0).values + (n + 64) * U)[:, None] * ref.absmass + U * ref.out.abs()
            v = bank_ref.Violations()
            if precision == 1:
                pb = torch.tensor(1.0 / n, dtype=torch.float32).bfloat16().double()
                v.note((out[i].double() - (pb * vals[i].double().sum(dim=0))[None, :]).abs(), hard, 'uniform read-out (bf16 p)')
                v.note((out[i].double() - ref.out).abs(), hard + 2.0 ** -9 * ref.absmass, 'uniform read-out')
            else:
                v.note((out[i].double() - ref.out).abs(), hard, 'uniform read-out')
            _report('uniform_attention', name, 'U', i, 'hard', v.worst)
            assert v == [], (name, v)
