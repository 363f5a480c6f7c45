"""Float64 references, derived error bounds and checkers for the feature-bank kernels (csrc/memory_read.hip, csrc/bank.hip):
the memory read (scan, apply, finish), the cosine match of FeatureBank.update, the row norms and the split-bf16 image.
Plain torch on the CPU; no GPU import.  tests/test_bank_ref_host.py holds the references to the oracle and feeds the checkers
wrong data; tests/test_bank_kernels_gpu.py holds the kernels to them.

References
    scores(keys, q, precision)   S[b, q] = <k_b, q> in f64 from the f32 inputs, in the operand form of the precision:
                                 0 the exact products; 1 products of bf16-rounded operands; 2 (bf16x3) (kh + kl)(qh + ql) - kl ql
                                 with h = RNE bf16(x), l = RNE bf16(x - h) -- the three products the kernels form.  Also
                                 A[b, q] = sum |k^||q^| over the same operand forms (the terms the kernel adds up).
    memread(...)                 softmax statistics per query (m, lse), the probabilities p, the read-out P^T V, P^T |V|.
    match(...)                   S * rowscale[b] and its abs-product mass.
    row_norms, split_image_keys, split_image_values

Error bounds (derived, not measured).  u = 2^-24, the unit roundoff of f32 round-to-nearest.

  Score.  A kernel forms a score as a sum of n products accumulated in f32 by the matrix cores: n = 128 for precision 0 (one fused
  multiply-add per term) and for precision 1 (a product of two bf16 numbers has 16 significant bits: exact in f32), n = 384 for
  precision 2 (three exact products per channel).  Whatever the order of the additions -- the MFMA's internal one, k in any
  grouping -- the computed sum s^ of n terms t_i with one rounding per addition satisfies |s^ - sum t_i| <= (n - 1) u sum|t_i|
  to first order (Higham, Accuracy and Stability, 4.4: the bound holds for every summation order); the product roundings of
  precision 0 are inside the fused operations.  One more rounding multiplies by `scale` (or by rowscale[b] in the match), and one
  more unit covers the second-order terms ((1 + u)^n - 1 <= (n + 1) u for n u < 0.01).  Hence
        ds(b, q) = (n + 2) u scale A(b, q)          (match: E(b, q) = (n + 2) u rowscale[b] A(b, q)).

  Statistics.  m^ is the maximum of computed scores, so |m^ - m| <= max_b ds.  With x^ = s^ - m^ the kernel sums e^ = exp(x^)
  over B entries in slices and folds them with factors exp(m_slice - m^); exp(x^) differs from exp(s - m) by the relative
  |x^ - x| <= 2 max ds, every exp (hardware v_exp_f32 on the f32 product x log2(e), memory_read.hip:144) by (|x| + 4) 2u
  relative (u |x| for the product, 1 ulp = 2u for the exp2, the rest for the subtraction and the rescale), and a sum of B
  non-negative terms in any order by (B - 1) u relative.  For  log l^ + m^  against  lse = log sum exp(s):  the shift m^ cancels
  between the two, what remains is the relative error of the sum of exp(s^ - m^): every term within 2 max ds (its own score
  error, and none from m^ because it cancels exactly in exact arithmetic -- kept at 2 max ds for the fold factors, which use
  slice maxima), (B + 4) u for the exps near x = 0 that carry the sum and the B additions; 4u |lse| for the final f32 values of
  m^ and log l^ as stored.  So
        |m^ - m| <= max ds,        |m^ + log l^ - lse| <= 2 max ds + (B + 4) u + 4u |lse|.

  Probability.  p^ = exp(s^ - m^) / l^:
        rho(b, q) = 2 max_b ds(., q) + (|x| + 4) 2u + (B + 2) u,      x = s - m,
  the three terms being: numerator and sum cancel only up to the score errors; the exp; the sum l of B terms and the reciprocal /
  product.  Any summation order, including the MFMA's and the slice folds, satisfies these bounds.

  Read-out (precision 0).  out^ = sum_b p^ V in f32 on the matrix cores, per slice, the slices added by the finish kernel:
  |out^ - out| <= max_b rho * sum p |V| (the probabilities) + (B + 64) u sum p |V| (B products and additions, up to 20 slice
  additions and second-order terms well inside the 64) + u |out| (the final store):
        |out^ - out| <= (max_b rho + (B + 64) u) absmass + u |out|.
  For precision 1 / 2 the probabilities and values are rounded / split to bf16 before the second contraction; the emulated
  read-out repeats exactly that in f64 and the project's own tolerances against it apply (tests/test_kernels_gpu.py:179,234,236).
  One thing the emulation cannot know: plain bf16 rounds the kernel's own p^ to 8 bits, and where p sits within rho p of the
  midpoint of two bf16 numbers, p^ may round to the other one -- a step of 2^-8 p in one operand, |V| / 256 of that entry's
  weight in the result (seen on case A: p = 0.01727, 2.4e-7 from a midpoint, moved three channels by 4.5e-4 against a
  tolerance of 3.5e-4 on all three bf16 kernels alike).  Both roundings are correct, so check_out lets exactly those entries
  take their other rounding (bf16_ties, _settle_bf16_ties) and then applies the unchanged tolerance.  In bf16x3 the low part
  absorbs the step (hi + lo is the same to 2^-17 either way): nothing to settle.

  Hit counts.  p^ > thres is certain when p > thres (1 + rho) and impossible when p < thres (1 - rho); in between (`maybe`) either
  answer is right:   sure <= cnt <= sure + maybe.

  Norms.  dim squares (one rounding each, as fused operations) and dim - 1 additions in a tree of depth <= log2(dim) + 2 plus the
  square root: relative error of the sum of squares <= (dim + 2) u, of its root half that, + u for the root itself:
  (dim / 2 + 2) u.

Checkers return a list of violations (strings), empty when the check passes; the list carries ``worst``, the largest observed
error as a fraction of its bound, for reports.
"""
import math

import torch

U = 2.0 ** -24
DK, DV, CH, QT = 128, 512, 64, 128
SCALE = 1.0 / math.sqrt(DK)
THRES = 1e-3
TERMS = {0: 128, 1: 128, 2: 384}          # additions per score

# lens, HW, bank slices of the scan, bank slices of the apply kernels
CASES = {
    'A': ([1000, 72], 157, 9, 3),
    'B': ([65, 8], 129, 2, 2),
    'C': ([200, 1], 33, 4, 4),
    'D': ([640, 129], 128, 1, 20),
    'E': ([129, 64, 7], 60, 2, 2),
}


def make_case(name):
    """The inputs of a case: queries [HW][128] (2 N(0,1)), per object keys [B][128] and values [B][512] (N(0,1)), query values
    [HW][512], new features for the match [obj][HW][640].  Seed sum(lens) + HW, queries drawn before keys."""
    lens, hw, _, _ = CASES[name]
    g = torch.Generator().manual_seed(sum(lens) + hw)
    q = 2.0 * torch.randn(hw, DK, generator=g)
    keys = [torch.randn(n, DK, generator=g) for n in lens]
    vals = [torch.randn(n, DV, generator=g) for n in lens]
    qv = torch.randn(hw, DV, generator=g)
    new = torch.randn(len(lens), hw, DK + DV, generator=g)
    return dict(lens=lens, hw=hw, q=q, keys=keys, vals=vals, qv=qv, new=new)


class Violations(list):
    """A list of violation messages; ``worst`` = largest error / bound seen (0 when nothing was compared)."""
    worst = 0.0

    def note(self, err, bound, what):
        """err, bound: tensors of one shape.  Records every element with err > bound (NaN counts as a violation)."""
        err, bound = err.double().reshape(-1), bound.double().reshape(-1)
        if err.numel() == 0:
            return
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
        ratio = torch.where(torch.isnan(err) | torch.isnan(bound), torch.full_like(err, float('inf')), ratio)
        self.worst = max(self.worst, float(ratio.max()))
        bad = (ratio > 1).nonzero().reshape(-1)
        if bad.numel():
            i = int(bad[ratio[bad].argmax()])
            self.append(f'{what}: {bad.numel()} of {err.numel()} outside the bound; worst at flat index {i}: '
                        f'error {float(err[i]):.3e}, bound {float(bound[i]):.3e}')


class Ref(dict):
    __getattr__ = dict.__getitem__


def _rb(x):
    return x.bfloat16().float()


def _split(x):
    h = _rb(x)
    return h, _rb(x - h)


def scores(keys, q, precision):
    """keys [B][128], q [HW][128] f32 -> S [B][HW] f64 (unscaled), A [B][HW] f64 = sum of the magnitudes of the terms."""
    assert keys.dtype == torch.float32 and q.dtype == torch.float32
    if precision == 0:
        k, x = keys.double(), q.double()
        return k @ x.t(), k.abs() @ x.abs().t()
    if precision == 1:
        k, x = _rb(keys).double(), _rb(q).double()
        return k @ x.t(), k.abs() @ x.abs().t()
    kh, kl = [t.double() for t in _split(keys)]
    qh, ql = [t.double() for t in _split(q)]
    s = (kh + kl) @ (qh + ql).t() - kl @ ql.t()
    a = (kh.abs() + kl.abs()) @ (qh.abs() + ql.abs()).t() - kl.abs() @ ql.abs().t()
    return s, a


def _mm_reduced(a, b, precision):
    """As tests/test_kernels_gpu.py::_mm_reduced: the f64 value of the reduced-precision contraction of f32 a, b."""
    if precision == 1:
        return _rb(a).double() @ _rb(b).double()
    ah, al = [t.double() for t in _split(a)]
    bh, bl = [t.double() for t in _split(b)]
    return (ah + al) @ (bh + bl) - al @ bl


def memread(keys, vals, q, precision, scale=SCALE, thres=THRES):
    """One object's memory read.  keys [B][128], vals [B][512], q [HW][128], all f32."""
    B, hw = keys.shape[0], q.shape[0]
    S, A = scores(keys, q, precision)
    s = S * scale
    ds = (TERMS[precision] + 2) * U * scale * A
    m = s.max(dim=0).values
    x = s - m
    e = torch.exp(x)
    lsum = e.sum(dim=0)
    p = e / lsum
    lse = m + torch.log(lsum)
    dsmax = ds.max(dim=0).values
    rho = 2 * dsmax + (x.abs() + 4) * 2 * U + (B + 2) * U
    v = vals.double()
    r = Ref(B=B, HW=hw, precision=precision, scale=scale, thres=thres, S=S, A=A, s=s, ds=ds, dsmax=dsmax, m_ref=m, lse_ref=lse,
            p=p, rho=rho, out=p.t() @ v, absmass=p.t() @ v.abs(), vals=vals)
    if precision:
        r['emulated'] = _mm_reduced(p.float().t().contiguous(), vals, precision)
        r['exact'] = memread(keys, vals, q, 0, scale, thres).out
    else:
        r['emulated'], r['exact'] = r.out, r.out
    r['sure'] = (p > thres * (1 + rho)).sum(dim=1)
    r['maybe'] = ((p - thres).abs() <= thres * rho).sum(dim=1)
    return r


def match(keys, rowscale, q, colscale, precision):
    """The cosine match of one object: S[b][q] = <k_b, q> rowscale[b] in f64, E its bound; keys [B][128], rowscale [B], q
    [HW][128], colscale [HW] (f32, as the kernel reads them)."""
    S, A = scores(keys, q, precision)
    rs = rowscale.double()[:, None]
    return Ref(B=keys.shape[0], HW=q.shape[0], precision=precision, S=S * rs, mass=A * rs.abs(),
               E=(TERMS[precision] + 2) * U * A * rs.abs(), colscale=colscale.double(),
               rowbits=torch.cat([keys.contiguous().view(torch.int32), rowscale.contiguous().view(torch.int32)[:, None]], dim=1))


def row_norms(x):
    """x [rows][dim] f32 -> ||x_r|| in f64."""
    return x.double().pow(2).sum(dim=1).sqrt()


def split_image_keys(keys):
    """keys [rows][128] f32 -> int16 [rows][256]: per row [128 hi | 128 lo] bf16 bit patterns (include/vfn_hip.h:582-590)."""
    h = keys.bfloat16()
    l = (keys - h.float()).bfloat16()
    return torch.cat([h.view(torch.int16), l.view(torch.int16)], dim=1)


def split_image_values(vals):
    """vals [B][512] f32 -> int16 [ceil(B/8)][2][512][8]: blocks of 8 rows, [hi plane | lo plane][channel][row in block] bf16;
    rows past B inside the last block are 0."""
    B = vals.shape[0]
    nblk = (B + 7) // 8
    pad = torch.zeros(nblk * 8, DV)
    pad[:B] = vals
    h = pad.bfloat16()
    l = (pad - h.float()).bfloat16()
    planes = torch.stack([h.view(torch.int16), l.view(torch.int16)], dim=0)            # [2][rows][512]
    return planes.view(2, nblk, 8, DV).permute(1, 0, 3, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------- score tiles
def _tile_shape(B_rows, hw):
    return (B_rows + CH - 1) // CH, (hw + QT - 1) // QT


def scores_from_tiles(buf, B, hw):
    """Decode vfn_bankscan_desc.scores of one object (include/vfn_hip.h:464-470): one 8192-float tile per (64-entry chunk c,
    128-query tile t) at tile index c * ceil(HW/128) + t, laid out [key half 2][row group 4][lane half 2][query 128][4]; entry =
    64c + 32 half + 8 group + 4 lane half + j.  Returns [B][HW]."""
    nch, nqt = _tile_shape(B, hw)
    t = buf.reshape(-1)[:nch * nqt * CH * QT].view(nch, nqt, 2, 4, 2, QT, 4)
    t = t.permute(0, 2, 3, 4, 6, 1, 5).reshape(nch * CH, nqt * QT)           # [c, half, group, lane half, j][t, query]
    return t[:B, :hw]


def scores_to_tiles(S, fill=float('nan')):
    """The inverse, for the host tests: S [B][HW] -> the flat tile buffer (rows / columns outside S hold ``fill``)."""
    B, hw = S.shape
    nch, nqt = _tile_shape(B, hw)
    full = torch.full((nch * CH, nqt * QT), fill, dtype=S.dtype)
    full[:B, :hw] = S
    return full.view(nch, 2, 4, 2, 4, nqt, QT).permute(0, 5, 1, 2, 3, 6, 4).contiguous().reshape(-1)


# ---------------------------------------------------------------------------------------------------------------- checkers
def check_stats(m, l, ref):
    """m, l [HW] from vfn_bank_scan_finish (mode 0) against a memread reference."""
    v = Violations()
    m, l = m.double(), l.double()
    v.note((m - ref.m_ref).abs(), ref.dsmax, 'm')
    bound = 2 * ref.dsmax + (ref.B + 4) * U + 4 * U * ref.lse_ref.abs()
    v.note((m + torch.log(l) - ref.lse_ref).abs(), bound, 'm + log l')
    return v


def check_scores_tiles(buf, ref):
    """The stored raw scores of one object: every live row, every column < HW."""
    v = Violations()
    got = scores_from_tiles(buf, ref.B, ref.HW).double()
    v.note((got - ref.S).abs(), ref.ds / ref.scale, 'stored scores')
    return v


def check_match(idx, corr, ref):
    """idx, corr [HW] from the match kernels against a match reference."""
    v = Violations()
    idx = idx.long()
    inside = (idx >= 0) & (idx < ref.B)
    if not bool(inside.all()):
        v.append(f'idx outside [0, {ref.B}): {idx[~inside].tolist()[:8]}')
        v.worst = float('inf')
        return v
    cols = torch.arange(ref.HW)
    S_at, E_at = ref.S[idx, cols], ref.E[idx, cols]
    best = ref.S.max(dim=0)
    v.note(best.values - S_at, E_at + ref.E[best.indices, cols], 'arg-max score below the maximum')
    v.note((corr.double() - S_at * ref.colscale).abs(), (E_at + 2 * U * S_at.abs()) * ref.colscale, 'corr')
    for i in idx.unique().tolist():                      # bit-identical rows: the lowest index wins
        first = int((ref.rowbits == ref.rowbits[i]).all(dim=1).nonzero()[0])
        if first != i:
            v.append(f'idx {i} chosen although row {first} holds the same bits')
            v.worst = float('inf')
    return v


def check_hits(cnt, ref):
    """cnt [>= B] int: the hit counters of one object after vfn_memread_apply."""
    v = Violations()
    cnt = cnt.long()
    live = cnt[:ref.B]
    low, high = live < ref.sure, live > ref.sure + ref.maybe
    if bool((low | high).any()):
        b = int((low | high).nonzero()[0])
        v.append(f'hit counts: {int((low | high).sum())} entries outside [sure, sure + maybe]; entry {b}: {int(live[b])} '
                 f'not in [{int(ref.sure[b])}, {int(ref.sure[b] + ref.maybe[b])}]')
        v.worst = float('inf')
    if bool((cnt[ref.B:] != 0).any()):
        v.append(f'hit counts of dead rows: {int((cnt[ref.B:] != 0).sum())} are not 0')
        v.worst = float('inf')
    return v


def bf16_ties(ref):
    """Where the plain-bf16 rounding of a probability is not decided by the reference: the kernel rounds ITS p^, which lies within
    rho p of p; if the midpoint between bf16(p) and its neighbour on p's side lies that close, the neighbour is as correct a
    rounding as bf16(p).  Returns (ambiguous [B][HW] bool, step [B][HW] f64 = neighbour - bf16(p))."""
    h = ref.p.float().bfloat16()
    bits = h.view(torch.int16).to(torch.int32)
    up = ref.p > h.double()
    nb = torch.where(up, bits + 1, bits - 1).to(torch.int16).view(torch.bfloat16).double()
    hd = h.double()
    usable = (bits > 0) & (bits < 0x7f7f)                      # positive, finite, not the smallest: p is a probability
    mid = 0.5 * (hd + nb)
    amb = usable & ((ref.p - mid).abs() <= ref.rho * ref.p)
    return amb, torch.where(usable, nb - hd, torch.zeros_like(hd))


def _settle_bf16_ties(resid, ref, tol):
    """resid [HW][512] = read-out - emulation.  For every query whose residual exceeds ``tol``, take the other rounding of
    ambiguous probabilities (bf16_ties) one at a time, greedily, as long as it shrinks the residual's 2-norm: rounding entry b of
    query q the other way moves the emulated read-out of q by step[b, q] * bf16(V[b]) in all 512 channels at once, so a single
    tie is identified by 512 numbers.  Only ambiguous entries may move, each once and by its one step, and the tolerance the
    residual must meet afterwards is unchanged: a wrong kernel finds no excuse here.  Returns (residual, ties taken)."""
    amb, step = bf16_ties(ref)
    V = _rb(ref.vals).double()
    resid = resid.clone()
    taken = 0
    for q in (resid.abs().max(dim=1).values > tol).nonzero().reshape(-1).tolist():
        cand = amb[:, q].nonzero().reshape(-1)
        r = resid[q]
        for _ in range(int(cand.numel())):
            if cand.numel() == 0 or float(r.abs().max()) <= tol:
                break
            d = step[cand, q]
            gain = 2 * d * (V[cand] @ r) - d * d * V[cand].pow(2).sum(dim=1)
            k = int(gain.argmax())
            if float(gain[k]) <= 0:
                break
            r = r - d[k] * V[cand[k]]
            cand = torch.cat([cand[:k], cand[k + 1:]])
            taken += 1
        resid[q] = r
    return resid, float(taken)


def check_out(out, ref, precision):
    """out [HW][512]: the read-out of one object.  ``parts`` holds the worst ratio per criterion."""
    v = Violations()
    v.parts = {}
    out = out.double()

    def crit(name, err, bound):
        w = Violations()
        w.note(err, bound, name)
        v.extend(w)
        v.parts[name] = w.worst
        v.worst = max(v.worst, w.worst)

    if precision == 0:
        hard = (ref.rho.max(dim=0).values + (ref.B + 64) * U)[:, None] * ref.absmass + U * ref.out.abs()
        crit('hard', (out - ref.out).abs(), hard)
        tol = 5e-5 * max(1.0, float(ref.out.abs().max()))
        crit('project', (out - ref.out).abs(), torch.full_like(out, tol))
    else:
        tol = 1e-4 * max(1.0, float(ref.emulated.abs().max()))
        resid = out - ref.emulated
        if precision == 1:
            resid, v.parts['ties_taken'] = _settle_bf16_ties(resid, ref, tol)
        crit('project', resid.abs(), torch.full_like(out, tol))
        bar = (5e-2 if precision == 1 else 2e-4) * max(1.0, float(ref.exact.abs().max()))
        crit('exact', (out - ref.exact).abs(), torch.full_like(out, bar))
    return v
