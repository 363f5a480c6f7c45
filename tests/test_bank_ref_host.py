"""tests/bank_ref.py on the CPU: its references against the oracle, the sharpness of the hit-count check on the inputs the GPU
tests use, and every checker against results damaged on purpose (dropped / dead rows, a count off by one, a missing slice, the
wrong duplicate, a misplaced score tile) -- what mutation runs of the kernels would show, without running a wrong kernel."""

import pytest
import torch

import bank_ref
from bank_ref import CASES, CH, DK, DV, U


def _results(ref):
    """What a correct kernel would hand back for a memread reference, in f32."""
    l = torch.exp(ref.s - ref.m_ref).sum(dim=0)
    return ref.m_ref.float(), l.float(), ref.out.float(), ref.sure.int()


def test_references_agree_with_the_oracle(monkeypatch):
    """bank_ref.memread (precision 0) against oracle.afb_urr_ref.matcher (read-out, query values, info bump) and bank_ref.match
    against the corr.argmax / gather lines of FeatureBankRef.update, on a two-object bank of 72 and 200 entries, HW 33.  The
    oracle runs in f32: 1e-5 of the largest value; the arg-max wherever the f64 top two are further apart than 2E."""
    from oracle import afb_urr_ref as orc
    lens, hw = [72, 200], 33
    g = torch.Generator().manual_seed(sum(lens) + hw)
    q = 2.0 * torch.randn(hw, DK, generator=g)
    keys = [torch.randn(n, DK, generator=g) for n in lens]
    vals = [torch.randn(n, DV, generator=g) for n in lens]
    qv = torch.randn(hw, DV, generator=g)

    fb = orc.FeatureBankRef(2, 250000)
    fb.init_bank([k.t().contiguous() for k in keys], [v.t().contiguous() for v in vals])
    for i in range(2):
        fb.info[i][:, 1] = 0.5
    got = orc.matcher(fb, q.t().unsqueeze(0), qv.t().unsqueeze(0))[0]                 # [obj][1024][HW]
    settled = 0
    for i in range(2):
        ref = bank_ref.memread(keys[i], vals[i], q, 0)
        mem = got[i, :DV].t().double()
        assert (mem - ref.out).abs().max() <= 1e-5 * ref.out.abs().max()
        assert torch.equal(got[i, DV:].t(), qv)
        # the bump, wherever the threshold test cannot go either way (the oracle's f32 softmax is well inside rho)
        ok = ref.maybe == 0
        settled += int(ok.sum())
        bump = 0.5 + torch.log(ref.sure.double() + 1)
        assert ((fb.info[i][:, 1].double() - bump).abs()[ok]).max() <= 1e-5 * bump.max()
        assert torch.equal(fb.info[i][:, 0], torch.zeros(lens[i]))
    assert settled >= 0.9 * sum(lens)

    # the match: the corr.argmax / gather lines of FeatureBankRef.update, observed as the oracle runs them
    new = torch.randn(2, hw, DK + DV, generator=g)
    for i in range(2):
        src = torch.randint(0, lens[i], (hw // 3,), generator=g)
        new[i, :hw // 3, :DK] = keys[i][src] * 0.7 + 0.05 * torch.randn(hw // 3, DK, generator=g)
    seen = []
    real_gather = torch.gather

    def spy(inp, dim, index, **kw):
        out = real_gather(inp, dim, index, **kw)
        if inp.dim() == 2 and inp.shape[1] == hw and dim == 0 and index.shape == (1, hw):
            seen.append((inp.clone(), index.clone(), out.clone()))
        return out
    monkeypatch.setattr(torch, 'gather', spy)
    fb.update([new[i, :, :DK].t().contiguous() for i in range(2)], [new[i, :, DK:].t().contiguous() for i in range(2)], 1)
    monkeypatch.undo()
    assert len(seen) == 2
    for i in range(2):
        corr_o, idx_o, best_o = seen[i]
        assert corr_o.shape == (lens[i], hw)
        rowscale = 1.0 / bank_ref.row_norms(keys[i]).clamp_min(1e-12)
        colscale = 1.0 / bank_ref.row_norms(new[i, :, :DK]).clamp_min(1e-12)
        ref = bank_ref.match(keys[i], rowscale.float(), new[i, :, :DK].contiguous(), colscale.float(), 0)
        C = ref.S * ref.colscale                                                        # the cosines in f64
        assert (corr_o.double() - C).abs().max() <= 1e-5 * C.abs().max()
        top = ref.S.topk(2, dim=0)
        clear = (top.values[0] - top.values[1]) > 2 * ref.E.max(dim=0).values
        assert clear.sum() >= hw // 2
        assert torch.equal(idx_o[0][clear], top.indices[0][clear])
        cols = torch.arange(hw)
        assert (best_o[0].double() - C[idx_o[0], cols]).abs().max() <= 1e-5 * C.abs().max()
        # ... and the checker accepts the oracle's own answer
        assert bank_ref.check_match(top.indices[0], C[top.indices[0], cols].float(), ref) == []


@pytest.mark.parametrize('precision', [0, 1, 2])
@pytest.mark.parametrize('case', sorted(CASES))
def test_inputs_keep_the_hit_check_sharp(case, precision):
    """A condition on the inputs, evaluated on the reference alone: at most 10 % of an object's live entries have a probability
    so close to the threshold that check_hits must accept two counts (largest share: 6.2 %, case B, length 65, bf16x3)."""
    c = bank_ref.make_case(case)
    for i, n in enumerate(c['lens']):
        ref = bank_ref.memread(c['keys'][i], c['vals'][i], c['q'], precision)
        share = float((ref.maybe > 0).double().mean())
        print(f'case {case} object {i} (length {n}) precision {precision}: maybe > 0 on {100 * share:.1f} % of the entries')
        assert share <= 0.10


def test_checkers_reject_known_wrong_results():
    """Every checker passes the reference's own results and reports a violation for each way a wrong kernel would damage them
    (case A, both objects, every precision)."""
    c = bank_ref.make_case('A')
    lens, hw, nsplit_scan, _ = CASES['A']
    g = torch.Generator().manual_seed(5)
    for i, B in enumerate(c['lens']):
        keys, vals, q = c['keys'][i], c['vals'][i], c['q']
        for precision in (0, 1, 2):
            ref = bank_ref.memread(keys, vals, q, precision)
            m, l, out, cnt = _results(ref)
            good = ref.emulated.float() if precision else out
            assert bank_ref.check_stats(m, l, ref) == []
            assert bank_ref.check_out(good, ref, precision) == []
            assert bank_ref.check_hits(cnt, ref) == []

            # read-out with the last live row dropped
            dropped = good.double() - ref.p[B - 1][:, None] * vals[B - 1].double()[None, :]
            assert bank_ref.check_out(dropped.float(), ref, precision)
            # read-out with the first dead row (stale key and value, N(0,1)) included with the probability its key would get
            dead_k, dead_v = torch.randn(DK, generator=g), torch.randn(DV, generator=g)
            s_dead = bank_ref.scores(dead_k[None], q, precision)[0][0] * ref.scale
            p_dead = torch.exp(s_dead - ref.lse_ref)
            leaked = good.double() + p_dead[:, None] * dead_v.double()[None, :]
            assert bank_ref.check_out(leaked.float(), ref, precision)

            if precision == 1:
                # plain bf16: a probability the reference puts within rho of a bf16 midpoint may take its other rounding ...
                amb, step = bank_ref.bf16_ties(ref)
                weight = (step.abs() * amb)[:, :, None] * bank_ref._rb(vals).double().abs().max(dim=1).values[:, None, None]
                bb, qq = divmod(int(weight.reshape(-1).argmax()), hw)
                assert bool(amb[bb, qq]) and 0 < float(amb.double().mean()) < 0.25
                other = good.double()
                other[qq] += step[bb, qq] * bank_ref._rb(vals[bb]).double()
                assert bank_ref.check_out(other.float(), ref, precision) == []
                # ... one that is decided may not: the heaviest such step is far above the tolerance
                weight = (step.abs() * ~amb)[:, :, None] * bank_ref._rb(vals).double().abs().max(dim=1).values[:, None, None]
                bb, qq = divmod(int(weight.reshape(-1).argmax()), hw)
                other = good.double()
                other[qq] += step[bb, qq] * bank_ref._rb(vals[bb]).double()
                assert float(weight.max()) > 1e-3 and bank_ref.check_out(other.float(), ref, precision)

            # a hit count off by one where the threshold test cannot go either way; a count on a dead row
            b = int((ref.maybe == 0).nonzero()[B // 2])
            for d in (1, -1):
                wrong = cnt.clone()
                wrong[b] += d
                assert bank_ref.check_hits(wrong, ref)
            assert bank_ref.check_hits(torch.cat([cnt, torch.tensor([0, 1], dtype=torch.int32)]), ref)
            assert bank_ref.check_hits(torch.cat([cnt, torch.zeros(3, dtype=torch.int32)]), ref) == []

            # l without one of the scan's bank slices (chunk_range of memory_read.hip: ceil(chunks / nsplit) chunks each)
            nchunks = (B + CH - 1) // CH
            per = (nchunks + nsplit_scan - 1) // nsplit_scan
            for split in range(nsplit_scan):
                lo, hi = split * per * CH, min(B, (split + 1) * per * CH)
                if lo >= hi or (lo == 0 and hi == B):
                    continue
                part = torch.exp(ref.s[lo:hi] - ref.m_ref).sum(dim=0)
                assert bank_ref.check_stats(m, (l.double() - part).float(), ref), (B, split)
            assert bank_ref.check_stats((ref.m_ref + 4 * ref.dsmax).float(), l, ref)

    # the stored scores: one tile written at the neighbouring query tile's position
    ref = bank_ref.memread(c['keys'][0], c['vals'][0], c['q'], 0)
    buf = bank_ref.scores_to_tiles(ref.S.float())
    assert torch.equal(bank_ref.scores_from_tiles(buf, ref.B, ref.HW), ref.S.float())
    assert bank_ref.check_scores_tiles(buf, ref) == []
    nqt = (hw + 127) // 128
    assert nqt == 2
    tiles = buf.view(-1, nqt, 8192).clone()
    tiles[3, 0], tiles[3, 1] = buf.view(-1, nqt, 8192)[3, 1], buf.view(-1, nqt, 8192)[3, 0]
    assert bank_ref.check_scores_tiles(tiles.reshape(-1), ref)
    shifted = buf.view(-1, 2, 4, 2, 128, 4).clone()                 # ... and one with the two lane halves exchanged
    shifted[7] = shifted[7].flip(2)
    assert bank_ref.check_scores_tiles(shifted.reshape(-1), ref)

    # the arg-max on the higher of two bit-identical rows
    keys = c['keys'][0].clone()
    keys[700] = keys[3]
    new = c['new'][0, :, :DK].clone()
    new[5] = 0.7 * keys[3]
    rowscale = (1.0 / bank_ref.row_norms(keys).clamp_min(1e-12)).float()
    colscale = (1.0 / bank_ref.row_norms(new).clamp_min(1e-12)).float()
    for precision in (0, 1, 2):
        mref = bank_ref.match(keys, rowscale, new, colscale, precision)
        idx = mref.S.argmax(dim=0)
        assert int(idx[5]) in (3, 700)
        idx[5] = 3
        corr = (mref.S[idx, torch.arange(hw)] * mref.colscale).float()
        assert abs(float(corr[5]) - 1.0) < 1e-2
        assert bank_ref.check_match(idx, corr, mref) == []
        idx[5] = 700
        assert bank_ref.check_match(idx, corr, mref)
        idx[5] = 3
        idx[6] = (idx[6] + 1) % mref.B                               # any other row: below the maximum by far more than 2E
        assert bank_ref.check_match(idx, corr, mref)
        idx[6] = -1
        assert bank_ref.check_match(idx, corr, mref)
