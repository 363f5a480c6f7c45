"""Re-measure the kernel choice of every Winograd-domain GEMM (default) or of every 1x1 / stride-1 convolution (argument `pconv`) of the
C2 / C3 / C5 plans (and of the training plan) now that the persistent kernel (vfn_winograd_gemm_f32, configuration ids >= 1000;
vfn_conv1x1_persistent_f32, ids >= 2000) competes with one-workgroup-per-tile launches: the table entry of a shape changes hands only
when the new choice is at least MARGIN faster than the old one, re-timed alternately.
Writes gpurun_out/tuned_gfx950.json + gpurun_out/r05_tune_{wino_gemm,pconv}_report.json."""
# Argument `rows32`: every F(6x6) GEMM of the inference plans whose rows shrink when padded to 32 instead of 64, through the 32-row tiles
# against its shipped 64-row choice -> tuned_gfx950_wino6.json gains (64 * rows32, Cout, Cin) where 32 rows are MARGIN faster.
# Argument `shortcut`: every fused shortcut launch (ops.shortcut_fused_launch) of the inference plans through the persistent kernel's
# configurations -> tuned_gfx950_shortcut.json (a shape whose best fused time does not beat its two launches in
# scripts/profile_layers.py's table gets tile cfg -1 there by hand: it keeps two launches).  Both write the table and
# tune_{rows32,shortcut}_report.json into the directory VFN_TUNE_OUT names (default tune_out/, as scripts/tune_winograd.py).
# Argument `thin3x3`: every 3x3 layer of the inference plans that the LDS-resident kernel takes (ops.thin3x3_eligible: 32 filters, 32 or
# 64 input channels) through that kernel's grids against the shape's choice in tuned_gfx950.json, each launch repeated in isolation ->
# tuned_gfx950_thin.json holds the shapes where it is MARGIN faster; tune_thin3x3_report.json lists every shape, won or not.
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, vfloodnet_amd
from vfloodnet_amd import AFB_URR, engine, ops
MARGIN = float(os.environ.get('VFN_TUNE_MARGIN', 0.97))
WHICH = sys.argv[1] if len(sys.argv) > 1 else 'wino'
dev = torch.device('cuda', 0)
model = AFB_URR(dev, update_bank=True).to(dev).eval()
eng = model.engine()
table = engine._TABLES[0]
report = []


def timeit(d, c, iters=12):
    for _ in range(2):
        ops.conv2d_launch(d, c, 0)
    torch.cuda.synchronize()
    best = None
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            ops.conv2d_launch(d, c, 0)
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        best = ms if best is None else min(best, ms)
    return best * 1e3


def time_call(fn, iters=12):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    best = None
    for _ in range(4):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record(); torch.cuda.synchronize()
        ms = e0.elapsed_time(e1) / iters
        best = ms if best is None else min(best, ms)
    return best * 1e3


def tune_rows32(plans):
    """The F(6x6) GEMMs on operands of their own (the timing does not depend on the values): shipped 64-row choice against every
    32-row configuration on the 32-padded rows."""
    seen = {}
    for p in plans:
        for lst in p.all_lists():
            for i, l in enumerate(lst):
                if l.fn is ops.conv2d_launch and engine.is_wino6_desc(l.args[0]) and i > 0 and lst[i - 1].fn is ops.winograd_input:
                    d, (N, H, W) = l.args[0], lst[i - 1].args[4:7]
                    rows32 = (ops.winograd6_tiles(N, H, W) + 31) // 32 * 32
                    if rows32 < d.w_batch_rows and d.w_batch_rows % 64 == 0:
                        seen.setdefault((d.w_batch_rows, rows32, d.Cout, d.Cin, d.cout_pad), (l.name, l.args[1]))
    for (rows, rows32, cout, cin, cout_pad), (name, old) in sorted(seen.items()):
        V, U = torch.randn(64 * rows, cin, device=dev), torch.randn(64 * cout_pad, cin, device=dev)
        Mb = torch.empty(64 * rows, cout, device=dev)
        d64 = ops.make_winograd_gemm_desc(V, U, Mb, rows, cin, cout, 64)
        d32 = ops.make_winograd_gemm_desc(V[:64 * rows32], U, Mb[:64 * rows32], rows32, cin, cout, 64)
        cand = sorted((time_call(lambda: ops.conv2d_launch(d32, c, 0), 6), c) for c in ops.wino_gemm_cfg_options(rows32, cout)
                      if ops.is_wino_gemm32_cfg(c))
        t_old = time_call(lambda: ops.conv2d_launch(d64, old, 0))
        best = min((time_call(lambda: ops.conv2d_launch(d32, c, 0)), c) for _, c in cand[:3])
        t_old = min(t_old, time_call(lambda: ops.conv2d_launch(d64, old, 0)))
        take = best[0] < MARGIN * t_old
        report.append({'layer': name, 'rows': rows, 'rows32': rows32, 'cout': cout, 'cin': cin, 'old': old, 'old_us': round(t_old, 1),
                       'new': best[1], 'new_cfg': list(ops.persistent_cfg_info(best[1])), 'new_us': round(best[0], 1), 'taken': bool(take)})
        print(report[-1], flush=True)
        if take:
            engine._TUNED_WINO6[(64 * rows32, cout, cin)] = (best[1], 1, 0)
    engine.save_tuned(OUT + '/tuned_gfx950_wino6.json', 'wino6')


def tune_shortcut(plans):
    seen = {}
    for p in plans:
        for lst in p.all_lists():
            for l in lst:
                if l.fn is ops.shortcut_fused_launch:
                    sc, d = l.args[:2]
                    seen.setdefault((d.M, d.Cout, sc.Cin, d.Cin), l)
    for key, l in sorted(seen.items()):
        sc, d = l.args[:2]
        cand = sorted((time_call(lambda: ops.shortcut_fused_launch(sc, d, *o), 6), o) for o in ops.shortcut_fused_cfg_options(sc, d))
        best = min((time_call(lambda: ops.shortcut_fused_launch(sc, d, *o)), o) for _, o in cand[:3])
        t_cur = time_call(lambda: ops.shortcut_fused_launch(sc, d, *l.args[2:4]))
        report.append({'layer': l.name, 'shape': list(key), 'current': list(l.args[2:4]), 'current_us': round(t_cur, 1), 'best': list(best[1]),
                       'best_us': round(best[0], 1), 'all_us': {'%d/%d' % o: round(t, 1) for t, o in cand}})
        print(report[-1], flush=True)
        engine._TUNED_SHORTCUT[key] = tuple(best[1])
    engine.save_tuned(OUT + '/tuned_gfx950_shortcut.json', 'shortcut')


def tune_thin3x3(plans):
    seen = {}
    for p in plans:
        for lst in p.all_lists():
            for l in lst:
                if l.fn is ops.conv2d_launch and int(l.args[2]) == 0 and ops.thin3x3_eligible(l.args[0], 0, ignore_split=True):
                    d = l.args[0]
                    seen.setdefault((d.M, d.Cout, d.KH * d.KW * d.Cin), (l, p))
    engine._TUNED_THIN.clear()
    for key, (l, p) in sorted(seen.items()):
        d, cur = l.args[0], (l.args[1],)
        old = tuple(table.get(key) or engine.choose_cfg(*key, 0))
        t_new = {}
        for rnd in range(2):                              # alternately with the old choice, the faster of the two rounds each
            for c in ops.thin3x3_cfg_options(d):
                ops.set_splitk(d, 1, None)
                t_new[c] = min(t_new.get(c, 1e30), timeit(d, c))
            cfg_old = engine.apply_choice(d, old, p.ws, p.cnt)
            t_old = min(t_old, timeit(d, cfg_old)) if rnd else timeit(d, cfg_old)
        if ops.is_thin3x3_cfg(cur[0]):                    # leave the plan's descriptor as it was found
            ops.set_splitk(d, 1, None)
        best = min((t, c) for c, t in t_new.items())
        take = best[0] < MARGIN * t_old
        fl = 2.0 * key[0] * key[1] * key[2]
        report.append({'layer': l.name, 'shape': list(key), 'old': list(old[:3]), 'old_us': round(t_old, 1), 'old_tf': round(fl / t_old / 1e6, 1),
                       'thin_us': {ops.thin3x3_cfg_info(c)[1]: round(t, 1) for c, t in sorted(t_new.items())}, 'new': best[1],
                       'new_us': round(best[0], 1), 'new_tf': round(fl / best[0] / 1e6, 1), 'taken': bool(take)})
        print(report[-1], flush=True)
        if take:
            engine._TUNED_THIN[key] = best[1]
    engine.save_tuned(OUT + '/tuned_gfx950_thin.json', 'thin')


seen = {}
plans = [eng.plan(h, w, 2) for (h, w) in [(480, 854), (480, 853)]]
if WHICH in ('rows32', 'shortcut', 'thin3x3'):
    OUT = os.environ.get('VFN_TUNE_OUT', 'tune_out')
    os.makedirs(OUT, exist_ok=True)
    {'rows32': tune_rows32, 'shortcut': tune_shortcut, 'thin3x3': tune_thin3x3}[WHICH](plans)
    json.dump(report, open(OUT + '/tune_%s_report.json' % WHICH, 'w'), indent=1)
    sys.exit(0)
if os.environ.get('VFN_TUNE_TRAIN', '1') == '1':
    try:
        tp = eng.plan(400, 400, 2, keep_acts=True)
        tp.batch_set(5)
        plans.append(tp)
    except Exception as e:                                # (the inference shapes are what matters here)
        print('training plan skipped:', repr(e))
for p in plans:
    for lst in p.all_lists():
        for l in lst:
            if l.fn is not ops.conv2d_launch or int(l.args[2]) != 0:
                continue
            d = l.args[0]
            if (WHICH == 'wino' and 'wino_gemm' in (l.name or '')) or (WHICH == 'pconv' and ops.pconv_eligible(d, 0)):
                seen.setdefault((d.M, d.Cout, d.KH * d.KW * d.Cin), (d, p))
for key, (d, p) in sorted(seen.items()):
    old = table.get(key) or engine.choose_cfg(*key, 0)
    cand = []
    for c in (ops.wino_gemm_cfg_options(d.w_batch_rows, d.Cout, rows32=False) if WHICH == 'wino' else ops.pconv_cfg_options(d.Cout)):
        engine.apply_choice(d, (c, 1, 0), p.ws, p.cnt)
        try:
            cand.append((timeit(d, c, 6), c))
        except RuntimeError:
            pass
    cand.sort()
    engine.apply_choice(d, tuple(old), p.ws, p.cnt)
    t_old = timeit(d, old[0])
    best = None
    for t_, c in cand[:3]:                               # the three fastest once more, alternately with the old choice
        engine.apply_choice(d, (c, 1, 0), p.ws, p.cnt)
        t_new = timeit(d, c)
        if best is None or t_new < best[0]:
            best = (t_new, c)
    engine.apply_choice(d, tuple(old), p.ws, p.cnt)
    t_old = min(t_old, timeit(d, old[0]))
    take = best is not None and best[0] < MARGIN * t_old
    fl = 2.0 * key[0] * key[1] * key[2]
    report.append({'shape': list(key), 'old': list(old), 'old_us': round(t_old, 1), 'new': [best[1], 1, 0] if best else None,
                   'new_us': round(best[0], 1) if best else None, 'taken': bool(take), 'old_tf': round(fl / t_old / 1e6, 1),
                   'new_tf': round(fl / best[0] / 1e6, 1) if best else None})
    print(report[-1], flush=True)
    if take:
        table[key] = (best[1], 1, 0) + (tuple(old[:3]) if WHICH == 'pconv' else ())      # (pconv: the old choice stays as the fallback)
os.makedirs('gpurun_out', exist_ok=True)
engine.save_tuned('gpurun_out/tuned_gfx950.json', 0)
json.dump(report, open('gpurun_out/r05_tune_%s_report.json' % ('wino_gemm' if WHICH == 'wino' else 'pconv'), 'w'), indent=1)
print('shapes', len(report), 'moved', sum(r['taken'] for r in report), 'old total %.1f us, new total %.1f us' % (
    sum(r['old_us'] for r in report), sum(r['new_us'] if r['taken'] else r['old_us'] for r in report)))
