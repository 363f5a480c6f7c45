"""The F(6x6) input / output transforms at the Winograd shapes of the 480x854 plan, each form of csrc/conv_winograd.hip in isolation
(vfn_winograd6_force_form): microseconds per form for the input transform, the output transform and the output transform with a
residual; the forms take turns inside every round, the figure is the fastest round and the spread is over the rounds.  A new form is
taken where it is at least 3 % faster than form 0 (VFN_TUNE_MARGIN, as scripts/tune_wino_gemm.py).
Writes <VFN_TUNE_OUT or tune_out>/tune_wino6_transforms.json.  usage: bench_wino6_transforms.py [rounds]"""
import sys, os, json
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch, vfloodnet_amd
from vfloodnet_amd import AFB_URR, _lib, ops
MARGIN = float(os.environ.get('VFN_TUNE_MARGIN', 0.97))
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 5
OUT = os.environ.get('VFN_TUNE_OUT', 'tune_out')
dev = torch.device('cuda', 0)
L = _lib.lib()


def time_call(fn, iters=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def plan_shapes():
    """(N, H, W, C) of every F(6x6) transform launch of the plan -> {'in' / 'out' / 'out_res': [layer names], 'rows': rows_pad}"""
    model = AFB_URR(dev, update_bank=True).to(dev).eval()
    plan = model.engine().plan(480, 854, 2)
    seen = {}
    for lst in plan.all_lists():
        for l in lst:
            if l.fn is ops.winograd_input and l.args[-1] == 6:
                key, kind, rows = tuple(l.args[4:8]), 'in', l.args[2]
            elif l.fn is ops.winograd_output and l.args[-1] == 6:
                key, kind, rows = tuple(l.args[3:7]), ('out_res' if l.args[9] is not None else 'out'), l.args[1]
            else:
                continue
            e = seen.setdefault(key, {'in': [], 'out': [], 'out_res': [], 'rows': rows})
            e['rows'] = min(e['rows'], rows)
            if l.name not in e[kind]:
                e[kind].append(l.name)
    return seen


def main():
    shapes = plan_shapes()
    report = []
    for (N, H, W, C), where in sorted(shapes.items()):
        rows = where['rows']
        x = torch.randn(N, H, W, C, device=dev)
        V = torch.zeros(64 * rows, C, device=dev)
        Mb = torch.randn(64 * rows, C, device=dev)
        out = torch.empty(N, H, W, C, device=dev)
        res = torch.randn(N, H, W, C, device=dev)
        sc, sh = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        calls = {'in': lambda: ops.winograd_input(x, V, rows, True, tile=6),
                 'out': lambda: ops.winograd_output(Mb, rows, out, N, H, W, C, sc, sh, None, 0, 0, True, tile=6),
                 'out_res': lambda: ops.winograd_output(Mb, rows, out, N, H, W, C, sc, sh, res, C, 0, False, tile=6)}
        forms = [0, 2]
        entry = {'shape': [N, H, W, C], 'rows_pad': rows, 'tiles': ops.winograd6_tiles(N, H, W), 'layers': {k: where[k] for k in calls}}
        for kind, fn in calls.items():
            t = {f: [] for f in forms}
            for _ in range(ROUNDS):
                for f in forms:
                    assert L.vfn_winograd6_force_form(f) == 0
                    t[f].append(time_call(fn))
            L.vfn_winograd6_force_form(-1)
            best = {f: min(v) for f, v in t.items()}
            new = min((best[f], f) for f in forms if f)
            take = new[1] if new[0] < MARGIN * best[0] else 0
            rule = L.vfn_winograd6_form(N, H, W, C, int(kind != 'in'), int(kind == 'out_res'))
            entry[kind] = {'us': {str(f): round(best[f], 2) for f in sorted(forms)},
                           'spread_us': {str(f): round(max(t[f]) - min(t[f]), 2) for f in sorted(forms)}, 'measured_best': take, 'rule': rule}
            print(f'[{N}x{H}x{W}x{C}] rows {rows} {kind:8s} ' + ' | '.join(f'form {f}: {best[f]:6.2f} us (+{max(t[f]) - min(t[f]):.2f})' for f in sorted(forms)) +
                  f' -> {take} (rule {rule})', flush=True)
        report.append(entry)
    os.makedirs(OUT, exist_ok=True)
    json.dump(report, open(OUT + '/tune_wino6_transforms.json', 'w'), indent=1)


main()
