"""Device time of one ``ops.track_update`` call (search + finish, all references of the call) by HIP events, on a 1080p frame at
S = 16: a 64 x 64 box, a 300 x 200 box, and both in one call.  usage: track_timing.py [calls]"""
import sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np, torch, vfloodnet_amd
from vfloodnet_amd import ops
from track_ref import texture

N = int(sys.argv[1]) if len(sys.argv) > 1 else 200
dev = torch.device('cuda', 0)
H, W, S = 1080, 1920, 16
rng = np.random.RandomState(0)
frame = torch.from_numpy(np.stack([texture(rng, H, W) for _ in range(3)]).astype(np.float32)).to(dev)
t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0.record()
for _ in range(N):
    luma = ops.track_luma(frame)
t1.record()
torch.cuda.synchronize()
print('track_luma 1080p: %.1f us per call' % (1e3 * t0.elapsed_time(t1) / N))
for boxes in ([(900, 500, 64, 64)], [(800, 400, 300, 200)], [(900, 500, 64, 64), (200, 300, 300, 200)]):
    st = ops.track_init(luma, np.array(boxes, np.int32), S)
    logs = (torch.zeros(1, len(boxes), 4, dtype=torch.int32, device=dev), torch.zeros(1, len(boxes), dtype=torch.int32, device=dev),
            torch.zeros(1, len(boxes), dtype=torch.float32, device=dev))
    for _ in range(10):
        ops.track_update(st, luma, *logs, 0)
    t0.record()
    for _ in range(N):
        ops.track_update(st, luma, *logs, 0)
    t1.record()
    torch.cuda.synchronize()
    assert logs[1].cpu().numpy().all()
    print('track_update 1080p S=%d boxes %s: %.1f us per call (%d calls back to back)'
          % (S, [b[2:] for b in boxes], 1e3 * t0.elapsed_time(t1) / N, N))
