"""Time of the draw product plmc_trmm_ut (Y = shift + U^T Z against a factor buffer) at n = 8192, q in {1, 8}, ns in {1, 16, 256}, fp32,
with plmc_wt_matvec -- the same walk on the other triangle of the same buffer, the same bytes -- beside the thin path as the yardstick.
HIP events around every launch, median of 50 launches after 5 warm-up launches, each kind alternating with its neighbour in one
process.  The buffer is a training workspace (U and W columns) filled with random numbers: neither kernel looks at the values.
`python tools/sample_time.py [--md profiles/sample_time.md] [--n 8192] [--reps 50]`"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8192)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--md", default=None)
a = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "projected-lmc_amd")]

import torch  # noqa: E402
from projectedlmc import _engine, _hip  # noqa: E402

assert torch.cuda.is_available(), "tools/sample_time.py measures on the GPU only"
dev = torch.device("cuda:0")
dt = torch.float32
L = _hip.lib()
n = a.n
WARM = 5


rows = []
for q in (1, 8):
    ws = _engine.Workspace(n, q, 0, dt, dev, with_inverse=True)
    ws.A.normal_()
    st = _hip.stream_ptr(dev)
    tri_bytes = q * (n * (n + 1) / 2) * 4

    def matvec():
        L.call("plmc_wt_matvec", dt, _hip.ptr(ws.W), ws.n_pad, ws.ldw, ws.strideW, _hip.ptr(ws.z), _hip.ptr(ws.alpha), q, st)

    ws.z.normal_()
    for ns in (1, 16, 256):
        Z = torch.randn(q, n, ns, dtype=dt, device=dev)
        shift = torch.randn(q, n, dtype=dt, device=dev)
        Y = torch.empty(q, n, ns, dtype=dt, device=dev)

        def trmm():
            L.call("plmc_trmm_ut", dt, _hip.ptr(ws.A), ws.n_pad, ws.lda, ws.strideA, n, _hip.ptr(Z), ns, ns, n * ns, _hip.ptr(shift),
                   _hip.ptr(Y), ns, n * ns, q, st)

        # alternate the two kinds launch by launch: whatever else shares the machine hits both alike
        for _ in range(WARM):
            trmm()
            matvec()
        torch.cuda.synchronize()
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(4)] for _ in range(a.reps)]
        for e in ev:
            e[0].record()
            trmm()
            e[1].record()
            e[2].record()
            matvec()
            e[3].record()
        torch.cuda.synchronize()
        tt, tm = [e[0].elapsed_time(e[1]) for e in ev], [e[2].elapsed_time(e[3]) for e in ev]
        med_t, med_m = statistics.median(tt), statistics.median(tm)
        qt = statistics.quantiles(tt, n=4)
        flops = 1.0 * q * n * n * ns                       # n^2 / 2 multiply-adds
        byts = tri_bytes + 2.0 * q * n * ns * 4
        rows.append((q, ns, "thin" if ns <= 16 else "wide", med_t, qt[0], qt[2], byts / med_t * 1e-6, flops / med_t * 1e-9, med_m,
                     tri_bytes / med_m * 1e-6, med_t / med_m))
    del ws
    _engine.free_workspaces()
    torch.cuda.empty_cache()

lines = ["| q | ns | path | trmm_ut median ms | quartiles ms | GB/s | TFLOP/s | wt_matvec median ms | wt_matvec GB/s | trmm / matvec |",
         "|---|---|---|---|---|---|---|---|---|---|"]
for q, ns, path, mt, q1, q3, gbs, tfs, mm, mgbs, ratio in rows:
    lines.append("| %d | %d | %s | %.4f | %.4f - %.4f | %.0f | %.2f | %.4f | %.0f | %.2f |" % (q, ns, path, mt, q1, q3, gbs, tfs, mm, mgbs, ratio))
text = "\n".join(lines)
print("n = %d, fp32, %d launches per cell (median), device %s" % (n, a.reps, torch.cuda.get_device_name(0)))
print(text)
if a.md:
    os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
    with open(a.md, "w") as fh:
        fh.write("n = %d, fp32, %d launches per cell (median), device %s\n\n%s\n" % (n, a.reps, torch.cuda.get_device_name(0), text))
