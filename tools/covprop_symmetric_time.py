"""shg_covprop_diag_symmetric at d/o 60 on a 2 degree grid (M = 16200 rows, P = 3721), event-timed in windows of 40 calls; for A / B
runs of two builds on one box, one process per build, alternated by the caller.
    python3 tools/covprop_symmetric_time.py [library.so | -] [windows]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import grates_amd as ga
if len(sys.argv) > 1 and sys.argv[1] != '-':
    ga._lib.use_library(sys.argv[1])
windows = int(sys.argv[2]) if len(sys.argv) > 2 else 7
N, CALLS = 60, 40
grid = ga.grid.GeographicGrid(2.0, 2.0)
colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel('potential'), N, grid.parallels, 3.9860044150e+14, 6.3781363000e+06,
                                               grid.semimajor_axis, grid.flattening)
plan = ga.engine.Plan(N, colat, kn, grid.meridians)
P = (N + 1) ** 2
gen = torch.Generator(device='cuda').manual_seed(7)
G = torch.randn((P, 512), dtype=torch.float64, device='cuda', generator=gen)
cov = ga.engine.gemm(G, G, transb=True, alpha=1.0 / 512)
cov.diagonal().add_(1.0)
cov = 0.5 * (cov + cov.T)
out = torch.empty(grid.parallels.size * grid.meridians.size, dtype=torch.float64, device='cuda')
for _ in range(5):
    plan.covariance_propagation(cov, 0, symmetric=True, out=out)
times = []
for w in range(windows):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(CALLS):
        plan.covariance_propagation(cov, 0, symmetric=True, out=out)
    b.record()
    torch.cuda.synchronize()
    times.append(a.elapsed_time(b) / CALLS)
times.sort()
print('%s: ms per call, windows of %d: min %.4f median %.4f max %.4f  checksum %.15e' %
      (sys.argv[1] if len(sys.argv) > 1 else '-', CALLS, times[0], times[len(times) // 2], times[-1], float(out.sum().item())), flush=True)
