"""Headline synthesis kernel (240 x d/o 96 -> 0.25 degree) with and without order pruning (shg_plan_set_order_pruning), interleaved in one
process: behind SETTLE_LAUNCHES untimed launches, blocks of 50 launches alternate between pruning off (every block at level N: the
unpruned kernel's launch) and on; the kernel is timed by the plan's own HIP events around it (profile kind lon_stage), the step
(repack + kernel) by events around the block.  Prints mean and block-to-block standard deviation of each arm and one JSON line.
    python3 tools/prune_ab.py [blocks per arm, default 12]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import grates_amd as ga
import bench
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 12
LAUNCHES = 50
grid = ga.grid.GeographicGrid(bench.GRID_STEP, bench.GRID_STEP)
colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(bench.KERNEL), bench.MAX_DEGREE, grid.parallels, bench.GM, bench.R_EARTH, grid.semimajor_axis, grid.flattening)
plan = ga.engine.Plan(bench.MAX_DEGREE, colat, kn, grid.meridians)
assert plan.info()['rotation_symmetry'] and any(level < bench.MAX_DEGREE for level in plan.info()['order_cutoffs'])
batch = torch.from_numpy(bench.coefficient_batch(1000, bench.EPOCHS, bench.MAX_DEGREE)).cuda()
out = torch.empty((bench.EPOCHS, grid.parallels.size, grid.meridians.size), dtype=torch.float64, device='cuda')
for _ in range(bench.SETTLE_LAUNCHES):
    plan.synthesis(batch, out=out)
torch.cuda.synchronize()
kernel_us, step_us = {0: [], 1: []}, {0: [], 1: []}
for blk in range(2 * blocks):
    arm = blk & 1
    plan.set_order_pruning(bool(arm))
    for _ in range(5):
        plan.synthesis(batch, out=out)
    torch.cuda.synchronize()
    plan.profile(True, kinds=['lon_stage'])
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(LAUNCHES):
        plan.synthesis(batch, out=out)
    b.record()
    torch.cuda.synchronize()
    ms, n = plan.profile_read()['lon_stage']
    plan.profile(False)
    assert n == LAUNCHES
    kernel_us[arm].append(1e3 * ms / n)
    step_us[arm].append(1e3 * a.elapsed_time(b) / LAUNCHES)
    print('block %2d pruning %s: kernel %.2f us  step %.2f us' % (blk, 'on ' if arm else 'off', kernel_us[arm][-1], step_us[arm][-1]), flush=True)
res = {'launches_per_block': LAUNCHES, 'blocks_per_arm': blocks, 'order_cutoffs': plan.info()['order_cutoffs'][:12]}
for arm, name in ((0, 'off'), (1, 'on')):
    res['kernel_us_' + name] = [statistics.mean(kernel_us[arm]), statistics.stdev(kernel_us[arm])]
    res['step_us_' + name] = [statistics.mean(step_us[arm]), statistics.stdev(step_us[arm])]
    print('pruning %-3s kernel %.2f +- %.2f us   step %.2f +- %.2f us (mean, block-to-block standard deviation, %d blocks)'
          % (name, *res['kernel_us_' + name], *res['step_us_' + name], blocks))
gain = res['kernel_us_off'][0] - res['kernel_us_on'][0]
res['kernel_gain_us'] = gain
res['kernel_ratio_on_over_off'] = res['kernel_us_on'][0] / res['kernel_us_off'][0]
res['clears_bar'] = gain > 2 * max(res['kernel_us_off'][1], res['kernel_us_on'][1])
print(json.dumps(res))
