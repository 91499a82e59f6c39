"""Headline synthesis kernel (240 x d/o 96 -> 0.25 degree) with and without the fold of the half column tile (shg_plan_set_half_tile_fold),
interleaved in one process: behind SETTLE_LAUNCHES untimed launches, blocks of 50 launches alternate between fold off (every column tile
forms and stores all 2 R images: the kernel's launch before the fold) and on; the kernel is timed by the plan's own HIP events around it
(profile kind lon_stage), the step (repack + kernel) by events around the block.  Prints mean and block-to-block standard deviation of
each arm and one JSON line.  The bar: the kernel's gain exceeds twice the larger standard deviation of the two arms.
    python3 tools/half_tile_ab.py [blocks per arm, default 12] [grid step in degrees, default bench.GRID_STEP]"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import grates_amd as ga
import bench
blocks = int(sys.argv[1]) if len(sys.argv) > 1 else 12
step = float(sys.argv[2]) if len(sys.argv) > 2 else bench.GRID_STEP
LAUNCHES = 50
grid = ga.grid.GeographicGrid(step, step)
colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(bench.KERNEL), bench.MAX_DEGREE, grid.parallels, bench.GM, bench.R_EARTH, grid.semimajor_axis, grid.flattening)
plan = ga.engine.Plan(bench.MAX_DEGREE, colat, kn, grid.meridians)
info = plan.info()
assert info['rotation_symmetry'] and info['half_tile_fold'], info
batch = torch.from_numpy(bench.coefficient_batch(1000, bench.EPOCHS, bench.MAX_DEGREE)).cuda()
out = torch.empty((bench.EPOCHS, grid.parallels.size, grid.meridians.size), dtype=torch.float64, device='cuda')
for _ in range(bench.SETTLE_LAUNCHES):
    plan.synthesis(batch, out=out)
torch.cuda.synchronize()
kernel_us, step_us = {0: [], 1: []}, {0: [], 1: []}
for blk in range(2 * blocks):
    arm = blk & 1
    plan.set_half_tile_fold(bool(arm))
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
    print('block %2d fold %s: kernel %.2f us  step %.2f us' % (blk, 'on ' if arm else 'off', kernel_us[arm][-1], step_us[arm][-1]), flush=True)
res = {'launches_per_block': LAUNCHES, 'blocks_per_arm': blocks, 'grid_step': step, 'nlon': int(grid.meridians.size), 'rotations': info['rotations']}
for arm, name in ((0, 'off'), (1, 'on')):
    res['kernel_us_' + name] = [statistics.mean(kernel_us[arm]), statistics.stdev(kernel_us[arm])]
    res['step_us_' + name] = [statistics.mean(step_us[arm]), statistics.stdev(step_us[arm])]
    print('fold %-3s kernel %.2f +- %.2f us   step %.2f +- %.2f us (mean, block-to-block standard deviation, %d blocks)'
          % (name, *res['kernel_us_' + name], *res['step_us_' + name], blocks))
gain = res['kernel_us_off'][0] - res['kernel_us_on'][0]
res['kernel_gain_us'] = gain
res['kernel_ratio_on_over_off'] = res['kernel_us_on'][0] / res['kernel_us_off'][0]
res['clears_bar'] = gain > 2 * max(res['kernel_us_off'][1], res['kernel_us_on'][1])
print(json.dumps(res))
