"""Headline synthesis kernel (240 x d/o 96 -> 0.25 degree) against the limit on workgroups in their Legendre stage (shg_plan_set_stage_limit),
by the method of tools/prune_ab.py: one process, SETTLE_LAUNCHES untimed launches, then blocks of 50 launches that go round the arms (one
limit each, the first arm is the reference); the kernel is timed by the plan's own HIP events around it (profile kind lon_stage), the step
(repack + kernel) by events around the block.  Prints mean and block-to-block standard deviation of each arm, the gain of every arm over the
first in units of the larger of the two standard deviations, and one JSON line.
    python3 tools/stage_limit_sweep.py [--arms 0,-4,-5,-6,-7,-8,-10,-12] [--blocks 12] [--library grates_amd/lib/variants/libshg_NAME.so]
Two arms are an A/B (`--arms 0,-7`); `default` as an arm leaves the plan as it was created."""
import argparse, json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument('--arms', default='0,-4,-5,-6,-7,-8,-10,-12')
ap.add_argument('--blocks', type=int, default=12, help='blocks of 50 launches per arm')
ap.add_argument('--library', default=None, help='a variant build (make variant) in place of libshg.so')
args = ap.parse_args()
import torch
import grates_amd as ga
if args.library:
    ga._lib.use_library(args.library)
import bench
arms = [a.strip() for a in args.arms.split(',')]
LAUNCHES = 50
grid = ga.grid.GeographicGrid(bench.GRID_STEP, bench.GRID_STEP)
colat, _, kn = ga.gravityfield.surface_factors(ga.kernel.get_kernel(bench.KERNEL), bench.MAX_DEGREE, grid.parallels, bench.GM, bench.R_EARTH, grid.semimajor_axis, grid.flattening)
plans = {}
for arm in arms:                                     # one plan per arm: `default` must never have seen set_stage_limit
    plans[arm] = ga.engine.Plan(bench.MAX_DEGREE, colat, kn, grid.meridians)
    if arm != 'default':
        plans[arm].set_stage_limit(int(arm))
batch = torch.from_numpy(bench.coefficient_batch(1000, bench.EPOCHS, bench.MAX_DEGREE)).cuda()
out = torch.empty((bench.EPOCHS, grid.parallels.size, grid.meridians.size), dtype=torch.float64, device='cuda')
for k in range(bench.SETTLE_LAUNCHES):
    plans[arms[k % len(arms)]].synthesis(batch, out=out)
torch.cuda.synchronize()
kernel_us, step_us = {a: [] for a in arms}, {a: [] for a in arms}
for blk in range(args.blocks * len(arms)):
    arm = arms[blk % len(arms)]
    plan = plans[arm]
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
    print('block %3d limit %-7s: kernel %.2f us  step %.2f us' % (blk, arm, kernel_us[arm][-1], step_us[arm][-1]), flush=True)
res = {'library': ga._lib.LIB_PATH if args.library else 'libshg.so', 'launches_per_block': LAUNCHES, 'blocks_per_arm': args.blocks, 'arms': {}}
for arm in arms:
    res['arms'][arm] = {'kernel_us': [statistics.mean(kernel_us[arm]), statistics.stdev(kernel_us[arm])],
                        'step_us': [statistics.mean(step_us[arm]), statistics.stdev(step_us[arm])]}
ref = res['arms'][arms[0]]
for arm in arms:
    r = res['arms'][arm]
    sd = max(r['step_us'][1], ref['step_us'][1])
    r['step_gain_us'] = ref['step_us'][0] - r['step_us'][0]
    r['step_gain_in_sd'] = r['step_gain_us'] / sd if sd > 0 else 0.0
    print('limit %-7s kernel %.2f +- %.2f us   step %.2f +- %.2f us   gain over %s %+.2f us = %+.1f sd (%+.2f %%)'
          % (arm, *r['kernel_us'], *r['step_us'], arms[0], r['step_gain_us'], r['step_gain_in_sd'], 100 * r['step_gain_us'] / ref['step_us'][0]))
print(json.dumps(res))
