#!/usr/bin/env python3
"""What the moments per label cost on one GPU (csrc/k_moments.h, host_moments.h):

    python tools/bench_moments.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216,noisy]

Three label maps at size^3, each the neargrid assignment of a density generated on the device, the centres its maxima:

    atoms8    the 8-atom cubic cell of bench.py                          (n = 8: the LDS route)
    atoms216  the 216-atom cell of bench.py's user leg                   (n = 216: the LDS route; also forced through the global
                                                                          route by padding the centres past the bin limit)
    noisy     the 8-atom cell with uniform noise in its vacuum, per Bader volume (n in the millions: the global route)

Per case, warm-up first, then median / min / max of the repeats of
    moment_sum_ms    xb_moment_sum, host clock around the call (it returns with its results on the host: the transfer of
                     3 n centres in and 11 n numbers out is inside)
    kernel_ms        the kernels of the same calls alone (XB_TIMER_MOMENTS of xb_kernel_time, HIP events)
    charge_sum_ms    xb_charge_sum on the same labels, the same way: the yardstick, it streams the same 12 B per voxel
and ratio = kernel_ms / charge_sum_ms (medians), roofline_share = (12 B * voxels / kernel time) / --hbm-gbs.

Every timed step runs under --limit seconds (a watchdog thread ends the process with status 124); run the tool under a limit
from outside as well.  Prints one JSON line."""
import argparse
import json
import os
import re
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import _lib, synth                       # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402

with open(os.path.join(os.path.dirname(_lib.__file__), 'csrc', 'k_moments.h')) as _f:
    MS_BINS = int(re.search(r'^#define MS_BINS (\d+)', _f.read(), re.M).group(1))


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_moments: {what} exceeded {seconds} s\n')
        sys.stderr.flush()
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def stats(x):
    return {'median': statistics.median(x), 'min': min(x), 'max': max(x)}


def timed(ctx, fn, warmup, repeats, limit, what, timer=None):
    wall, dev = [], []
    for k in range(warmup + repeats):
        if timer is not None:
            ctx.kernel_time_reset()
        ctx.sync()
        t0 = time.perf_counter()
        limited(limit, what, fn)
        ctx.sync()
        if k >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            if timer is not None:
                dev.append(ctx.kernel_time(timer)[0])
    return stats(wall), (stats(dev) if dev else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--cases', default='8,216,noisy')
    ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='the HBM bandwidth the roofline share refers to (MI355X: 8 TB/s peak)')
    a = ap.parse_args()
    shape = (a.size,) * 3
    nvox = float(np.prod(shape))
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    out = {'shape': list(shape), 'ms_bins': MS_BINS, 'hbm_gbs': a.hbm_gbs, 'cases': {}}
    for case in a.cases.split(','):
        atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
        if case == 'noisy':
            rho = ctx.download_density()
            rho += np.where(rho < 0.2, 2e-3 * np.random.default_rng(11).random(shape), 0.0)
            ctx.upload_density(rho)
            del rho
        ctx.vacuum_assign(None, vv)
        n = limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
        centres = np.dot(ctx.maxima() / np.array(shape, dtype=np.float64), lat)
        routes = [('', centres)]
        if n <= MS_BINS:        # the same labels through the global route: centres nobody carries past the bin limit
            routes.append(('_global_route', np.concatenate([centres, np.zeros((MS_BINS + 1 - n, 3))])))
        res = {'n_labels': int(n)}
        ctx.enable_timing(only=[_lib.XB_TIMER_MOMENTS])
        for tag, cen in routes:
            wall, dev = timed(ctx, lambda: ctx.moment_sum(lat, cen, vv), a.warmup, a.repeats, a.limit, 'moment_sum', timer=_lib.XB_TIMER_MOMENTS)
            res['moment_sum_ms' + tag], res['kernel_ms' + tag] = wall, dev
        ctx.enable_timing(False)
        res['charge_sum_ms'], _ = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        for tag, _ in routes:
            k = res['kernel_ms' + tag]['median']
            res['ratio' + tag] = k / res['charge_sum_ms']['median']
            res['roofline_share' + tag] = 12.0 * nvox / (k * 1e-3) / (a.hbm_gbs * 1e9)
        mo, vo = ctx.moment_sum(lat, centres, vv)
        ch, _ = ctx.charge_sum(vv, n)
        res['m0_minus_charge_max'] = float(np.max(np.abs(mo[:, 0] - ch)))
        res['dipole_norm_max'] = float(np.max(np.linalg.norm(mo[:, 1:4], axis=1)))
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
