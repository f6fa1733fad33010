#!/usr/bin/env python3
"""What the Voronoi partition costs on one GPU (csrc/k_voronoi.h, host_voronoi.h):

    python tools/bench_voronoi.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216]

Two sets of atoms at size^3 in the cubic cell of bench.py, the density generated on the device:

    8     the 8-atom cell of bench.py
    216   the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (xb_voronoi_assign has no timer slot; it returns with its statistics on the host):
    voronoi_ms        xb_voronoi_assign by the candidate route
    full_search_ms    the same call with XB_VORONOI_FULL_SEARCH: every tile searches all 27 n images
    charge_sum_ms     xb_charge_sum on the resulting map   (the yardsticks: one streaming pass of 12 B per voxel each,
    moment_sum_ms     xb_moment_sum on the resulting map    the second with a 27-image search per voxel)
and the candidate statistics, speedup = full_search_ms / voronoi_ms (medians), and whether the two routes gave the same map.

Every timed step runs under --limit seconds (a watchdog thread ends the process with status 124); run the tool under a limit
from outside as well.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import _lib, synth                       # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_voronoi: {what} exceeded {seconds} s\n')
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


def timed(ctx, fn, warmup, repeats, limit, what):
    wall = []
    for k in range(warmup + repeats):
        ctx.sync()
        t0 = time.perf_counter()
        limited(limit, what, fn)
        ctx.sync()
        if k >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
    return stats(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--cases', default='8,216')
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    out = {'shape': list(shape), 'cand_max': _lib.XB_VORONOI_CAND_MAX, 'cases': {}}
    for case in a.cases.split(','):
        atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        atoms = synth.atoms_cartesian(atoms5, lat)
        n = atoms.shape[0]
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
        res = {'n_atoms': int(n), 'images': 27 * int(n)}
        res['full_search_ms'] = timed(ctx, lambda: ctx.voronoi_assign(lat, atoms, full_search=True, want_stats=False), a.warmup,
                                      a.repeats, a.limit, 'full search')
        full = ctx.download_labels(np.int32)
        res['voronoi_ms'] = timed(ctx, lambda: ctx.voronoi_assign(lat, atoms, want_stats=False), a.warmup, a.repeats, a.limit,
                                  'candidate route')
        res['stats'] = ctx.voronoi_assign(lat, atoms)
        res['routes_agree'] = bool(np.array_equal(ctx.download_labels(np.int32), full))
        del full
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        res['moment_sum_ms'] = timed(ctx, lambda: ctx.moment_sum(lat, atoms, vv), a.warmup, a.repeats, a.limit, 'moment_sum')
        res['speedup'] = res['full_search_ms']['median'] / res['voronoi_ms']['median']
        _, vo = ctx.charge_sum(vv, n)
        res['volume_min_max'] = [float(vo.min()), float(vo.max())]
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
