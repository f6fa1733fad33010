#!/usr/bin/env python3
"""What the stockholder moments cost on one GPU (csrc/k_stockmom.h, host_stockmom.h), beside the Hirshfeld sum and one MBIS iteration
on the same geometry in the same run:

    python tools/bench_stockmom.py [--size 512] [--warmup 1] [--repeats 3] [--limit 300] [--cases 8,216] [--r-cut 3.0]
                                   [--routes reduced] [--small-size 64] [--small-routes reduced,direct,full_search]

Two sets of atoms at size^3 in the cubic cell of bench.py, the density generated on the device:

    8     the 8-atom cell of bench.py
    216   the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    sum_ms              xb_hirshfeld_sum on an ISA setup of the same atoms and cutoff (the kernel of DESIGN.md section 19)
    mbis_iteration_ms   xb_mbis_iterate, (5 iterations - 1 iteration) / 4 of the medians (the kernel of section 24, one shell)
    moments_ms          xb_stockholder_moments per kind of setup (hirshfeld: a table of 4096 knots per atom; isa; mbis) and route
    over_mbis           moments_ms / mbis_iteration_ms of the same run
The second implementations are timed at --small-size^3 (0: not at all): XB_STOCKMOM_DIRECT sends twelve global atomics per pair
onto a few addresses, XB_HIRSHFELD_FULL_SEARCH runs every tile over the whole image list; at 512^3 either takes minutes.

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

from pybader_amd import _lib, isa, mbis, synth                       # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_stockmom: {what} exceeded {seconds} s\n')
        sys.stderr.flush()
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def progress(what, value):
    """what is known so far, to stderr: a run that is cut short still says what it measured"""
    sys.stderr.write(f'bench_stockmom: {what}: {json.dumps(value)}\n')
    sys.stderr.flush()


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


ROUTES = {'reduced': {}, 'direct': {'direct': True}, 'full_search': {'full_search': True}}


def setups(ctx, lat, atoms, rc, shape, bound, vv, E):
    """kind -> the call that makes that kind's setup on the context"""
    n = atoms.shape[0]
    K = isa.default_shells(lat, shape, rc)
    sh = np.ones(n, np.int32)
    N0, s0 = mbis.default_initial(sh)
    x = np.arange(4097, dtype=np.float64) / 4096.0
    tables = np.tile(np.exp(-4.0 * x) * (1.0 - x), (n, 1))      # (one table per atom, as ISA's; the last knot is 0)
    return {
        'hirshfeld': lambda: ctx.hirshfeld_setup(lat, atoms, np.arange(n, dtype=np.int32), tables, rc),
        'isa': lambda: ctx.isa_setup(lat, atoms, rc, K, bound),
        'mbis': lambda: ctx.mbis_setup(lat, atoms, rc, sh, E, 256, N0, s0, bound, vv),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--limit', type=float, default=300.0)
    ap.add_argument('--cases', default='8,216')
    ap.add_argument('--r-cut', type=float, default=3.0)
    ap.add_argument('--routes', default='reduced')
    ap.add_argument('--small-size', type=int, default=64)
    ap.add_argument('--small-routes', default='reduced,direct,full_search')
    a = ap.parse_args()
    lat = synth.CUBIC6
    ctx = _lib.default_context()
    E = mbis.exp_table()
    out = {'r_cut': a.r_cut, 'cases': {}}
    for size in dict.fromkeys([a.size] + ([a.small_size] if a.small_size > 0 else [])):
        shape = (size,) * 3
        vv = abs(np.linalg.det(lat)) / np.prod(shape)
        routes = [r for r in a.routes.split(',') if r] if size == a.size else []
        if size == a.small_size:
            routes = list(dict.fromkeys(routes + [r for r in a.small_routes.split(',') if r]))
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
        for case in a.cases.split(','):
            atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
            atoms = synth.atoms_cartesian(atoms5, lat)
            rc = np.full(atoms.shape[0], a.r_cut)
            limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
            bound = ctx.density_absmax()
            make = setups(ctx, lat, atoms, rc, shape, bound, vv, E)
            key = f'{case}@{size}'
            res = {'n_atoms': int(atoms.shape[0]), 'shape': list(shape), 'rho_bound': bound}
            # the yardsticks of the same run: the Hirshfeld sum and one MBIS iteration, both kernels as they were
            make['isa']()
            res['sum_ms'] = timed(ctx, lambda: ctx.hirshfeld_sum(vv), a.warmup, a.repeats, a.limit, 'sum')
            make['mbis']()
            it = {m: timed(ctx, lambda: ctx.mbis_iterate(m), a.warmup, a.repeats, a.limit, f'mbis {m}') for m in (1, 5)}
            res['mbis_iteration_ms'] = (it[5]['median'] - it[1]['median']) / 4
            progress(key, res)
            bins = {}
            for kind in ('hirshfeld', 'isa', 'mbis'):
                make[kind]()
                r = {}
                for route in routes:
                    t = timed(ctx, lambda: ctx.stockholder_moments(bound, **ROUTES[route]), a.warmup, a.repeats, a.limit, f'{kind} {route}')
                    got = ctx.stockholder_moments(bound, **ROUTES[route])
                    bins.setdefault(kind, []).append(got[0])
                    r[route] = {'moments_ms': t, 'over_mbis': t['median'] / res['mbis_iteration_ms'], 'over_sum': t['median'] / res['sum_ms']['median'],
                                'info': got[1], 'stats': got[2]}
                    progress(f'{key} {kind} {route}', r[route])
                res[kind] = r
            res['routes_agree'] = bool(all(np.array_equal(b, v[0]) for v in bins.values() for b in v))
            out['cases'][key] = res
    print(json.dumps(out))


if __name__ == '__main__':
    main()
