#!/usr/bin/env python3
"""What the iterative stockholder atoms cost on one GPU (csrc/k_isa.h, host_isa.h):

    python tools/bench_isa.py [--size 512] [--warmup 2] [--repeats 7] [--limit 300] [--cases 8,216] [--r-cut 3.0] [--shells K]
                              [--tol 1e-6] [--max-iter 2000]

Two sets of atoms at size^3 in the cubic cell of bench.py, the density generated on the device:

    8     the 8-atom cell of bench.py
    216   the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    setup_ms                  xb_isa_setup: the image list, the tables, the position table, the counting pass
    iterate1_ms, iterate9_ms  xb_isa_iterate of 1 and of 9 iterations, per route: windows (the default), direct, full_search
    iteration_ms              (iterate9 - iterate1) / 8 of the medians: one shell pass and one update kernel, without the call's
                              fixed cost (the fills, the read-back, the wait)
    sum_ms                    xb_hirshfeld_sum on the same setup, the yardstick: k_hirshfeld<HS_SUM>, the kernel an iteration is
                              modelled on, unchanged by this feature
    converge                  isa.isa_charges to --tol: iterations, wall seconds, charges, the largest residual
The split of an iteration into the shell pass and the update kernel, and the counting pass alone, come from a kernel trace of this
tool (rocprofv3 --kernel-trace --stats -- python tools/bench_isa.py --repeats 1 --warmup 0 --max-iter 0).

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

from pybader_amd import _lib, isa, synth                       # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_isa: {what} exceeded {seconds} s\n')
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
    sys.stderr.write(f'bench_isa: {what}: {json.dumps(value)}\n')
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


ROUTES = {'windows': {}, 'direct': {'direct': True}, 'full_search': {'full_search': True}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--limit', type=float, default=300.0)
    ap.add_argument('--cases', default='8,216')
    ap.add_argument('--routes', default='windows,direct,full_search')
    ap.add_argument('--r-cut', type=float, default=3.0)
    ap.add_argument('--shells', type=int, default=0)
    ap.add_argument('--tol', type=float, default=1e-6)
    ap.add_argument('--max-iter', type=int, default=2000)
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.default_context()
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    out = {'shape': list(shape), 'r_cut': a.r_cut, 'tol': a.tol, 'cases': {}}
    for case in a.cases.split(','):
        atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        atoms = synth.atoms_cartesian(atoms5, lat)
        n = atoms.shape[0]
        rc = np.full(n, a.r_cut)
        K = a.shells or isa.default_shells(lat, shape, rc)
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
        bound = ctx.density_absmax()
        res = {'n_atoms': int(n), 'shells': int(K), 'rho_bound': bound}
        res['setup_ms'] = timed(ctx, lambda: ctx.isa_setup(lat, atoms, rc, K, bound), a.warmup, a.repeats, a.limit, 'setup')
        res['info'] = ctx.isa_setup(lat, atoms, rc, K, bound)
        res['sum_ms'] = timed(ctx, lambda: ctx.hirshfeld_sum(vv), a.warmup, a.repeats, a.limit, 'sum')
        progress(case, {k: res[k] for k in ('shells', 'info', 'setup_ms', 'sum_ms')})
        rows = {}
        for route in a.routes.split(','):
            kw = ROUTES[route]
            r = {}
            for m in (1, 9):
                r[f'iterate{m}_ms'] = timed(ctx, lambda: ctx.isa_iterate(m, **kw), a.warmup, a.repeats, a.limit, f'{route} {m}')
            r['iteration_ms'] = (r['iterate9_ms']['median'] - r['iterate1_ms']['median']) / 8
            r['iteration_over_sum'] = r['iteration_ms'] / res['sum_ms']['median']
            ctx.isa_setup(lat, atoms, rc, K, bound)
            rows[route], r['stats'] = ctx.isa_iterate(3, **kw)
            res[route] = r
            progress(f'{case} {route}', r)
        res['routes_agree'] = bool(all(np.array_equal(v, rows[a.routes.split(',')[0]]) for v in rows.values()))
        if a.max_iter > 0:
            t0 = time.perf_counter()
            got = limited(a.limit, 'converge', lambda: converge(ctx, lat, atoms, rc, K, bound, vv, a.tol, a.max_iter))
            got['seconds'] = time.perf_counter() - t0
            res['converge'] = got
        out['cases'][case] = res
    print(json.dumps(out))


def converge(ctx, lat, atoms, rc, K, bound, vv, tol, max_iter, every=16):
    """isa_charges' loop on the resident density of the context (generated on the device: there is no array to hand over)"""
    info = ctx.isa_setup(lat, atoms, rc, K, bound)
    scale = 2.0 ** -info['e'] * vv
    last, done, hit = None, 0, None
    while done < max_iter and hit is None:
        q, _ = ctx.isa_iterate(min(every, max_iter - done))
        progress('converge', {'iterations': done + q.shape[0], 'change': None if last is None else float(np.max(np.abs(q[-1] * scale - last)))})
        for row in q.astype(np.float64) * scale:
            done += 1
            if last is not None and np.max(np.abs(row - last)) < tol:
                hit = done
                break
            last = row
    charge, volume, rest, _ = ctx.hirshfeld_sum(vv)
    return {'iterations': hit or done, 'converged': hit is not None, 'charge_min_max': [float(charge.min()), float(charge.max())],
            'charge_total_and_rest': [float(charge.sum()), float(rest[0])]}


if __name__ == '__main__':
    main()
