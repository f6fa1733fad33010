#!/usr/bin/env python3
"""What the minimal-basis iterative stockholder atoms cost on one GPU (csrc/k_mbis.h, host_mbis.h), beside the Hirshfeld sum and
the ISA iteration on the same geometry in the same build:

    python tools/bench_mbis.py [--size 512] [--warmup 1] [--repeats 3] [--limit 300] [--cases 8,216] [--r-cuts 3.0,5.0]
                               [--shells 1] [--routes reduced,direct] [--tol 1e-6] [--max-iter 500] [--skip 216@5.0]

Two sets of atoms at size^3 in the cubic cell of bench.py, the density generated on the device:

    8     the 8-atom cell of bench.py
    216   the 216-atom cell of bench.py's user leg

Per case and cutoff, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait
for the device (the calls have no timer slot):
    setup_ms                  xb_mbis_setup: the image list, the table, the position table, the counting pass
    iterate1_ms, iterate5_ms  xb_mbis_iterate of 1 and of 5 iterations, per route: reduced (the default), direct
    iteration_ms              (iterate5 - iterate1) / 4 of the medians: one shell pass and one update kernel, without the call's
                              fixed cost (the fills, the read-back, the wait)
    sum_ms                    xb_hirshfeld_sum on an ISA setup of the same atoms and cutoff: the yardstick of DESIGN.md sections 19, 23
    isa_iteration_ms          xb_isa_iterate likewise, (iterate5 - iterate1) / 4
    converge                  the iterations to --tol from the default start, wall seconds, charges, the tail beyond the cutoff

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
        sys.stderr.write(f'bench_mbis: {what} exceeded {seconds} s\n')
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
    sys.stderr.write(f'bench_mbis: {what}: {json.dumps(value)}\n')
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--limit', type=float, default=300.0)
    ap.add_argument('--cases', default='8,216')
    ap.add_argument('--r-cuts', default='3.0,5.0')
    ap.add_argument('--routes', default='reduced,direct')
    ap.add_argument('--shells', type=int, default=1)
    ap.add_argument('--tol', type=float, default=1e-6)
    ap.add_argument('--max-iter', type=int, default=500)
    ap.add_argument('--skip', default='', help='comma-separated case@r_cut pairs to leave out, e.g. 216@5.0')
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.default_context()
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    E = mbis.exp_table()
    out = {'shape': list(shape), 'tol': a.tol, 'shells': a.shells, 'cases': {}}
    for case in a.cases.split(','):
        atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        atoms = synth.atoms_cartesian(atoms5, lat)
        n = atoms.shape[0]
        sh = np.full(n, a.shells, np.int32)
        N0, s0 = mbis.default_initial(sh)
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
        bound = ctx.density_absmax()
        for r_cut in (float(x) for x in a.r_cuts.split(',')):
            key = f'{case}@{r_cut}'
            if key in a.skip.split(','):
                continue
            rc = np.full(n, r_cut)
            make = lambda: ctx.mbis_setup(lat, atoms, rc, sh, E, 256, N0, s0, bound, vv)
            res = {'n_atoms': int(n), 'r_cut': r_cut, 'rho_bound': bound}
            # the yardsticks: the Hirshfeld sum and an ISA iteration on the same atoms and cutoff
            K = isa.default_shells(lat, shape, rc)
            ctx.isa_setup(lat, atoms, rc, K, bound)
            res['sum_ms'] = timed(ctx, lambda: ctx.hirshfeld_sum(vv), a.warmup, a.repeats, a.limit, 'sum')
            isa_t = {m: timed(ctx, lambda: ctx.isa_iterate(m), a.warmup, a.repeats, a.limit, f'isa {m}') for m in (1, 5)}
            res['isa_shells'] = int(K)
            res['isa_iteration_ms'] = (isa_t[5]['median'] - isa_t[1]['median']) / 4
            res['setup_ms'] = timed(ctx, make, a.warmup, a.repeats, a.limit, 'setup')
            res['info'] = make()
            progress(key, res)
            rows = {}
            for route in a.routes.split(','):
                kw = ROUTES[route]
                r = {}
                for m in (1, 5):
                    r[f'iterate{m}_ms'] = timed(ctx, lambda: ctx.mbis_iterate(m, **kw), a.warmup, a.repeats, a.limit, f'{route} {m}')
                r['iteration_ms'] = (r['iterate5_ms']['median'] - r['iterate1_ms']['median']) / 4
                r['iteration_over_sum'] = r['iteration_ms'] / res['sum_ms']['median']
                r['iteration_over_isa'] = r['iteration_ms'] / res['isa_iteration_ms']
                make()
                got = ctx.mbis_iterate(3, **kw)
                rows[route], r['stats'] = got[0], got[3]
                res[route] = r
                progress(f'{key} {route}', r)
            res['routes_agree'] = bool(all(np.array_equal(v, rows[a.routes.split(',')[0]]) for v in rows.values()))
            if a.max_iter > 0:
                t0 = time.perf_counter()
                got = limited(a.limit, 'converge', lambda: converge(ctx, make, rc, vv, a.tol, a.max_iter))
                got['seconds'] = time.perf_counter() - t0
                res['converge'] = got
                progress(f'{key} converge', got)
            out['cases'][key] = res
    print(json.dumps(out))


def converge(ctx, make, rc, vv, tol, max_iter, every=8):
    """mbis_charges' loop on the resident density of the context (generated on the device: there is no array to hand over)"""
    info = make()
    last, done, hit, charge, rest = None, 0, None, None, None
    while done < max_iter and hit is None:
        q, v, r, _ = ctx.mbis_iterate(min(every, max_iter - done))
        for j in range(q.shape[0]):
            charge, _, rest = mbis._results(info, vv, q[j], v[j], r[j])
            done += 1
            if last is not None and np.max(np.abs(charge - last)) < tol:
                hit = done
                break
            last = charge
    N, sg, _ = ctx.mbis_params()
    return {'iterations': hit or done, 'converged': hit is not None, 'charge_min_max': [float(charge.min()), float(charge.max())],
            'charge_total_and_rest': [float(charge.sum()), float(rest[0])], 'tail_max': float(mbis.tail(N, sg, rc).max())}


if __name__ == '__main__':
    main()
