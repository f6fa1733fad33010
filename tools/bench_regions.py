#!/usr/bin/env python3
"""What the connected regions cost on one GPU (csrc/k_regions.h, host_regions.h), next to the critical points, the NCI sums and the
charge sums of the same build on the same grid:

    python tools/bench_regions.py [--size 512] [--warmup 1] [--repeats 5] [--limit 120] [--cases 8,216,noise]

Three densities at size^3 in the cubic cell of bench.py:

    8       the 8-atom cell of bench.py (generated on the device)
    216     the 216-atom cell of bench.py's user leg (generated on the device)
    noise   the background of bench.py times (1 + 0.5 uniform noise): a vacuum with nothing but ripples (uploaded)

Per case and per membership -- ABOVE at the median of the field, ABOVE at 0.001, NCI with the default cuts -- and per route (tiles,
XB_DOMAINS_GLOBAL), warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait
for the device (the calls have no timer slot):
    label_ms      xb_regions_label: membership and tile union-find (or parent[v] = v), the seam / global unions, the flatten and
                  the numbering (count, three scan launches, emit, rewrite), one call
    stages_ms     the same call with XB_DOMAINS_TIMES: events on the stream around its four stages -- tile (membership and the
                  union-find in LDS, or parent[v] = v), link (the unions in global memory), flatten, numbering (with its wait
                  for the component count and the allocation of the seeds) --, the median of the repeats
    sums_ms       xb_regions_sums (classes in NCI mode)
    shares_ms     xb_regions_shares against the atom map (a dense table while m n <= 2^24, else the key list)
and m, the member fraction, whether the two routes gave the same map, and critical_ms, nci_sum_ms, charge_sum_ms of the same build.

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

from pybader_amd import _lib, nci, synth                                # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_regions: {what} exceeded {seconds} s\n')
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
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--cases', default='8,216,noise')
    a = ap.parse_args()
    shape = (a.size,) * 3
    nvox = float(np.prod(shape))
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    cuts = (nci.S_CUT, nci.RHO_CUT, nci.RHO_SPLIT)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    out = {'shape': list(shape), 'cuts': list(cuts), 'cases': {}}
    for case in a.cases.split(','):
        res = {}
        if case == 'noise':
            rho = synth.BACKGROUND * (1.0 + 0.5 * np.random.default_rng(7).random(shape))
            limited(a.limit, 'density', lambda: ctx.upload_density(rho))
            median = float(np.median(rho[::4, ::4, ::4]))
            del rho
            n = 1
            ctx.upload_labels(np.zeros(shape, np.int8))
        else:
            atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
            limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
            median = float(np.median(ctx.download_density()[::4, ::4, ::4]))
            ctx.vacuum_assign(None, vv)
            limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
            maxima = np.dot(ctx.maxima() / np.array(shape, dtype=np.float64), lat)
            owner, _ = _lib.atom_assign(maxima, synth.atoms_cartesian(atoms, lat), lat)
            ctx.volume_assign(owner)
            n = atoms.shape[0]
        res['n_labels'] = int(n)
        for name, mode, level in (('above_median', _lib.XB_DOMAINS_ABOVE, median), ('above_0.001', _lib.XB_DOMAINS_ABOVE, 0.001),
                                  ('nci', _lib.XB_DOMAINS_NCI, 0.0)):
            r = {'level': level}
            is_nci = mode == _lib.XB_DOMAINS_NCI
            maps = []
            for route, key in ((False, 'tiles'), (True, 'global')):
                def label(times=False):
                    return ctx.regions_label(mode, None, level, lat if is_nci else None, cuts[0], cuts[1], global_route=route, times=times)
                r[f'label_{key}_ms'] = timed(ctx, label, a.warmup, a.repeats, a.limit, f'{name} label, {key}')
                stage = []
                for _ in range(a.repeats):
                    m = limited(a.limit, f'{name} label with events, {key}', lambda: label(True))
                    stage.append(ctx.regions_times())
                r[f'stages_{key}_ms'] = dict(zip(('tile', 'link', 'flatten', 'numbering'), np.median(np.array(stage), axis=0).tolist()))
                maps.append(synth.sha256(ctx.regions_map()))
                r['m'] = m
                r[f'sums_{key}_ms'] = timed(ctx, lambda: ctx.regions_sums(m, vv, cuts[2] if is_nci else None), a.warmup, a.repeats, a.limit,
                                            f'{name} sums')
                r[f'shares_{key}_ms'] = timed(ctx, lambda: ctx.regions_shares(n), a.warmup, a.repeats, a.limit, f'{name} shares')
            r['member_fraction'] = float(ctx.regions_sums(r['m'], vv)[1].sum() / nvox) if r['m'] else 0.0
            r['share_route'] = 'dense' if r['m'] * n <= _lib.XB_DOMAINS_SHARE_CELLS else 'list'
            r['routes_agree'] = maps[0] == maps[1]
            res[name] = r
            ctx.regions_release()
        res['critical_ms'] = timed(ctx, lambda: ctx.critical_points(), a.warmup, a.repeats, a.limit, 'critical points')
        res['nci_sum_ms'] = timed(ctx, lambda: ctx.nci_sum(lat, n, vv, *cuts), a.warmup, a.repeats, a.limit, 'nci sums')
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
