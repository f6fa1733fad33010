#!/usr/bin/env python3
"""What IGM costs on one GPU (csrc/k_igm.h, host_igm.h), next to the Hirshfeld field and sums and the DORI field of the same
build on the same grid in the same run:

    python tools/bench_igm.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216] [--r-cut 3.0] [--knots 4096]

Two densities at size^3 in the cubic cell of bench.py, generated on the device, with pro-atoms sampled from the generator's own
atom profile (one species per atom), as tools/bench_hirshfeld.py makes them:

    8       the 8-atom cell of bench.py, fragments {0..3}, {4..7}
    216     the 216-atom cell of bench.py's user leg, in two and in four fragments of consecutive atoms

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    pro_ms, stockholder_ms               xb_igm_field, both fields into two device arrays, two fragments, the candidate route
    pro_f4_ms, stockholder_f4_ms         the same with four fragments (the second instantiation)
    stockholder_inter_ms                 delta-g_inter alone
    igm_sum_ms                           xb_igm_sum of delta-g_inter >= cut on the nearest-atom label map
    promolecule_ms, hirshfeld_sum_ms     xb_hirshfeld_field (promolecule) and xb_hirshfeld_sum on the same setup
    dori_field_ms, nci_field_ms          xb_dori_field (gamma and x) and xb_nci_field into two device arrays
and, once per case outside the timing, whether the forced full search gives the same bits (--check-full; slow at 216 atoms), the
maxima of both fields and the voxels of the region per class.

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

from pybader_amd import _lib, device, dori, igm, synth      # noqa: E402
from pybader_amd.hirshfeld import ProAtoms                    # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_igm: {what} exceeded {seconds} s\n')
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


def synth_proatoms(atoms5, r_cut, knots):
    """A max(0, 1 - r^2 / (2048 s^2))^1024 at the r^2-uniform knots, one species per atom, the last knot 0"""
    x = np.arange(knots + 1, dtype=np.float64) * (r_cut * r_cut) / knots
    tab = np.zeros((atoms5.shape[0], knots + 1))
    for s, a in enumerate(atoms5):
        tab[s] = a[4] * np.maximum(1.0 - x / (2048.0 * a[3] * a[3]), 0.0) ** 1024
    tab[:, -1] = 0.0
    return ProAtoms(tab, np.full(atoms5.shape[0], float(r_cut)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--limit', type=float, default=120.0)
    ap.add_argument('--cases', default='8,216')
    ap.add_argument('--r-cut', type=float, default=3.0)
    ap.add_argument('--knots', type=int, default=4096)
    ap.add_argument('--check-full', action='store_true', help='compare with the forced full search once per case')
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    fields = [device.DeviceArray(ctx, shape, np.float64) for _ in range(2)]
    other = [device.DeviceArray(ctx, shape, np.float64) for _ in range(2)]
    out = {'shape': list(shape), 'r_cut': a.r_cut, 'knots': a.knots, 'p_min': igm.P_MIN, 'cases': {}}
    PRO, STOCK = _lib.XB_IGM_PRO, _lib.XB_IGM_STOCKHOLDER
    for case in a.cases.split(','):
        atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        atoms = synth.atoms_cartesian(atoms5, lat)
        n = atoms.shape[0]
        species = np.arange(n, dtype=np.int32)
        pro = synth_proatoms(atoms5, a.r_cut, a.knots)
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
        limited(a.limit, 'setup', lambda: ctx.hirshfeld_setup(lat, atoms, species, pro.tables, pro.r_cut))
        limited(a.limit, 'labels', lambda: ctx.voronoi_assign(lat, atoms, want_stats=False))      # the nearest-atom map
        res = {'n_atoms': int(n)}
        two, four = (np.arange(n) * 2 // n).astype(np.int32), (np.arange(n) * 4 // n).astype(np.int32)

        def field(mode, fr, F, full=False, outs=fields):
            return ctx.igm_field(lat, fr, mode, igm.P_MIN, full, out=outs, n_fragments=F)

        for mode, name in ((PRO, 'pro'), (STOCK, 'stockholder')):
            res[name + '_ms'] = timed(ctx, lambda: field(mode, two, 2), a.warmup, a.repeats, a.limit, name)
            res[name + '_f4_ms'] = timed(ctx, lambda: field(mode, four, 4), a.warmup, a.repeats, a.limit, name + ', four fragments')
        res['stockholder_inter_ms'] = timed(ctx, lambda: field(STOCK, two, 2, outs=[None, fields[1]]), a.warmup, a.repeats, a.limit,
                                            'delta-g_inter alone')
        res['stats'] = field(STOCK, two, 2)[2]
        dg, dgi = fields[0].to_host(), fields[1].to_host()
        res['dg_max'], res['dgi_max'], res['dg_min'], res['dgi_min'] = float(dg.max()), float(dgi.max()), float(dg.min()), float(dgi.min())
        res['inter_not_above_whole'] = bool((dgi <= dg + 1e-12 * (1.0 + np.abs(dg))).all())
        if a.check_full:
            field(STOCK, two, 2, full=True, outs=other)
            res['routes_agree'] = bool(np.array_equal(other[0].to_host().view(np.uint64), dg.view(np.uint64))
                                       and np.array_equal(other[1].to_host().view(np.uint64), dgi.view(np.uint64)))
        cut = 0.01 * res['dgi_max']
        del dg, dgi
        ctx.nci_field(lat, out=other)                  # other[1] = x, the colour
        res['igm_sum_ms'] = timed(ctx, lambda: ctx.igm_sum(fields[1], other[1], n, vv, cut, igm.RHO_SPLIT), a.warmup, a.repeats, a.limit,
                                  'igm sums')
        count, _, integral = ctx.igm_sum(fields[1], other[1], n, vv, cut, igm.RHO_SPLIT)
        res['cut'], res['region_voxels_per_class'] = cut, count.sum(axis=0).tolist()
        res['region_integral_per_class'] = integral.sum(axis=0).tolist()
        res['promolecule_ms'] = timed(ctx, lambda: ctx.hirshfeld_field(_lib.XB_HIRSHFELD_PROMOLECULE, out=other[0]), a.warmup, a.repeats,
                                      a.limit, 'promolecule')
        res['hirshfeld_sum_ms'] = timed(ctx, lambda: ctx.hirshfeld_sum(vv), a.warmup, a.repeats, a.limit, 'hirshfeld sums')
        res['dori_field_ms'] = timed(ctx, lambda: ctx.dori_field(lat, dori.RHO_MIN, out=other), a.warmup, a.repeats, a.limit, 'dori field')
        res['nci_field_ms'] = timed(ctx, lambda: ctx.nci_field(lat, out=other), a.warmup, a.repeats, a.limit, 'nci field')
        for name in ('pro', 'stockholder'):
            res[name + '_over_promolecule'] = res[name + '_ms']['median'] / res['promolecule_ms']['median']
            res[name + '_over_hirshfeld_sum'] = res[name + '_ms']['median'] / res['hirshfeld_sum_ms']['median']
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
