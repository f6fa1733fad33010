#!/usr/bin/env python3
"""What the Hirshfeld charges and fields cost on one GPU (csrc/k_hirshfeld.h, host_hirshfeld.h):

    python tools/bench_hirshfeld.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216] [--r-cut 3.0] [--knots 4096]

Two sets of atoms at size^3 in the cubic cell of bench.py, the density generated on the device, the pro-atoms sampled from synth's
own atom profile (one species per atom):

    8     the 8-atom cell of bench.py
    216   the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    setup_ms                    xb_hirshfeld_setup: the image list, the tables, the position table (host work and uploads)
    sum_ms, full_sum_ms         xb_hirshfeld_sum by the candidate route and with XB_HIRSHFELD_FULL_SEARCH
    promolecule_ms, full_...    xb_hirshfeld_field(XB_HIRSHFELD_PROMOLECULE) into device memory, both routes
    deformation_ms, full_...    xb_hirshfeld_field(XB_HIRSHFELD_DEFORMATION) into device memory, both routes
    voronoi_ms, charge_sum_ms   the yardsticks on the same case: xb_voronoi_assign and xb_charge_sum on its map
and the candidate statistics, the speedups full / candidate (medians), and whether the two routes gave the same bits (both fields
compared on the device's copy brought to the host; the sums within 1e-12 of each other, relative -- their order is free).

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

from pybader_amd import _lib, device, synth                       # noqa: E402
from pybader_amd.hirshfeld import ProAtoms                        # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_hirshfeld: {what} exceeded {seconds} s\n')
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
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    field = device.DeviceArray(ctx, shape, np.float64)
    out = {'shape': list(shape), 'cand_max': _lib.XB_HIRSHFELD_CAND_MAX, 'r_cut': a.r_cut, 'knots': a.knots, 'cases': {}}
    PRO, DEF = _lib.XB_HIRSHFELD_PROMOLECULE, _lib.XB_HIRSHFELD_DEFORMATION
    for case in a.cases.split(','):
        atoms5 = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        atoms = synth.atoms_cartesian(atoms5, lat)
        n = atoms.shape[0]
        species = np.arange(n, dtype=np.int32)
        pro = synth_proatoms(atoms5, a.r_cut, a.knots)
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms5, synth.BACKGROUND))
        res = {'n_atoms': int(n), 'images': int(_lib.hirshfeld_images(lat, atoms, species, pro.r_cut).shape[0])}
        res['setup_ms'] = timed(ctx, lambda: ctx.hirshfeld_setup(lat, atoms, species, pro.tables, pro.r_cut), a.warmup, a.repeats,
                                a.limit, 'setup')
        bits = {}
        for full, tag in ((True, 'full_'), (False, '')):
            res[tag + 'sum_ms'] = timed(ctx, lambda: ctx.hirshfeld_sum(vv, full), a.warmup, a.repeats, a.limit, tag + 'sum')
            bits[tag + 'sum'] = ctx.hirshfeld_sum(vv, full)
            for mode, name in ((PRO, 'promolecule'), (DEF, 'deformation')):
                res[tag + name + '_ms'] = timed(ctx, lambda: ctx.hirshfeld_field(mode, full, out=field), a.warmup, a.repeats, a.limit,
                                                tag + name)
                bits[tag + name] = field.to_host()
        res['stats'] = bits['sum'][3]
        res['fields_agree'] = bool(all(np.array_equal(bits[k].view(np.uint64), bits['full_' + k].view(np.uint64))
                                       for k in ('promolecule', 'deformation')))
        ch, fch = bits['sum'][0], bits['full_sum'][0]
        res['sums_agree'] = bool(np.all(np.abs(ch - fch) <= 1e-12 * np.abs(ch)))
        res['charge_min_max'] = [float(ch.min()), float(ch.max())]
        res['charge_total_and_rest'] = [float(ch.sum()), float(bits['sum'][2][0])]
        res['deformation_abs_max'] = float(np.abs(bits['deformation']).max())
        del bits
        for k in ('sum', 'promolecule', 'deformation'):
            res['speedup_' + k] = res['full_' + k + '_ms']['median'] / res[k + '_ms']['median']
        res['voronoi_ms'] = timed(ctx, lambda: ctx.voronoi_assign(lat, atoms, want_stats=False), a.warmup, a.repeats, a.limit, 'voronoi')
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
