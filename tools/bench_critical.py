#!/usr/bin/env python3
"""What the critical points and the bond graph cost on one GPU (csrc/k_critical.h, host_critical.h):

    python tools/bench_critical.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216,noisy]

Three densities at size^3 in the cubic cell of bench.py, generated on the device:

    8       the 8-atom cell of bench.py
    216     the 216-atom cell of bench.py's user leg
    noisy   the 8-atom cell with uniform noise in its vacuum (rho < 0.2): a third of the vacuum's voxels are critical, the list
            outgrows its first allocation and the pass runs twice; with the vacuum tolerance 0.2 the noise is left out again

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot; they return with their results on the host, so the record transfer and the host's sort
of the records are inside):
    critical_ms          xb_critical_points through the table
    critical_flood_ms    the same with XB_CRITICAL_FLOOD: components by flood fill in registers
    critical_vacuum_ms   (noisy) through the table with the vacuum tolerance 0.2
    bonds_ms             xb_critical_bonds on the atom map (noisy: on the Bader volumes)
    charge_sum_ms        xb_charge_sum on the same map         (the yardsticks: streaming passes of 12 B per voxel,
    adjacency_ms         xb_adjacency on the same map           one and two of them)
and the counts, the list's length, whether table and flood fill gave the same list, the Euler sum (0), and roofline_share =
8 B per voxel / critical_ms against --hbm-gbs.

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

from pybader_amd import _lib, adjacency, synth                       # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402

VACUUM_TOL = 0.2


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_critical: {what} exceeded {seconds} s\n')
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
    ap.add_argument('--cases', default='8,216,noisy')
    ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='the HBM bandwidth the roofline share refers to (MI355X: 8 TB/s peak)')
    a = ap.parse_args()
    shape = (a.size,) * 3
    nvox = float(np.prod(shape))
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    dirs, _ = adjacency.active_directions(vl)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    out = {'shape': list(shape), 'hbm_gbs': a.hbm_gbs, 'cases': {}}
    for case in a.cases.split(','):
        atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
        if case == 'noisy':
            rho = ctx.download_density()
            rho += np.where(rho < VACUUM_TOL, 2e-3 * np.random.default_rng(11).random(shape), 0.0)
            ctx.upload_density(rho)
            del rho
        ctx.vacuum_assign(None, vv)
        n = limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
        res = {'n_maxima': int(n)}
        if case != 'noisy':       # per atom: every maximum to its nearest atom, as Bader.bader_to_atom_distance does
            maxima = np.dot(ctx.maxima() / np.array(shape, dtype=np.float64), lat)
            owner, _ = _lib.atom_assign(maxima, synth.atoms_cartesian(atoms, lat), lat)
            ctx.volume_assign(owner)
            n = atoms.shape[0]
        res['n_labels'] = int(n)
        res['critical_flood_ms'] = timed(ctx, lambda: ctx.critical_points(flood=True), a.warmup, a.repeats, a.limit, 'flood fill')
        flood = ctx.critical_points(flood=True)
        res['critical_ms'] = timed(ctx, lambda: ctx.critical_points(), a.warmup, a.repeats, a.limit, 'table')
        table = ctx.critical_points()
        res['implementations_agree'] = bool(all(np.array_equal(x, y) for x, y in zip(table, flood)))
        del flood
        counts = table[0]
        res['counts'] = [int(v) for v in counts]
        res['list'] = int(table[1].size)
        res['euler'] = int(counts[_lib.XB_CRITICAL_MINIMA] - counts[_lib.XB_CRITICAL_RING_SUM] + counts[_lib.XB_CRITICAL_BOND_SUM] -
                           counts[_lib.XB_CRITICAL_MAXIMA])
        del table
        res['roofline_share'] = 8.0 * nvox / (res['critical_ms']['median'] * 1e-3) / (a.hbm_gbs * 1e9)
        if case == 'noisy':
            res['critical_vacuum_ms'] = timed(ctx, lambda: ctx.critical_points(VACUUM_TOL), a.warmup, a.repeats, a.limit, 'table, vacuum')
            res['list_vacuum'] = int(ctx.critical_points(VACUUM_TOL)[1].size)
            res['roofline_share_vacuum'] = 8.0 * nvox / (res['critical_vacuum_ms']['median'] * 1e-3) / (a.hbm_gbs * 1e9)
        ctx.critical_points()     # (the list xb_critical_bonds works on: the whole one, the noise included)
        res['bonds_ms'] = timed(ctx, lambda: ctx.critical_bonds(n), a.warmup, a.repeats, a.limit, 'bonds')
        pairs, saddles, _, _, same = ctx.critical_bonds(n)
        res['bond_pairs'], res['bond_saddles'], res['same_basin'] = int(pairs.shape[0]), int(saddles.sum()), int(same)
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        res['adjacency_ms'] = timed(ctx, lambda: ctx.adjacency(dirs, n), a.warmup, a.repeats, a.limit, 'adjacency')
        res['touching_pairs'] = int(ctx.adjacency(dirs, n)[0].shape[0])
        ctx.adjacency_release()
        held = ctx.memory_stats()[2]
        ctx.critical_release()
        res['list_bytes'] = int(held - ctx.memory_stats()[2])
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
