#!/usr/bin/env python3
"""What the Laplacian of the density costs on one GPU (csrc/k_stencil.h, host_stencil.h):

    python tools/bench_laplacian.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216]

Two densities at size^3 in the cubic cell of bench.py, generated on the device:

    8       the 8-atom cell of bench.py
    216     the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    field_ms, field_gather_ms      xb_laplacian_field into one device array, through the tiles and through XB_STENCIL_GATHER
    sum_ms, sum_gather_ms          xb_laplacian_sum on the atom map, both routes
    points_ms                      xb_stencil_points on the list of xb_critical_points
    charge_sum_ms                  xb_charge_sum on the same map           (the yardsticks: streaming passes of 12 and of
    critical_ms                    xb_critical_points on the same density    8 B per voxel)
and whether the two routes gave the same field, the largest |L| / L_abs over the atoms, the list's length, and the shares of the
rooflines: 16 B per voxel for the field, 12 B per voxel for the sums, against --hbm-gbs.

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

from pybader_amd import _lib, device, synth                            # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_laplacian: {what} exceeded {seconds} s\n')
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
    ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='the HBM bandwidth the roofline shares refer to (MI355X: 8 TB/s peak)')
    a = ap.parse_args()
    shape = (a.size,) * 3
    nvox = float(np.prod(shape))
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    field = device.DeviceArray(ctx, shape, np.float64)
    out = {'shape': list(shape), 'hbm_gbs': a.hbm_gbs, 'cases': {}}

    def share(bytes_per_voxel, ms):
        return bytes_per_voxel * nvox / (ms['median'] * 1e-3) / (a.hbm_gbs * 1e9)

    for case in a.cases.split(','):
        atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
        ctx.vacuum_assign(None, vv)
        n = limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
        res = {'n_maxima': int(n)}
        maxima = np.dot(ctx.maxima() / np.array(shape, dtype=np.float64), lat)   # per atom, as Bader.bader_to_atom_distance does
        owner, _ = _lib.atom_assign(maxima, synth.atoms_cartesian(atoms, lat), lat)
        ctx.volume_assign(owner)
        n = atoms.shape[0]
        res['n_labels'] = int(n)
        res['field_gather_ms'] = timed(ctx, lambda: ctx.laplacian_field(lat, gather=True, out=field), a.warmup, a.repeats, a.limit, 'field, gather')
        gathered = field.to_host()
        res['field_ms'] = timed(ctx, lambda: ctx.laplacian_field(lat, out=field), a.warmup, a.repeats, a.limit, 'field, tiles')
        res['routes_agree'] = bool(np.array_equal(field.to_host().view(np.uint64), gathered.view(np.uint64)))
        del gathered
        res['sum_gather_ms'] = timed(ctx, lambda: ctx.laplacian_sum(lat, n, vv, gather=True), a.warmup, a.repeats, a.limit, 'sums, gather')
        res['sum_ms'] = timed(ctx, lambda: ctx.laplacian_sum(lat, n, vv), a.warmup, a.repeats, a.limit, 'sums, tiles')
        L, L_abs, _ = ctx.laplacian_sum(lat, n, vv)
        res['worst_L_over_L_abs'] = float(np.max(np.abs(L) / L_abs))
        res['critical_ms'] = timed(ctx, lambda: ctx.critical_points(), a.warmup, a.repeats, a.limit, 'critical points')
        lin = ctx.critical_points()[1]
        res['list'] = int(lin.size)
        res['points_ms'] = timed(ctx, lambda: ctx.stencil_points(lat, lin), a.warmup, a.repeats, a.limit, 'points')
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        ctx.critical_release()
        for key, per_voxel in (('field_ms', 16.0), ('field_gather_ms', 16.0), ('sum_ms', 12.0), ('sum_gather_ms', 12.0)):
            res[key.replace('_ms', '_roofline_share')] = share(per_voxel, res[key])
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
