#!/usr/bin/env python3
"""What an isosurface costs on one GPU (csrc/k_isosurface.h, host_isosurface.h), next to the critical points and the Laplacian of the
same build on the same grid:

    python tools/bench_isosurface.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216]

Two densities at size^3 in the cubic cell of bench.py, generated on the device:

    8       the 8-atom cell of bench.py
    216     the 216-atom cell of bench.py's user leg

Per case three levels -- `cores` (a tenth of the density's maximum: small surfaces around the nuclei), `envelope` (0.001) and
`median` (the median of the field: the largest surface of the three) --, and per level, warm-up first, then median / min / max of
the repeats, each a host clock around a call that ends with a wait for the device (the calls have no timer slot):
    ms, gather_ms              xb_isosurface with the atom map's per-label volumes, through the tiles and through XB_ISO_GATHER;
                               the mesh stays on the device (count, offsets, scan, allocation of the mesh, emit)
    plain_ms                   ... through the tiles without labels
and V, T, the bytes of the mesh written, area, volume, and whether the two routes gave the same counts.  Next to them
    critical_ms                xb_critical_points
    laplacian_field_ms         xb_laplacian_field into a device array

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

from pybader_amd import _lib, device, synth                             # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_isosurface: {what} exceeded {seconds} s\n')
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
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    field = device.DeviceArray(ctx, shape, np.float64)
    out = {'shape': list(shape), 'cases': {}}
    for case in a.cases.split(','):
        atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
        ctx.vacuum_assign(None, vv)
        limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
        maxima = np.dot(ctx.maxima() / np.array(shape, dtype=np.float64), lat)   # per atom, as Bader.bader_to_atom_distance does
        owner, _ = _lib.atom_assign(maxima, synth.atoms_cartesian(atoms, lat), lat)
        ctx.volume_assign(owner)
        n = atoms.shape[0]
        rho = ctx.download_density()
        res = {'n_labels': int(n), 'levels': {}}
        for name, level in (('cores', 0.1 * float(rho.max())), ('envelope', 0.001), ('median', float(np.median(rho)))):
            r = {'level': level}
            r['gather_ms'] = timed(ctx, lambda: ctx.isosurface(lat, level, n=n, gather=True, fetch=False), a.warmup, a.repeats, a.limit, name + ', gather')
            gathered = ctx.isosurface(lat, level, n=n, gather=True, fetch=False)
            r['ms'] = timed(ctx, lambda: ctx.isosurface(lat, level, n=n, fetch=False), a.warmup, a.repeats, a.limit, name + ', tiles')
            r['plain_ms'] = timed(ctx, lambda: ctx.isosurface(lat, level, fetch=False), a.warmup, a.repeats, a.limit, name + ', no labels')
            V, T = ctx.isosurface(lat, level, n=n, fetch=False)
            r['routes_agree'] = bool((V, T) == gathered)
            r['vertices'], r['triangles'], r['mesh_bytes'] = V, T, 24 * max(V, 1) + 34 * max(T, 1)
            if T <= 50_000_000:
                m = ctx.isosurface_fetch(V, T, False, n)
                r['area'], r['volume'], r['volume_by_label_sum'] = m[5], m[6], float(m[7].sum())
            ctx.isosurface_release()
            res['levels'][name] = r
        del rho
        res['critical_ms'] = timed(ctx, lambda: ctx.critical_points(), a.warmup, a.repeats, a.limit, 'critical points')
        ctx.critical_release()
        res['laplacian_field_ms'] = timed(ctx, lambda: ctx.laplacian_field(lat, out=field), a.warmup, a.repeats, a.limit, 'laplacian field')
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
