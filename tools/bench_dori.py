#!/usr/bin/env python3
"""What DORI costs on one GPU (csrc/k_dori.h, host_dori.h), next to the NCI index and the Laplacian of the same build on the same
grid:

    python tools/bench_dori.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216,noisy]

Three densities at size^3 in the cubic cell of bench.py, generated on the device:

    8       the 8-atom cell of bench.py
    216     the 216-atom cell of bench.py's user leg
    noisy   the 8-atom cell with uniform noise in its vacuum (rho < 0.2), summed over its Bader volumes (global-memory bins)

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    gamma_ms, gamma_gather_ms            xb_dori_field, gamma alone into a device array, through the tiles and XB_STENCIL_GATHER
    field_ms, field_gather_ms            xb_dori_field, gamma and x into two device arrays, both routes
    sum_ms, sum_gather_ms                xb_dori_sum on the label map, both routes (8 atoms: LDS bins; 216, noisy: global memory)
    nci_field_ms, nci_sum_ms             xb_nci_field into two device arrays and xb_nci_sum on the same map
    laplacian_field_ms                   xb_laplacian_field into a device array
and whether the two routes gave the same bits for the fields and the same counts, the voxels in the region per class, and the
shares of the rooflines: 16 B per voxel for gamma alone (8 read, 8 written), 24 B with x, 12 B for the sums, against --hbm-gbs.

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

from pybader_amd import _lib, device, dori, nci, synth                 # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402

VACUUM_TOL = 0.2


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_dori: {what} exceeded {seconds} s\n')
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
    ap.add_argument('--hbm-gbs', type=float, default=8000.0, help='the HBM bandwidth the roofline shares refer to (MI355X: 8 TB/s peak)')
    a = ap.parse_args()
    shape = (a.size,) * 3
    nvox = float(np.prod(shape))
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    cuts = (dori.D_CUT, dori.RHO_MIN, dori.RHO_SPLIT)
    nci_cuts = (nci.S_CUT, nci.RHO_CUT, nci.RHO_SPLIT)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    fields = [device.DeviceArray(ctx, shape, np.float64) for _ in range(2)]
    out = {'shape': list(shape), 'hbm_gbs': a.hbm_gbs, 'cuts': list(cuts), 'cases': {}}

    def share(bytes_per_voxel, ms):
        return bytes_per_voxel * nvox / (ms['median'] * 1e-3) / (a.hbm_gbs * 1e9)

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

        def both(key, fn, same):
            """fn(gather) timed through both routes; same(result): what two equal results share"""
            res[key + '_gather_ms'] = timed(ctx, lambda: fn(True), a.warmup, a.repeats, a.limit, key + ', gather')
            first = same(fn(True))
            res[key + '_ms'] = timed(ctx, lambda: fn(False), a.warmup, a.repeats, a.limit, key + ', tiles')
            res[key + '_routes_agree'] = bool(first == same(fn(False)))

        both('gamma', lambda g: ctx.dori_field(lat, cuts[1], gather=g, out=[fields[0], None]), lambda _: synth.sha256(fields[0].to_host()))
        both('field', lambda g: ctx.dori_field(lat, cuts[1], gather=g, out=fields), lambda _: tuple(synth.sha256(f.to_host()) for f in fields))
        both('sum', lambda g: ctx.dori_sum(lat, n, vv, *cuts, gather=g), lambda r: r[0].tobytes())
        count, charge, _ = ctx.dori_sum(lat, n, vv, *cuts)
        res['region_voxels_per_class'] = count.sum(axis=0).tolist()
        res['region_electrons_per_class'] = charge.sum(axis=0).tolist()
        res['nci_field_ms'] = timed(ctx, lambda: ctx.nci_field(lat, out=fields), a.warmup, a.repeats, a.limit, 'nci field')
        res['nci_sum_ms'] = timed(ctx, lambda: ctx.nci_sum(lat, n, vv, *nci_cuts), a.warmup, a.repeats, a.limit, 'nci sums')
        res['laplacian_field_ms'] = timed(ctx, lambda: ctx.laplacian_field(lat, out=fields[0]), a.warmup, a.repeats, a.limit, 'laplacian field')
        for key, per_voxel in (('gamma', 16.0), ('gamma_gather', 16.0), ('field', 24.0), ('field_gather', 24.0), ('sum', 12.0),
                               ('sum_gather', 12.0), ('nci_field', 24.0), ('nci_sum', 12.0), ('laplacian_field', 16.0)):
            res[key + '_roofline_share'] = share(per_voxel, res[key + '_ms'])
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
