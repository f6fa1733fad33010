#!/usr/bin/env python3
"""What the NCI index costs on one GPU (csrc/k_nci.h, host_nci.h), next to the Laplacian and the charge sums of the same build on
the same grid:

    python tools/bench_nci.py [--size 512] [--warmup 2] [--repeats 7] [--limit 120] [--cases 8,216]

Two densities at size^3 in the cubic cell of bench.py, generated on the device:

    8       the 8-atom cell of bench.py
    216     the 216-atom cell of bench.py's user leg

Per case, warm-up first, then median / min / max of the repeats, each a host clock around a call that ends with a wait for the
device (the calls have no timer slot):
    field_ms, field_gather_ms            xb_nci_field into two device arrays, through the tiles and through XB_STENCIL_GATHER
    sum_ms, sum_gather_ms                xb_nci_sum on the atom map, both routes (8 atoms: LDS bins; 216: global memory)
    hist_ms, hist_gather_ms              xb_nci_hist with 32 x 32 bins (counted in LDS), both routes
    hist_global_ms, hist_global_gather_ms    ... with 100 x 200 bins (counted in global memory)
    laplacian_field_ms, laplacian_sum_ms     xb_laplacian_field into a device array and xb_laplacian_sum on the same map
    charge_sum_ms                        xb_charge_sum on the same map
and whether the two routes gave the same bits for both fields, the same counts and the same histograms, the voxels in the region
per class, and the shares of the rooflines: 24 B per voxel for the fields (8 read, 16 written), 12 B per voxel for the sums, 8 B
per voxel for the histogram, against --hbm-gbs.

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

from pybader_amd import _lib, device, nci, synth                       # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_nci: {what} exceeded {seconds} s\n')
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
    cuts = (nci.S_CUT, nci.RHO_CUT, nci.RHO_SPLIT)
    small = (np.linspace(0.0, 2.0, 33), np.linspace(-0.05, 0.05, 33))          # 1024 bins: counted in LDS
    large = (np.linspace(0.0, 2.0, 101), np.linspace(-0.05, 0.05, 201))        # 20 000 bins: counted in global memory
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    fields = [device.DeviceArray(ctx, shape, np.float64) for _ in range(2)]
    out = {'shape': list(shape), 'hbm_gbs': a.hbm_gbs, 'cuts': list(cuts), 'cases': {}}

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

        def both(key, fn, same):
            """fn(gather) timed through both routes; same(a, b): whether two results are equal"""
            res[key + '_gather_ms'] = timed(ctx, lambda: fn(True), a.warmup, a.repeats, a.limit, key + ', gather')
            first = same(fn(True))
            res[key + '_ms'] = timed(ctx, lambda: fn(False), a.warmup, a.repeats, a.limit, key + ', tiles')
            res[key + '_routes_agree'] = bool(first == same(fn(False)))

        def field_bits(_):
            return tuple(synth.sha256(f.to_host()) for f in fields)
        both('field', lambda g: ctx.nci_field(lat, gather=g, out=fields), field_bits)
        both('sum', lambda g: ctx.nci_sum(lat, n, vv, *cuts, gather=g), lambda r: r[0].tobytes())
        both('hist', lambda g: ctx.nci_hist(lat, *small, gather=g), lambda r: r.tobytes())
        both('hist_global', lambda g: ctx.nci_hist(lat, *large, gather=g), lambda r: r.tobytes())
        count, _, _ = ctx.nci_sum(lat, n, vv, *cuts)
        res['region_voxels_per_class'] = count.sum(axis=0).tolist()
        res['histogram_voxels'] = int(ctx.nci_hist(lat, *small).sum())
        res['laplacian_field_ms'] = timed(ctx, lambda: ctx.laplacian_field(lat, out=fields[0]), a.warmup, a.repeats, a.limit, 'laplacian field')
        res['laplacian_sum_ms'] = timed(ctx, lambda: ctx.laplacian_sum(lat, n, vv), a.warmup, a.repeats, a.limit, 'laplacian sums')
        res['charge_sum_ms'] = timed(ctx, lambda: ctx.charge_sum(vv, n), a.warmup, a.repeats, a.limit, 'charge_sum')
        for key, per_voxel in (('field', 24.0), ('field_gather', 24.0), ('sum', 12.0), ('sum_gather', 12.0), ('hist', 8.0),
                               ('hist_gather', 8.0), ('hist_global', 8.0), ('hist_global_gather', 8.0), ('laplacian_field', 16.0),
                               ('laplacian_sum', 12.0), ('charge_sum', 12.0)):
            res[key + '_roofline_share'] = share(per_voxel, res[key + '_ms'])
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
