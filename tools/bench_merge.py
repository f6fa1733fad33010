#!/usr/bin/env python3
"""What merging Bader volumes by persistence costs on one GPU (csrc/k_merge.h, host_merge.h), next to what the adjacency
route costs for the same information:

    python tools/bench_merge.py [--size 512] [--tol 4e-3] [--warmup 2] [--repeats 7] [--parent-warmup 1] [--parent-repeats 3]
                                [--limit 300] [--cases 8,216,noisy]

The label maps of tools/bench_adjacency.py at size^3, each from the neargrid assignment of a density generated on the device:

    8       the 8-atom cubic cell of bench.py, labels per atom
    216     the 216-atom cell of bench.py's user leg, labels per atom
    noisy   the 8-atom cell with uniform noise of 2e-3 in its vacuum, labels per Bader volume (n in the millions)

The maximum of a label is the Bader maximum of the highest density that carries it.  Per case, warm-up first, then median / min /
max of the repeats of
    merge_ms             Context.merge_basins (xb_merge_basins + xb_merge_fetch), host clock around the call
    merge_kernel_ms      the kernels of the same calls alone (XB_TIMER_MERGE of xb_kernel_time, HIP events); per_round_ms = this / rounds
    adjacency_kernel_ms  the kernels of xb_adjacency on the same labels (XB_TIMER_ADJACENCY), measured in the same run
    parent_route_ms      Context.adjacency + adjacency.persistence, host clock: what the library offered for the same
                         information before (the pair table, its download and host sort, the Python loop over the pairs)
and rounds, survivors, merge_bytes (the method's device buffer) and pair_table_bytes.

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


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_merge: {what} exceeded {seconds} s\n')
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


def timed(ctx, fn, warmup, repeats, limit, what, timer=None):
    wall, dev = [], []
    for k in range(warmup + repeats):
        if timer is not None:
            ctx.kernel_time_reset()
        ctx.sync()
        t0 = time.perf_counter()
        limited(limit, what, fn)
        ctx.sync()
        if k >= warmup:
            wall.append((time.perf_counter() - t0) * 1e3)
            if timer is not None:
                dev.append(ctx.kernel_time(timer)[0])
    return stats(wall), (stats(dev) if dev else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--tol', type=float, default=4e-3, help='twice the amplitude of the noisy case\'s noise')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--parent-warmup', type=int, default=1)
    ap.add_argument('--parent-repeats', type=int, default=3)
    ap.add_argument('--limit', type=float, default=300.0)
    ap.add_argument('--cases', default='8,216,noisy')
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    dirs, _ = adjacency.active_directions(vl)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    out = {'shape': list(shape), 'n_dirs': int(dirs.shape[0]), 'tol': a.tol, 'cases': {}}
    for case in a.cases.split(','):
        atoms = synth.atoms_jittered_grid(6) if case == '216' else synth.ATOMS8
        limited(a.limit, 'density', lambda: ctx.synth_density(lat, atoms, synth.BACKGROUND))
        rho = ctx.download_density()
        if case == 'noisy':
            rho += np.where(rho < 0.2, 2e-3 * np.random.default_rng(11).random(shape), 0.0)
            ctx.upload_density(rho)
        ctx.vacuum_assign(None, vv)
        n = limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
        res = {'n_maxima': int(n)}
        vox = np.asarray(ctx.maxima(), dtype=np.int64)
        max_idx = np.ravel_multi_index(tuple(vox.T), shape)
        peak = rho.reshape(-1)[max_idx]
        del rho
        if case != 'noisy':       # per atom: every maximum to its nearest atom, as Bader.bader_to_atom_distance does
            maxima = np.dot(vox / np.array(shape, dtype=np.float64), lat)
            owner, _ = _lib.atom_assign(maxima, synth.atoms_cartesian(atoms, lat), lat)
            ctx.volume_assign(owner)
            n = atoms.shape[0]
            top = np.zeros(n, np.int64)       # an atom's maximum: the highest of its Bader maxima
            for m in np.argsort(peak, kind='stable'):
                top[owner[m]] = max_idx[m]
            max_idx, peak = top, None
        res['n_labels'] = int(n)
        ctx.enable_timing(only=[_lib.XB_TIMER_MERGE])
        res['merge_ms'], res['merge_kernel_ms'] = timed(ctx, lambda: ctx.merge_basins(dirs, max_idx, a.tol), a.warmup, a.repeats,
                                                        a.limit, 'merge_basins', timer=_lib.XB_TIMER_MERGE)
        root, rnd, pers, rounds, left, converged = ctx.merge_basins(dirs, max_idx, a.tol)
        res.update(rounds=rounds, survivors=left, converged=converged,
                   per_round_ms=res['merge_kernel_ms']['median'] / rounds)
        held = ctx.memory_stats()[2]
        ctx.merge_release()
        res['merge_bytes'] = int(held - ctx.memory_stats()[2])
        ctx.enable_timing(only=[_lib.XB_TIMER_ADJACENCY])
        _, res['adjacency_kernel_ms'] = timed(ctx, lambda: ctx.adjacency(dirs, n), a.parent_warmup, a.parent_repeats, a.limit,
                                              'adjacency', timer=_lib.XB_TIMER_ADJACENCY)
        ctx.enable_timing(False)
        if peak is None:
            peak = ctx.download_density().reshape(-1)[max_idx]

        def parent_route():
            pairs, _, saddle, _ = ctx.adjacency(dirs, n)
            return pairs.shape[0], adjacency.persistence(pairs, saddle, peak)

        res['parent_route_ms'], _ = timed(ctx, parent_route, a.parent_warmup, a.parent_repeats, a.limit, 'adjacency + persistence')
        n_pairs, want = parent_route()
        res['n_pairs'] = int(n_pairs)
        # round 0 of the merge is that persistence wherever the peaks differ: the two routes agree on the survivors of round 0
        first = ctx.merge_basins(dirs, max_idx, a.tol, 1)
        res['round0_matches_persistence'] = bool(len(np.unique(peak)) < n or np.array_equal(first[2], want))
        held = ctx.memory_stats()[2]
        ctx.adjacency_release()
        res['pair_table_bytes'] = int(held - ctx.memory_stats()[2])
        ctx.merge_release()
        res['ratio_round_to_adjacency'] = res['per_round_ms'] / res['adjacency_kernel_ms']['median']
        out['cases'][case] = res
    print(json.dumps(out))
    ctx.close()


if __name__ == '__main__':
    main()
