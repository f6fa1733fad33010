#!/usr/bin/env python3
"""What the weight method costs on one GPU (csrc/k_weight.h, host_weight.h):

    python tools/bench_weight.py [--size 512] [--warmup 2] [--repeats 5] [--limit 120]

The synthetic 8-atom cubic cell of bench.py at size^3, generated on the device.  Timed with a host clock around calls that
end in a device wait (xb_weight_sum returns with its results on the host; so does xb_charge_sum), warm-up first, median / min /
max of the repeats:

    weight_sum_ms    xb_weight_sum with the resident density as the integrand
    charge_sum_ms    xb_charge_sum on the same grid after a neargrid assignment (for scale: one pass over the grid)
    levels, levels_batched, levels_tail, batches, maxima     what the level loop did (xb_weight_stats)

Every timed step runs under --limit seconds: a step that overruns ends the process with status 124 and no result line (a
watchdog thread; a hung device call cannot be interrupted from Python).  The watchdog is a backstop inside the process: run the
tool under a limit from outside as well, `timeout -k 10 600 python tools/bench_weight.py`.  Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import threading
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import _lib, synth                       # noqa: E402
from pybader_amd.weight import voronoi_weights            # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform   # noqa: E402


def limited(seconds, what, fn):
    """run fn() under a time limit of its own"""
    def overrun():
        sys.stderr.write(f'bench_weight: {what} exceeded {seconds} s\n')
        sys.stderr.flush()
        os._exit(124)
    t = threading.Timer(seconds, overrun)
    t.daemon = True
    t.start()
    try:
        return fn()
    finally:
        t.cancel()


def timed(ctx, fn, warmup, repeats, limit, what):
    out = []
    for k in range(warmup + repeats):
        ctx.sync()
        t0 = time.perf_counter()
        limited(limit, what, fn)
        ctx.sync()
        if k >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return {'median': statistics.median(out), 'min': min(out), 'max': max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--limit', type=float, default=120.0)
    a = ap.parse_args()
    shape = (a.size,) * 3
    lat = synth.CUBIC6
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    vv = abs(np.linalg.det(lat)) / np.prod(shape)
    alpha = voronoi_weights(vl)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    limited(a.limit, 'density', lambda: ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND))
    ctx.vacuum_assign(None, vv)
    res = {}
    w = timed(ctx, lambda: res.__setitem__('w', ctx.weight_sum(alpha, vv)), a.warmup, a.repeats, a.limit, 'weight_sum')
    st = ctx.weight_stats()
    n = limited(a.limit, 'assign', lambda: ctx.assign('neargrid'))
    c = timed(ctx, lambda: res.__setitem__('c', ctx.charge_sum(vv, n)), a.warmup, a.repeats, a.limit, 'charge_sum')
    idx, ch, vo = res['w']
    print(json.dumps({'shape': list(shape), 'weight_sum_ms': w, 'charge_sum_ms': c, 'levels': st['levels'],
                      'levels_batched': st['levels_batched'], 'levels_tail': st['levels_tail'], 'batches': st['batches'],
                      'peak_frontier': st['peak_frontier'], 'weight_buffer_bytes': st['bytes'], 'weight_maxima': int(idx.size),
                      'grid_maxima': int(n), 'weight_charge_total': float(np.sum(ch)), 'grid_charge_total': float(np.sum(res['c'][0])),
                      'weight_volume_total': float(np.sum(vo)), 'cell_volume': float(abs(np.linalg.det(lat)))}))
    ctx.close()


if __name__ == '__main__':
    main()
