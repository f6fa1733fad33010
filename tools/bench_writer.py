"""Density -> CHGCAR text on the device (io_vasp.write's block writer): device formatting time, device-to-host copy
time, file-write time and n_host at 256^3 and 512^3, against Python's own ' {:.11E}' on a 1 M-value sample of the same
array on this host.  One JSON line per size.

    python tools/bench_writer.py [--sizes 256 512] [--reps 3] [--dir /tmp]

Device times are the writer's own event pairs (xb_format_times): the kernels of every chunk (length pass, scan, write
pass; one host round trip per chunk for the chunk's byte count is inside), and the chunk copies into pinned memory.
The wall time covers the whole call, the file writes included; the file-write time is the time spent in f.write."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pybader_amd import _lib, synth  # noqa: E402
from pybader_amd.interface import distance_matrix, gradient_transform  # noqa: E402


def one(ctx, rho, vol, path, style):
    t_write = 0.0
    t0 = time.perf_counter()
    n_host = nbytes = 0
    with open(path, 'wb') as f:
        for chunk, n in ctx.format_density_text(rho, vol, style, 11, 'chgcar'):
            t1 = time.perf_counter()
            f.write(chunk)
            t_write += time.perf_counter() - t1
            n_host, nbytes = n, nbytes + len(chunk)
    wall = time.perf_counter() - t0
    fm, cm = ctx.format_times
    os.unlink(path)
    return {'wall_s': wall, 'format_ms': fm, 'copy_ms': cm, 'file_write_s': t_write, 'n_host': n_host, 'bytes': nbytes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[256, 512])
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--dir', default='/tmp')
    ap.add_argument('--style', default='E')
    a = ap.parse_args()
    ctx = _lib.Context(0)
    lat = synth.CUBIC6
    vol = float(np.dot(lat[0], np.cross(lat[1], lat[2])))
    for s in a.sizes:
        shape = (s, s, s)
        vl = lat / np.array(shape, dtype=np.float64)[:, None]
        ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
        ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)
        rho = ctx.download_density()
        path = os.path.join(a.dir, f'bench_writer_{os.getpid()}_{s}')
        one(ctx, rho, vol, path, a.style)                     # warm-up
        runs = [one(ctx, rho, vol, path, a.style) for _ in range(a.reps)]
        sample = (np.swapaxes(rho, 0, 2).ravel()[:1_000_000] * vol).tolist()
        t0 = time.perf_counter()
        ''.join([' {:.11E}'.format(v) for v in sample])
        py_us = (time.perf_counter() - t0) / len(sample) * 1e6
        best = min(runs, key=lambda r: r['wall_s'])
        print(json.dumps({'size': s, 'style': a.style, 'values': rho.size, **best,
                          'format_ms_all': [r['format_ms'] for r in runs], 'wall_s_all': [r['wall_s'] for r in runs],
                          'python_format_us_per_value': py_us,
                          'python_estimate_s': py_us * rho.size * 1e-6}), flush=True)
    ctx.close()


if __name__ == '__main__':
    main()
