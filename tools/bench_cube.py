#!/usr/bin/env python3
"""Throughput of the cube density-block path on one GPU:

    python tools/bench_cube.py [--size 512] [--no-file] [--no-chgcar]

Builds a size^3 cube file in numpy (the reference writer's layout: records of nz values in lines of six,
' d.dddddE+ee' per value), and times
  * Context.parse_cube_text on the block (PCIe upload of the text + device parse, result resident in HBM),
  * io_cube.read on the file written to a temporary directory (header, memory map, upload, parse, download of the
    density; leave it out with --no-file),
  * the CHGCAR block of tools/bench_chgcar.py at the same size with Context.parse_density_text, for bytes/s side by
    side (--no-chgcar leaves it out).
EVERY value of the cube parse is checked against exact host arithmetic (mantissa / 10^k is one correctly rounded
operation, then the multiply by ang_to_bohr**3)."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_header(shape, voxel=0.2):
    lines = ['bench cube', 'density', '%5d %11.6f %11.6f %11.6f' % (1, 0.0, 0.0, 0.0)]
    for i, n in enumerate(shape):
        row = [0.0, 0.0, 0.0]
        row[i] = voxel
        lines.append('%5d %11.6f %11.6f %11.6f' % ((n,) + tuple(row)))
    lines.append('%5d %11.6f %11.6f %11.6f %11.6f' % (8, 8.0, 1.0, 1.0, 1.0))
    return ('\n'.join(lines) + '\n').encode()


def make_block(shape, seed=5, planes=16):
    """the density block as uint8 text, the mantissas (d.ddddd as an integer) and the decimal exponents"""
    nx, ny, nz = shape
    width = 12
    full, rem = nz // 6, nz % 6
    rec = full * (6 * width + 1) + (rem * width + 1 if rem else 0)
    text = np.empty(nx * ny * rec, dtype=np.uint8)
    mant = np.empty(nx * ny * nz, dtype=np.int64)
    expo = np.empty(nx * ny * nz, dtype=np.int64)
    rng = np.random.default_rng(seed)
    for x0 in range(0, nx, planes):
        x1 = min(nx, x0 + planes)
        r = (x1 - x0) * ny
        n = r * nz
        digits = rng.integers(0, 10, size=(n, 6), dtype=np.uint8)
        digits[:, 0] = np.maximum(digits[:, 0], 1)
        e = rng.integers(-3, 4, size=n, dtype=np.int64)
        tok = np.empty((n, width), dtype=np.uint8)
        tok[:, 0] = ord(' ')
        tok[:, 1] = digits[:, 0] + ord('0')
        tok[:, 2] = ord('.')
        tok[:, 3:8] = digits[:, 1:] + ord('0')
        tok[:, 8] = ord('E')
        tok[:, 9] = np.where(e < 0, ord('-'), ord('+'))
        tok[:, 10] = ord('0')
        tok[:, 11] = np.abs(e) + ord('0')
        tok = tok.reshape(r, nz * width)
        out = text[x0 * ny * rec:x1 * ny * rec].reshape(r, rec)
        lines = out[:, :full * (6 * width + 1)].reshape(r, full, 6 * width + 1)
        lines[:, :, :-1] = tok[:, :full * 6 * width].reshape(r, full, 6 * width)
        lines[:, :, -1] = ord('\n')
        if rem:
            out[:, full * (6 * width + 1):-1] = tok[:, full * 6 * width:]
            out[:, -1] = ord('\n')
        m = np.zeros(n, dtype=np.int64)
        for k in range(6):
            m = m * 10 + digits[:, k]
        mant[x0 * ny * nz:x1 * ny * nz] = m
        expo[x0 * ny * nz:x1 * ny * nz] = e - 5
    return text, mant, expo


def best_of(fn, repeats=3):
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        times.append(time.perf_counter() - t0)
    return min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--no-file', action='store_true')
    ap.add_argument('--no-chgcar', action='store_true')
    args = ap.parse_args()
    from pybader_amd import _lib, io_cube
    shape = (args.size,) * 3
    n = args.size ** 3
    text, mant, e10 = make_block(shape)
    scale = io_cube.ang_to_bohr ** 3
    ctx = _lib.Context(0)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    stats = {}

    def parse():
        stats['tokens'], stats['host'] = ctx.parse_cube_text(text, scale)
        ctx.sync()
    dt = best_of(parse)
    got = ctx.download_density()
    p = np.power(10.0, np.abs(e10).astype(np.float64))               # exact powers of ten
    val = np.where(e10 < 0, mant.astype(np.float64) / p, mant.astype(np.float64) * p) * scale
    ok = bool(np.array_equal(got.reshape(-1).view(np.int64), val.view(np.int64)))
    del got, val, p
    result = {
        'workload': f'{args.size}^3 cube density block, {text.size / 1e9:.2f} GB of text, host (pageable) -> resident rho',
        'all_values_bit_exact': ok, 'tokens': int(stats['tokens']), 'host_fallback_tokens': int(stats['host']),
        'gpu_seconds_incl_pcie_upload': dt, 'gpu_Mvalues_per_s': n / dt / 1e6, 'gpu_text_GB_per_s': text.size / dt / 1e9}
    if not args.no_file:
        d = tempfile.mkdtemp(prefix='bench_cube_')
        try:
            fn = os.path.join(d, 'bench.cube')
            with open(fn, 'wb') as f:
                f.write(make_header(shape))
                f.write(memoryview(text))
            out = {}

            def read():
                out['d'] = io_cube.read(fn, ctx=ctx)[0]
            dt_read = best_of(read)
            result['io_cube_read_seconds'] = dt_read
            result['io_cube_read_same_values'] = bool(np.array_equal(out['d']['charge'], ctx.download_density()))
        finally:
            shutil.rmtree(d, ignore_errors=True)
    del text
    if not args.no_chgcar:
        from bench_chgcar import make_text
        ctext = make_text(n)[0]

        def parse_chgcar():
            ctx.parse_density_text(ctext, 216.0)
            ctx.sync()
        dc = best_of(parse_chgcar)
        result.update({'chgcar_text_GB': ctext.size / 1e9, 'chgcar_seconds_incl_pcie_upload': dc,
                       'chgcar_text_GB_per_s': ctext.size / dc / 1e9})
    print(json.dumps(result))
    ctx.close()


if __name__ == '__main__':
    main()
