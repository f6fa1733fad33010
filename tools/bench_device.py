#!/usr/bin/env python3
"""What the device-array boundary costs on one GPU (pybader_amd/device.py, csrc/host_interop.h):

    python tools/bench_device.py [--size 512] [--repeats 20] [--e2e-repeats 5]

1. IMPORT RATE of xb_import_density for each of its paths -- contiguous float64 (a device-to-device copy), contiguous
   float32 (vectorised widening), permuted layouts through the LDS tile and through the plain strided gather (option
   2 bit 64), sliced layouts (gather) -- against a plain device-to-device copy of the same destination bytes
   (torch's contiguous copy_, a hipMemcpyAsync), timed in this process the same way: device events on the caller's
   stream around the call, warm-up first, median of the repeats.  The copy is the yardstick, not code under test.
2. END TO END from a device tensor to a device label tensor: bader_calc_refine on the tensor, against the route a
   caller without this boundary has: t.cpu().numpy(), bader_calc_refine on the host array, torch.from_numpy(...).cuda().

Prints one JSON line.  (A tool: it uses torch to make the tensors; the library never imports it.)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch          # before the library is loaded: both then share one HIP runtime

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pybader_amd import _lib, thread_handlers   # noqa: E402

DEV = 'cuda:0'


def event_ms(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def import_rates(ctx, n, repeats):
    shape = (n, n, n)
    N = n ** 3
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    rows = []
    src = torch.rand(shape, dtype=torch.float64, device=DEV)
    dst = torch.empty_like(src)
    copy_ms, lo, hi = event_ms(lambda: dst.copy_(src, non_blocking=True), 3, repeats)
    del dst
    rows.append({'path': 'yardstick: device-to-device copy of the destination bytes', 'ms': copy_ms, 'min_ms': lo, 'max_ms': hi,
                 'ratio_to_copy': 1.0, 'GB_per_s': 2 * 8 * N / copy_ms / 1e6})

    def run(name, t, read_bytes, gather_only=False):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, _lib.XB_CHECK_IO_GATHER if gather_only else 0)
        try:
            ms, lo, hi = event_ms(lambda: ctx.import_density(t), 3, repeats)
        finally:
            ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
        rows.append({'path': name, 'ms': ms, 'min_ms': lo, 'max_ms': hi, 'ratio_to_copy': ms / copy_ms,
                     'GB_per_s': (read_bytes + 8 * N) / ms / 1e6})

    run('float64 contiguous (copy)', src, 8 * N)
    for perm, what in (((2, 0, 1), 'stride 1 on y'), ((1, 2, 0), 'stride 1 on x'), ((2, 1, 0), 'axes reversed')):
        t = src.permute(*perm)            # (a cube: every permutation has the grid's shape)
        run(f'float64 permuted, {what}: LDS tile', t, 8 * N)
        run(f'float64 permuted, {what}: strided gather', t, 8 * N, gather_only=True)
    f32 = src.to(torch.float32)
    run('float32 contiguous (vectorised widening)', f32, 4 * N)
    t = f32.permute(2, 0, 1)
    run('float32 permuted, stride 1 on y: LDS tile', t, 4 * N)
    run('float32 permuted, stride 1 on y: strided gather', t, 4 * N, gather_only=True)
    del f32, t
    big = torch.rand((2 * n, n, n), dtype=torch.float64, device=DEV)
    run('float64 every second x-plane (gather, z stride 1)', big[::2], 8 * N)
    del big
    big = torch.rand((n, n, 2 * n), dtype=torch.float64, device=DEV)
    run('float64 every second z (gather, z stride 2)', big[:, :, ::2], 16 * N)
    del big
    run('float64 expanded along x (gather, x stride 0)', src[:1].expand(*shape), 8 * n * n)
    return rows


def end_to_end(n, repeats):
    thread_handlers.VERBOSE = False
    g = np.load(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests', 'golden', f'c{n}_cubic.npz'))
    shape = (n, n, n)
    ctx = _lib.default_context()
    ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
    ctx.synth_density(g['lattice'], g['atoms'], float(g['background']))          # bit-identical to synth.synth_density

    class View:
        __cuda_array_interface__ = {'shape': shape, 'typestr': '<f8', 'data': (int(ctx.lib.xb_density_ptr(ctx.h)), False),
                                    'version': 2, 'strides': None}

    t = torch.as_tensor(View(), device=DEV).clone()
    torch.cuda.synchronize()
    args = ('neargrid', 'neargrid', ('changed', 2))
    dm, tg = g['dist_mat'], g['T_grad']

    def new_route():
        bmax, lab = thread_handlers.bader_calc_refine(*args, t, None, dm, tg, 1)
        out = torch.as_tensor(lab, device=DEV)
        torch.cuda.synchronize()
        return bmax, out

    def old_route():
        host = t.cpu().numpy()
        bmax, lab = thread_handlers.bader_calc_refine(*args, host, np.zeros(shape, np.int32), dm, tg, 1)
        out = torch.from_numpy(lab).cuda()
        torch.cuda.synchronize()
        return bmax, out

    times = {}
    results = {}
    for name, fn in (('new', new_route), ('old', old_route)):
        results[name] = fn()                                     # warm-up (allocations, first launches)
    for k in range(repeats):                                     # alternating, so both see the same machine
        for name, fn in (('new', new_route), ('old', old_route)):
            t0 = time.perf_counter()
            results[name] = fn()
            times.setdefault(name, []).append(1e3 * (time.perf_counter() - t0))
    same = bool(np.array_equal(results['new'][0], results['old'][0]) and torch.equal(results['new'][1], results['old'][1])
                and results['new'][1].dtype == results['old'][1].dtype)
    return {'size': n, 'basins': int(results['new'][0].shape[0]), 'label_dtype': str(results['new'][1].dtype),
            'device_tensor_to_device_labels_ms': statistics.median(times['new']), 'new_all_ms': times['new'],
            'through_the_host_ms': statistics.median(times['old']), 'old_all_ms': times['old'], 'results_equal': same}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--e2e-repeats', type=int, default=5)
    ap.add_argument('--no-e2e', action='store_true')
    args = ap.parse_args()
    ctx = _lib.Context(0)
    rows = import_rates(ctx, args.size, args.repeats)
    ctx.close()
    for r in rows:
        print(f"  {r['path']:<62s} {r['ms']:8.3f} ms  x{r['ratio_to_copy']:5.2f} of the copy  {r['GB_per_s']:8.1f} GB/s", file=sys.stderr)
    out = {'tool': 'bench_device', 'size': args.size, 'import': rows}
    if not args.no_e2e:
        out['end_to_end'] = end_to_end(args.size, args.e2e_repeats)
        e = out['end_to_end']
        print(f"  end to end at {args.size}^3: {e['device_tensor_to_device_labels_ms']:.2f} ms on the device, "
              f"{e['through_the_host_ms']:.2f} ms through the host, results equal: {e['results_equal']}", file=sys.stderr)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
