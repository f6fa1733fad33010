"""Random soak of the one-GPU pipeline against the CPU oracle (test infrastructure; run by hand on a GPU box, and in a short
seeded form by tests/test_gpu_soak.py):

    python tests/soak_vs_oracle.py [cases] [seed] [--method neargrid|ongrid] [--odd | --oddbig | --big | --tiny | --thin]

Each case: a random grid shape (whole 8^3 bricks, or anything from 10 to 60 with --odd: the routes for grids that are not
made of bricks; every axis from 3 to 9 with --tiny: grids below one 8^3 brick, down to the axes of 3 and 4 voxels on which the
planes x-2 and x+1 or x+2 are one plane; one such axis beside two of 16 to 96 with --thin: a short axis on both sides of the
routes' `>= 16` and `nz < 80` tests), one of four lattices, optional noise / plateaus / vacuum tolerance, a random refinement mode.  The library's
assignment (map, maxima in basin order) must equal the oracle's -- the own-trajectory map of methods.neargrid's stepping
rule, or methods.ongrid's map -- and its refinement of that map the oracle's refinement, log and map.  Round 3: 1 800 cases
of this soak found the slow kernel applying the vacuum rule to labels nobody had written (fixed, regression test in
test_gpu_rough.py) and nothing else."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

HEX = np.array([[6.0, 0.0, 0.0], [-3.0, 5.196152422706632, 0.0], [0.0, 0.0, 7.0]])
ORTHO = np.array([[5.0, 0.0, 0.0], [0.0, 6.5, 0.0], [0.0, 0.0, 7.25]])


# Magnitude and sign cases (tests/test_gpu_soak.py runs them, tests/test_magnitude_cpu.py proves on the CPU that their inputs reach
# what they are for).  The shapes, one case each: the smallest grid of the fused route, cut bricks, whole bricks with trapping
# regions, whole edge-sweep tiles (nz >= 80).  name -> (method, seed, scale, offset, tols); lattice, noise, plateaus and refinement
# mode are drawn from the seed as always.
#   grad-40 / -44 / -48   max_grad * 2^k straddles the 1E-14 of the stay test: gradient steps and ongrid steps mix
#   subnormal[-tol]       2^-140: every brick potential is a subnormal float, without and with a vacuum tolerance
#   overflow              2^130: brick potentials beyond FLT_MAX
#   negative[-tol]        the density quantised to 2^-20, minus 4: values in about [-4, 4], a negative tolerance
# The seeds of the grad cases are seeds of 201.. for which, on all four grids, the share of voxels below 1E-14 lies in [0.05, 0.80]
# and at least 0.03 of the voxels have a gradient that is small but not zero (a drawn plateau quantum alone fills the share with
# exact zeros, which the plateau cases of the plain soak already take through the branch); test_magnitude_cpu.py asserts both
# and records the shares.  The seeds of the -tol cases: such that the tolerance cuts through every one of the four grids.
MAGNITUDE_SHAPES = [(16, 16, 16), (20, 24, 28), (32, 32, 32), (24, 32, 128)]
_TOLS = [0.02, 0.2, 0.02, 0.2]
MAGNITUDE_CASES = {
    'neargrid-grad-40': ('neargrid', 216, -40, None, None), 'neargrid-grad-44': ('neargrid', 204, -44, None, None),
    'neargrid-grad-48': ('neargrid', 201, -48, None, None), 'ongrid-grad-40': ('ongrid', 246, -40, None, None),
    'ongrid-grad-44': ('ongrid', 207, -44, None, None), 'ongrid-grad-48': ('ongrid', 202, -48, None, None),
    'neargrid-subnormal': ('neargrid', 222, -140, None, [None] * 4), 'neargrid-subnormal-tol': ('neargrid', 221, -140, None, _TOLS),
    'ongrid-subnormal': ('ongrid', 224, -140, None, [None] * 4), 'ongrid-subnormal-tol': ('ongrid', 233, -140, None, _TOLS),
    'neargrid-overflow': ('neargrid', 225, 130, None, None), 'ongrid-overflow': ('ongrid', 226, 130, None, None),
    'neargrid-negative': ('neargrid', 227, 0, 4.0, [None] * 4), 'neargrid-negative-tol': ('neargrid', 240, 0, 4.0, _TOLS),
    'ongrid-negative': ('ongrid', 229, 0, 4.0, [None] * 4), 'ongrid-negative-tol': ('ongrid', 223, 0, 4.0, _TOLS),
}


def run_magnitude(name, verbose=False):
    method, seed, scale, offset, tols = MAGNITUDE_CASES[name]
    return run(len(MAGNITUDE_SHAPES), seed, method, shapes=MAGNITUDE_SHAPES, scale=scale, offset=offset, tols=tols, verbose=verbose)


def directed_vacuum_case():
    """Fix 1's case: the 32^3 triclinic two-atom density of test_gpu_neighbour_bits.vacuum_brick_case times 2^-140, and a
    tolerance halfway between float32(m) * (1 + 1e-6) and m, m the maximum of a brick that float32 rounds down -- the smallest
    such maximum: that brick holds voxels above the tolerance, and its float image says it holds none.
    -> (rho, dist_mat, T_grad, tol, brick index (3), m)"""
    from test_gpu_neighbour_bits import vacuum_brick_case
    rho, dm, tg, _ = vacuum_brick_case()
    rho = np.ascontiguousarray(rho * 2.0 ** -140)
    bmax = rho.reshape(4, 8, 4, 8, 4, 8).max(axis=(1, 3, 5))
    with np.errstate(under='ignore'):
        f = bmax.astype(np.float32).astype(np.float64)
    low = np.where(f * (1 + 1e-6) < bmax, bmax, np.inf)
    brick = np.unravel_index(int(np.argmin(low)), low.shape)
    m = float(bmax[brick])
    return rho, dm, tg, 0.5 * (float(f[brick]) * (1 + 1e-6) + m), tuple(int(b) for b in brick), m


def draw_cases(cases, seed, odd=False, big=False, oddbig=False, tiny=False, thin=False, shapes=None, tols=None):
    """the drawn part of run()'s cases, one dict each (no GPU, no oracle: tests/test_magnitude_cpu.py draws the same cases)"""
    from pybader_amd import synth
    lattices = [('cubic', synth.CUBIC6), ('triclinic', synth.TRICLINIC), ('hexagonal', HEX), ('orthorhombic', ORTHO)]
    rng = np.random.default_rng(seed)
    for k in range(cases):
        shape = tuple(int(rng.choice([16, 24, 32, 40, 48, 64, 72, 96])) for _ in range(3))
        if big:       # (--big: a few seconds of oracle time per case)
            shape = tuple(int(rng.choice([64, 96, 128, 160, 192])) for _ in range(3))
        elif oddbig:  # (--oddbig: grids the brick lattice does not divide, large enough for trapping regions to form)
            shape = tuple(int(rng.integers(41, 150)) for _ in range(3))
        elif odd:
            shape = tuple(int(rng.integers(10, 61)) for _ in range(3))
        elif tiny:    # (--tiny: below one brick, axes of 3 and 4 voxels included)
            shape = tuple(int(rng.integers(3, 10)) for _ in range(3))
        elif thin:    # (--thin: one short axis, the other two on either side of the routes' axis-length tests)
            short = int(rng.integers(3))
            shape = tuple(int(rng.integers(3, 10)) if j == short else int(rng.choice([16, 24, 40, 80, 96])) for j in range(3))
        elif rng.random() < 0.3:
            shape = (shape[0], shape[1], int(rng.choice([64, 128])))     # whole tiles in z: the tile-wise dilation
        if shapes is not None:
            shape = tuple(int(v) for v in shapes[k])
        lname, lat = lattices[int(rng.integers(4))]
        noise = float(rng.choice([0.0, 0.0, 1e-6, 1e-3, 3e-2]))
        quant = float(rng.choice([0.0, 0.0, 0.0, 1.0 / 32]))
        tol = [None, None, 0.02, 0.2][int(rng.integers(4))]
        if tols is not None:
            tol = tols[k]
        mode, iters = [('changed', 2), ('all', 2), ('changed', -1), ('all', -1)][int(rng.integers(4))]
        yield {'k': k, 'shape': shape, 'lname': lname, 'lat': lat, 'noise': noise, 'quant': quant, 'tol': tol, 'mode': mode, 'iters': iters}


def finish_density(rho, case, scale=0, offset=None):
    """(density, vacuum tolerance) of a case from the synthetic atoms' density `rho`: the case's noise and plateaus, then
    `offset` (the density rounded to multiples of 2^-20, minus the dyadic constant: an exact subtraction, the tolerance shifted
    likewise) and `scale` (density and tolerance times 2^scale: exact)"""
    shape, tol = rho.shape, case['tol']
    if case['noise']:
        rho = rho + case['noise'] * np.random.default_rng(case['k']).random(shape)
    if case['quant']:
        rho = np.round(rho / case['quant']) * case['quant']
    if offset is not None:
        rho = np.round(rho * 2.0 ** 20) * 2.0 ** -20 - offset
        tol = None if tol is None else tol - offset
    if scale:
        rho = rho * 2.0 ** scale
        tol = None if tol is None else tol * 2.0 ** scale
    return np.ascontiguousarray(rho), tol


def oracle_expectation(rho, tol, method, mode, iters, dm, tg):
    """(maxima, assignment map, refinement log, refined map) of the oracle"""
    import oracle
    from rough_common import own_map, rank_labels
    shape = rho.shape
    vol0 = np.zeros(shape, np.int32)
    vol0, _, _ = oracle.vacuum_assign(rho, vol0, float('nan') if tol is None else tol, rho, 1.0)
    if method == 'neargrid':
        lab, maxima = rank_labels(own_map(rho, vol0, dm, tg, main_ties=True))
    else:
        bmax, lab = oracle.bader_calc('ongrid', rho, vol0.copy(), dm, tg, 1)
        maxima = np.ravel_multi_index(tuple(np.asarray(bmax).T), shape) if len(bmax) else np.zeros(0, np.int64)
        lab = lab.astype(np.int64)
    v = lab.astype(np.int32).copy()
    olog = []
    oracle.refine('neargrid', (mode, iters), rho, v, dm, tg, 1, log=olog)
    return maxima, lab, olog, v


def run(cases, seed, method='neargrid', odd=False, verbose=False, big=False, oddbig=False, tiny=False, thin=False, shapes=None,
        scale=0, offset=None, tols=None):
    """-> descriptions of the cases whose result differs from the oracle's.  `shapes`: a list of grid shapes that replace the
    drawn ones, case by case (everything else of a case is drawn as always); `tols`: vacuum tolerances (or None) that replace
    the drawn ones likewise.  `scale`, `offset`: see finish_density -- the magnitudes and signs the drawn densities never have"""
    from pybader_amd import _lib, synth
    from pybader_amd.interface import distance_matrix, gradient_transform
    bad = []
    for case in draw_cases(cases, seed, odd, big, oddbig, tiny, thin, shapes, tols):
        k, shape, lname, lat, mode, iters = (case[f] for f in ('k', 'shape', 'lname', 'lat', 'mode', 'iters'))
        noise, quant = case['noise'], case['quant']
        vl = np.divide(lat, shape)
        dm, tg = distance_matrix(vl), gradient_transform(vl)
        ctx = _lib.Context(0)
        ctx.set_grid(shape, dm, tg)
        ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)
        rho, tol = finish_density(ctx.download_density(), case, scale, offset)
        ctx.upload_density(rho)
        ctx.vacuum_assign(tol, 1.0)
        n = ctx.assign(method)
        got0 = ctx.download_labels(np.int64)
        gmax = np.ravel_multi_index(tuple(ctx.maxima().T), shape) if n else np.zeros(0, np.int64)
        log = ctx.refine(mode, iters)
        got = ctx.download_labels(np.int32)
        ctx.close()
        maxima, lab, olog, v = oracle_expectation(rho, tol, method, mode, iters, dm, tg)
        parts = {'basins': n == len(maxima), 'maxima': np.array_equal(gmax, maxima), 'assignment': np.array_equal(got0, lab),
                 'log': [list(x) for x in log] == [list(x) for x in olog], 'refined map': np.array_equal(got, v)}
        what = f'case {k} of seed {seed}: {method} {shape} {lname} noise {noise} quantum {quant} vacuum_tol {tol} refine {mode}:{iters}, {n} basins'
        if scale or offset is not None:
            what += f', scale 2^{scale} offset {offset}'
        if not all(parts.values()):
            bad.append(what + ' -- differs in ' + ', '.join(p for p, ok in parts.items() if not ok))
        if verbose:
            print(('OK  ' if all(parts.values()) else 'BAD ') + what, flush=True)
    return bad


if __name__ == '__main__':
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    method = sys.argv[sys.argv.index('--method') + 1] if '--method' in sys.argv else 'neargrid'
    if '--method' in sys.argv:
        args.remove(method)
    failures = run(int(args[0]) if args else 20, int(args[1]) if len(args) > 1 else 1, method, '--odd' in sys.argv, verbose=True, big='--big' in sys.argv,
                   oddbig='--oddbig' in sys.argv, tiny='--tiny' in sys.argv, thin='--thin' in sys.argv)
    print('\n'.join(failures))
    print('bad cases:', len(failures))
    sys.exit(1 if failures else 0)
