"""Size-independent properties at BASELINE.json's full sizes (no CPU oracle can follow there):
conservation, maxima consistency, idempotence of refinement, translation invariance of the
partition, and N-slab == 1-GPU."""
import hashlib
import os

import numpy as np
import pytest

import torch  # noqa: F401  (before the library: see conftest)
import oracle
from conftest import load_golden
from pybader_amd import _lib, synth
from pybader_amd.interface import distance_matrix, gradient_transform

REGIONS_ON = _lib.XB_REGIONS_BOXES | _lib.XB_REGIONS_BRICKS   # the default of XB_OPT_REGIONS; 0: plain full trajectories

pytestmark = pytest.mark.gpu


def matrices(shape, lattice):
    vl = np.divide(lattice, shape)
    return distance_matrix(vl), gradient_transform(vl)


def assert_map_hash(got, want_sha, what, ctx=None, method=None, refine=None, dist_mat=None, T_grad=None):
    """A map against the fixture's sha256.  A hash says nothing about WHERE two maps differ: on a mismatch the CPU oracle
    recomputes the map (minutes at these sizes -- only ever on a failing run) and the message names how many voxels differ,
    the first of them with both labels, and whether the oracle's own map still hashes to the fixture."""
    sha = hashlib.sha256(np.ascontiguousarray(got)).hexdigest()
    if sha == str(want_sha):
        return
    msg = f'{what}: sha256 {sha[:16]}... != fixture {str(want_sha)[:16]}...'
    if ctx is not None and method is not None:
        from rough_common import own_map, rank_labels
        rho = ctx.download_density()
        shape = rho.shape
        vol0 = np.zeros(shape, np.int32)
        if method == 'neargrid':
            lab, _ = rank_labels(own_map(rho, vol0, dist_mat, T_grad, main_ties=True))
        else:
            _, lab = oracle.bader_calc('ongrid', rho, vol0.copy(), dist_mat, T_grad, 1)
        lab = np.ascontiguousarray(lab.astype(np.int32))
        if refine is not None:
            oracle.refine('neargrid', refine, rho, lab, dist_mat, T_grad, 1)
        ora = lab.astype(got.dtype)
        diff = np.flatnonzero(ora.reshape(-1) != np.asarray(got).reshape(-1))
        first = [(tuple(int(c) for c in np.unravel_index(i, shape)), int(np.asarray(got).reshape(-1)[i]), int(ora.reshape(-1)[i])) for i in diff[:10]]
        msg += (f'; against the CPU oracle {diff.size} of {ora.size} voxels differ, first (voxel, library, oracle): {first}; '
                f'the oracle\'s own map {"hashes to" if hashlib.sha256(np.ascontiguousarray(ora)).hexdigest() == str(want_sha) else "does NOT hash to"} the fixture')
    raise AssertionError(msg)


def run(ctx, shape, lattice, rho=None, method='neargrid'):
    dm, tg = matrices(shape, lattice)
    ctx.set_grid(shape, dm, tg)
    if rho is None:
        ctx.synth_density(lattice, synth.ATOMS8, synth.BACKGROUND)
    else:
        ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign(method)
    return n, ctx.maxima(), ctx.download_labels(np.int32)


@pytest.mark.parametrize('size,method', [(512, 'neargrid'), (512, 'ongrid'), (384, 'neargrid')])
def test_full_size_invariants(size, method):
    ctx = _lib.Context(0)
    shape = (size,) * 3
    n, maxima, lab = run(ctx, shape, synth.CUBIC6, method=method)
    assert n == 8 and lab.min() == 0 and lab.max() == n - 1
    # every maximum carries its own label, and labels are numbered by first appearance in C order
    assert np.array_equal(lab[tuple(maxima.T)], np.arange(n))
    flat = lab.reshape(-1)
    first = np.array([np.argmax(flat == k) for k in range(n)])
    assert np.all(np.diff(first) > 0)
    # conservation: basin charges/volumes add up to the whole cell
    ch, vo = ctx.charge_sum(1.0, n)
    rho_sum = float(ctx.download_density().sum(dtype=np.float64))
    assert abs(ch.sum() - rho_sum) <= 1e-9 * rho_sum
    assert vo.sum() == float(size) ** 3
    hist = np.bincount(flat, minlength=n)
    assert np.array_equal(hist.astype(np.float64), vo)
    # refinement: the neargrid own-trajectory map is a fixed point; ongrid maps do change
    log = ctx.refine('changed', 2)
    after = ctx.download_labels(np.int32)
    if method == 'neargrid':
        assert all(c == 0 for _, c in log) and np.array_equal(after, lab)
    else:
        assert log[0][1] > 0
        # a second full refinement pass from the refined map must not re-flag unchanged interior
        assert int((after != lab).sum()) >= log[0][1]
    if size == 512:
        # the headline size against the REFERENCE itself (round 4): tests/golden/c512_cubic.npz holds what pybader's own
        # bader_calc / refine return on this very density (make_golden.py, hashes of the int8 maps, logs, maxima, charges)
        g = load_golden('c512_cubic')
        assert tuple(int(x) for x in g['shape']) == shape

        dm, tg = matrices(shape, synth.CUBIC6)
        if method == 'neargrid':
            assert np.array_equal(maxima, g['ng_bader_max'])
            assert_map_hash(lab.astype(np.int8), g['ng_F_sha256'], 'neargrid assignment at 512^3', ctx, 'neargrid', None, dm, tg)
            assert_map_hash(after.astype(np.int8), g['ng_changed_2_sha256'], "neargrid + refine ('changed', 2) at 512^3", ctx, 'neargrid', ('changed', 2), dm, tg)
            np.testing.assert_allclose(ch * float(g['voxel_volume']), g['ng_bader_charge'], rtol=1e-9)
            np.testing.assert_allclose(vo * float(g['voxel_volume']), g['ng_bader_volume'], rtol=1e-9)
        else:
            assert np.array_equal(maxima, g['og_bader_max'])
            assert_map_hash(lab.astype(np.int8), g['og_main_sha256'], 'ongrid assignment at 512^3', ctx, 'ongrid', None, dm, tg)
            assert np.array_equal(np.array(log, np.int64).reshape(-1, 2), g['og_ngrefine_changed_2_log'])
            assert_map_hash(after.astype(np.int8), g['og_ngrefine_changed_2_sha256'], "ongrid + refine ('changed', 2) at 512^3", ctx, 'ongrid', ('changed', 2), dm, tg)
    ctx.close()


@pytest.mark.parametrize('size', [256, 512])
def test_translation_invariance(size):
    """roll(rho) gives the rolled partition (holds for the reference's final map)."""
    ctx = _lib.Context(0)
    shape = (size,) * 3
    n1, max1, lab1 = run(ctx, shape, synth.CUBIC6)
    rho = ctx.download_density()
    shift = (5, 3, 7)
    n2, max2, lab2 = run(ctx, shape, synth.CUBIC6, rho=np.ascontiguousarray(np.roll(rho, shift, axis=(0, 1, 2))))
    del rho
    assert n1 == n2
    moved = (max1 + np.array(shift)) % size
    # basin k of the original is basin perm[k] of the rolled grid
    key2 = {tuple(m): k for k, m in enumerate(max2.tolist())}
    perm = np.array([key2[tuple(m)] for m in moved.tolist()], np.int32)
    assert np.array_equal(perm[np.roll(lab1, shift, axis=(0, 1, 2))], lab2)
    ctx.close()


def test_slabs_equal_one_gpu_256():
    from test_gpu_slabs import run_slabs
    ctx = _lib.Context(0)
    shape = (256,) * 3
    n, maxima, lab = run(ctx, shape, synth.CUBIC6)
    rho = ctx.download_density()
    ctx.close()
    dm, tg = matrices(shape, synth.CUBIC6)
    g = {'dist_mat': dm, 'T_grad': tg}
    pre, post, log, mx, ch, vo, fb = run_slabs(4, g, rho, 'neargrid', 'all', 2, 8, None)
    assert np.array_equal(pre, lab) and np.array_equal(post, lab)
    assert np.array_equal(np.array(np.unravel_index(mx, shape)).T, maxima)
    # with an 8-plane halo about 1 % of the retraces glide out of the valid planes along a dividing surface (they never
    # enter a trapping region: regions hold no edge voxel) and are finished through the owners' path queries -- the
    # maps above are equal all the same
    assert fb <= 2, fb


def test_768_eight_slabs_equal_one_gpu():
    """Eight logical slabs (the slab count of BASELINE config 4) on the largest grid whose eight full-size contexts fit one
    card: 768^3 (8 x 28 GB).  96 planes per rank, halo 16, table window +-48: the map, the maxima and the sums equal the
    one-context run's (int8 labels, hashed)."""
    import hashlib
    from test_gpu_slabs import run_slabs
    size = 768
    shape = (size,) * 3
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('neargrid')
    maxima = ctx.maxima()
    log = ctx.refine('changed', 2)
    ch, vo = ctx.charge_sum(1.0, n)
    sha = hashlib.sha256(ctx.download_labels(np.int8)).hexdigest()
    ctx.close()
    assert n == 8 and vo.sum() == float(size) ** 3
    g = {'dist_mat': dm, 'T_grad': tg}
    pre, post, slog, mx, ch2, vo2, fb = run_slabs(8, g, None, 'neargrid', 'changed', 2, 16, None, shape=shape,
                                                  synth_args=(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND),
                                                  label_dtype=np.int8, keep_pre=False, margin=48)
    assert all(run_slabs.last_windowed)
    assert hashlib.sha256(np.ascontiguousarray(post)).hexdigest() == sha
    assert np.array_equal(np.array(np.unravel_index(mx, shape)).T, maxima)
    assert np.array_equal(vo2, vo) and np.allclose(ch2, ch, rtol=1e-12)
    assert [tuple(x) for x in slog] == [tuple(x) for x in log]
    assert fb > 0      # with a 16-plane halo some retraces travel as walkers


@pytest.mark.parametrize('size,lattice', [(256, synth.CUBIC6), (192, synth.TRICLINIC), (512, synth.CUBIC6)])
def test_trapping_regions_do_not_change_the_map(size, lattice):
    """The trapping-region early exit (brick masks + growth) is exact by construction; check it anyway against the plain
    full-trajectory trace (XB_OPT_REGIONS = 0: records for every voxel, no regions) at sizes the CPU oracle cannot reach."""
    ctx = _lib.Context(0)
    shape = (size,) * 3
    ctx.set_option(_lib.XB_OPT_REGIONS, 0)             # plain tracing
    n0, max0, lab0 = run(ctx, shape, lattice)
    assert ctx.box_stats() == (0, 0)
    ctx.set_option(_lib.XB_OPT_REGIONS, REGIONS_ON)    # trapping regions (the default)
    n2, max2, lab2 = run(ctx, shape, lattice)
    nb, nv2 = ctx.box_stats()
    assert nb == n2 and nv2 > 0.4 * size ** 3
    assert n0 == n2 and np.array_equal(max0, max2) and np.array_equal(lab0, lab2)
    ctx.close()


def test_config4_1024_one_gpu_four_and_eight_slabs():
    """BASELINE config 4 (1024^3, EIGHT axis-0 slabs of 128 planes) on one GPU: the whole grid in one context (66.6 GB), then
    four and eight logical slabs on the same device -- since round 3 a rank's table and scratch are sized by its slab
    (30 GB per rank on eight slabs, 243 GB in all; round 2's full-size arrays stopped at four) -- properties of the map, and
    N-slab == 1-slab bit for bit (int8 labels, hashed)."""
    import hashlib
    from test_gpu_slabs import run_slabs
    size = 1024
    shape = (size,) * 3
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('neargrid')
    maxima = ctx.maxima()
    log = ctx.refine('changed', 2)
    assert n == 8 and all(c == 0 for _, c in log) and log[0][0] > 0
    ch, vo = ctx.charge_sum(1.0, n)
    assert vo.sum() == float(size) ** 3 and np.all(vo > 0)
    lab = ctx.download_labels(np.int8)
    assert np.array_equal(lab[tuple(maxima.T)], np.arange(n))          # every maximum carries its own label
    assert np.array_equal(np.bincount(lab.reshape(-1), minlength=n).astype(np.float64), vo)
    first = np.array([int(np.argmax(lab.reshape(-1) == k)) for k in range(n)])
    assert np.all(np.diff(first) > 0)                                   # numbered by first appearance in C order
    sha = hashlib.sha256(lab).hexdigest()
    del lab
    ctx.close()
    g = {'dist_mat': dm, 'T_grad': tg}
    for n_slabs, margin in ((4, 64), (8, 64)):
        pre, post, slog, mx, ch2, vo2, fb = run_slabs(n_slabs, g, None, 'neargrid', 'changed', 2, 16, None, shape=shape,
                                                      synth_args=(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND),
                                                      label_dtype=np.int8, keep_pre=False, margin=margin)
        assert hashlib.sha256(np.ascontiguousarray(post)).hexdigest() == sha, n_slabs
        del pre, post
        assert np.array_equal(np.array(np.unravel_index(mx, shape)).T, maxima)
        assert np.array_equal(vo2, vo) and np.allclose(ch2, ch, rtol=1e-12)
        assert [tuple(x) for x in slog] == [tuple(x) for x in log]
        per_rank = max(m[0] for m in run_slabs.last_memory)
        print(f'{n_slabs} slabs of 1024^3: {per_rank / 2**30:.1f} GiB per rank')
        assert per_rank < (36 << 30 if n_slabs == 8 else 48 << 30)


def test_config4_1024_against_the_reference():
    """BASELINE config 4's grid against what pybader itself returns on it (tests/golden/c1024_cubic.npz: 1.6 h of the
    reference's numba path, hashes + logs + maxima + charges).  ongrid + refinement: bit for bit.  neargrid: the reference's
    default two iterations do NOT converge at this size -- its log ends with 33 relabelled voxels; iterated on it needs four:
    [377, 4], [72, 0] -- so its ('changed', 2) map is not yet the own-trajectory map this library returns.  Pinned EXACTLY
    (round 5): the fixture names the 4 voxels (of 2^30) on which the reference's default map differs from its own
    converged ('changed', -1) map, with its labels in both; this library's map is the converged one bit for bit (hash), and with
    exactly those 4 voxels set to the reference's default labels it hashes to the reference's default map."""
    g = load_golden('c1024_cubic')
    shape = tuple(int(x) for x in g['shape'])
    ctx = _lib.Context(0)
    ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
    ctx.synth_density(g['lattice'], g['atoms'], float(g['background']))
    vv = float(g['voxel_volume'])

    def sha(a):
        return hashlib.sha256(np.ascontiguousarray(a)).hexdigest()
    ctx.vacuum_assign(None, vv)
    n = ctx.assign('neargrid')
    assert np.array_equal(ctx.maxima(), g['ng_bader_max'])
    log = ctx.refine('changed', 2)
    assert all(c == 0 for _, c in log)
    ch, vo = ctx.charge_sum(vv, n)
    lab = ctx.download_labels(np.int8)
    assert_map_hash(lab, g['ng_changed_inf_sha256'], 'neargrid + refinement at 1024^3 (the reference\'s converged map)', ctx, 'neargrid',
                    ('changed', 2), g['dist_mat'], g['T_grad'])
    idx, ref_default, ref_conv = g['ng_changed_2_vs_inf_idx'], g['ng_changed_2_vs_inf_default_labels'], g['ng_changed_2_vs_inf_converged_labels']
    assert idx.size == 4 and int(g['ng_changed_inf_log'][2, 1]) == 4      # the reference's own log: 4 voxels were still to move
    flat = lab.reshape(-1)
    assert np.array_equal(flat[idx], ref_conv)
    flat[idx] = ref_default.astype(np.int8)
    assert sha(lab) == str(g['ng_changed_2_sha256'])                        # == the reference's default-mode map, those 4 voxels apart
    # per-basin volumes differ by exactly those voxels, the charges far inside north_star's 1e-6
    want = g['ng_bader_volume'] / vv
    moved = np.zeros(n)
    np.add.at(moved, ref_default, 1.0)
    np.add.at(moved, ref_conv, -1.0)
    np.testing.assert_allclose(vo / vv + moved, want, rtol=0, atol=0.5)
    np.testing.assert_allclose(ch, g['ng_bader_charge'], rtol=1e-6)
    del lab, flat
    ctx.vacuum_assign(None, vv)
    ctx.assign('ongrid')
    assert np.array_equal(ctx.maxima(), g['og_bader_max'])
    assert_map_hash(ctx.download_labels(np.int8), g['og_main_sha256'], 'ongrid assignment at 1024^3', ctx, 'ongrid', None, g['dist_mat'], g['T_grad'])
    log = ctx.refine('changed', 2)
    assert np.array_equal(np.array(log, np.int64).reshape(-1, 2), g['og_ngrefine_changed_2_log'])
    assert_map_hash(ctx.download_labels(np.int8), g['og_ngrefine_changed_2_sha256'], "ongrid + refine ('changed', 2) at 1024^3", ctx, 'ongrid',
                    ('changed', 2), g['dist_mat'], g['T_grad'])
    ctx.close()


def test_many_atoms_keep_their_trapping_regions():
    """A cell with 216 atoms (more than the 64 seed cubes round 1 allowed): the trapping regions are built and the map
    equals the plain full-trajectory trace; one more case with more maxima than seed cubes can be (plain tracing)."""
    rng = np.random.default_rng(5)
    k = 6
    cells = np.stack(np.meshgrid(*(np.arange(k),) * 3, indexing='ij'), -1).reshape(-1, 3)
    frac = (cells + 0.5 + 0.18 * (rng.random(cells.shape) - 0.5)) / k
    atoms = np.concatenate([frac, 0.09 + 0.04 * rng.random((len(frac), 1)), 2.0 + 6.0 * rng.random((len(frac), 1))], 1)
    shape = (256,) * 3
    lattice = synth.CUBIC6
    dm, tg = matrices(shape, lattice)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(lattice, atoms, synth.BACKGROUND)
    out = []
    for opt in (0, REGIONS_ON):               # plain tracing / cubes + brick growth
        ctx.set_option(_lib.XB_OPT_REGIONS, opt)
        ctx.vacuum_assign(None, 1.0)
        n = ctx.assign('neargrid')
        out.append((n, ctx.maxima(), ctx.download_labels(np.int32), ctx.box_stats()))
    (n0, m0, l0, s0), (n1, m1, l1, s1) = out
    assert n0 == n1 and n0 >= len(atoms) and np.array_equal(m0, m1) and np.array_equal(l0, l1)
    assert s0 == (0, 0) and s1[0] > 64 and s1[1] > 0.3 * 256 ** 3, s1   # basins of ~5 bricks: about half the voxels
    log = ctx.refine('changed', 2)
    assert all(c == 0 for _, c in log) and np.array_equal(ctx.download_labels(np.int32), l1)
    ctx.close()


@pytest.mark.parametrize('method', ['neargrid', 'ongrid'])
def test_vacuum_at_scale_sparse_table_equals_full_table(method):
    """256^3 with half of the cell declared vacuum: the pipeline (brick masks, records for the walk-list / mixed bricks
    only, deferred from-rho retraces -- no region stop with vacuum) against plain full-trajectory tracing over a record for
    every voxel (XB_OPT_REGIONS = 0); maps, maxima and refinement logs must agree."""
    shape = (256,) * 3
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    res = []
    for boxes in (REGIONS_ON, 0):
        ctx.set_option(_lib.XB_OPT_REGIONS, boxes)
        ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
        vc, vv = ctx.vacuum_assign(0.03, 1.0)
        n = ctx.assign(method)
        pre = ctx.download_labels(np.int32)
        log = ctx.refine('changed', 2)
        res.append((n, ctx.maxima(), pre, log, ctx.download_labels(np.int32), vv))
    deferred = ctx.deferred_stats()
    ctx.close()
    assert 0.2 * 256 ** 3 < res[0][5] < 0.7 * 256 ** 3          # about half of the voxels are vacuum
    for r in res[1:]:
        assert r[0] == res[0][0] and np.array_equal(r[1], res[0][1])
        assert np.array_equal(r[2], res[0][2])
        assert r[3] == res[0][3] and np.array_equal(r[4], res[0][4])
    assert (res[0][2] == -1).sum() == res[0][5]
    if method == 'ongrid':
        assert res[0][3][0][1] > 0                                # the refinement relabels voxels
    print('deferred retraces', deferred)


def test_noisy_vacuum_keeps_the_atoms_regions():
    """What a real CHGCAR looks like: smooth atoms, noise in the low-density region -- thousands of spurious maxima.  Round 1
    dropped every trapping region beyond 64 maxima; with the growth seeded by the bricks that hold exactly one maximum the
    atoms keep theirs (no cap but the table), and the map still equals plain full-trajectory tracing."""
    shape = (256,) * 3
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    rho = ctx.download_density()
    rng = np.random.default_rng(11)
    low = rho < 0.2
    rho = np.ascontiguousarray(rho + np.where(low, 2e-3 * rng.random(shape), 0.0))
    ctx.upload_density(rho)
    out = []
    for opt in (0, REGIONS_ON):
        ctx.set_option(_lib.XB_OPT_REGIONS, opt)
        ctx.vacuum_assign(None, 1.0)
        n = ctx.assign('neargrid')
        out.append((n, ctx.maxima(), ctx.download_labels(np.int32), ctx.box_stats()))
    (n0, m0, l0, s0), (n1, m1, l1, s1) = out
    assert n0 == n1 and n0 > 2000, n0                       # thousands of maxima, most of them noise
    assert np.array_equal(m0, m1) and np.array_equal(l0, l1)
    assert s1[0] > 1023 and s1[1] > 0.25 * 256 ** 3, s1     # regions survive (round 1: none beyond 64 maxima)
    ctx.close()


HEXAGONAL = np.array([[5.2, 0.0, 0.0], [-2.6, 4.503332099679081, 0.0], [0.0, 0.0, 6.4]])   # only the third axis is a mirror axis
ORTHO = np.array([[5.0, 0.0, 0.0], [0.0, 6.5, 0.0], [0.0, 0.0, 7.25]])


@pytest.mark.parametrize('shape,lattice,noise', [((256, 256, 256), synth.CUBIC6, 0.0), ((128, 160, 192), ORTHO, 0.0),
                                                 ((160, 160, 128), HEXAGONAL, 0.0), ((128, 128, 128), synth.TRICLINIC, 0.0),
                                                 ((128, 128, 128), synth.CUBIC6, 1e-3)])
def test_mirror_prefilter_and_lean_walker_do_not_change_the_map(shape, lattice, noise):
    """Round 3's two instruction diets are exact by construction -- pass A's mirror prefilter (k_masks.h, bm_mirror) only
    closes faces the exact ongrid test would close too, the lean walker (k_trace.h, ng_walk_lean) follows the same
    trajectory -- but check them anyway: each switched off against both on, on lattices with three, one and no mirror
    axis, smooth and with noise (thousands of maxima: ongrid steps, plateaus), map + maxima + refinement log."""
    ctx = _lib.Context(0)
    dm, tg = matrices(shape, lattice)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(lattice, synth.ATOMS8, synth.BACKGROUND)
    if noise:
        rho = ctx.download_density()
        rho = np.ascontiguousarray(rho + noise * np.random.default_rng(3).random(shape))
        ctx.upload_density(rho)
    res = []
    for mirror, lean, diag in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 0)):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, (0 if mirror else _lib.XB_CHECK_NO_MIRROR) | (0 if lean else _lib.XB_CHECK_GENERIC_WALKER) |
                       (0 if diag else _lib.XB_CHECK_FULL_TGRAD))
        ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
        ctx.vacuum_assign(None, 1.0)
        n = ctx.assign('neargrid')
        pre = ctx.download_labels(np.int32)
        log = ctx.refine('changed', 2)
        res.append((n, ctx.maxima(), pre, log, ctx.download_labels(np.int32), ctx.box_stats()))
    ctx.close()
    for r in res[1:]:
        assert r[0] == res[0][0] and np.array_equal(r[1], res[0][1]) and np.array_equal(r[2], res[0][2])
        assert r[3] == res[0][3] and np.array_equal(r[4], res[0][4])
    # the prefilter decides a subset of the faces the exact test leaves closed: never fewer certified bricks with it
    assert res[0][5][1] >= res[1][5][1] and res[2][5][1] >= res[3][5][1]
    assert res[0][5] == res[2][5] and res[1][5] == res[3][5]          # the walker does not touch the regions
    assert res[0][5] == res[4][5]                                     # nor does the diagonal form of T_grad . grad
    print('certified voxels with / without the mirror prefilter:', res[0][5][1], res[1][5][1])


@pytest.mark.parametrize('shape,lattice,noise,tol', [((256, 256, 256), synth.CUBIC6, 0.0, None), ((128, 160, 200), ORTHO, 0.0, None),
                                                     ((128, 128, 128), synth.TRICLINIC, 0.0, 0.02), ((96, 96, 96), synth.CUBIC6, 3e-2, None),
                                                     ((64, 64, 64), synth.CUBIC6, 0.0, 0.05)])
def test_tile_wise_dilation_leaves_the_same_flags(shape, lattice, noise, tol):
    """k_edge_dilate_tiles (the dilation of refinement.py:385-404 from LDS tiles of the flags; XB_CHECK_LIST_DILATE selects the other) against
    k_edge_dilate_list (27 byte gathers per edge voxel): the same `known` array after the first refinement iteration, the
    same log and map after three -- smooth, rough, with vacuum (uniform vacuum tiles are on the list too), a z extent that
    is not a whole number of tiles."""
    ctx = _lib.Context(0)
    dm, tg = matrices(shape, lattice)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(lattice, synth.ATOMS8, synth.BACKGROUND)
    if noise:
        rho = ctx.download_density()
        rho = np.ascontiguousarray(rho + noise * np.random.default_rng(7).random(shape))
        ctx.upload_density(rho)
    res = []
    for tiled in (1, 0):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0 if tiled else _lib.XB_CHECK_LIST_DILATE)   # the dilation from the edge list
        ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
        ctx.vacuum_assign(tol, 1.0)
        n = ctx.assign('neargrid')
        log1 = ctx.refine('all', 1)
        known1 = ctx.download_known()
        log = ctx.refine('all', 2)
        res.append((n, log1, known1, log, ctx.download_labels(np.int32)))
    ctx.close()
    a, b = res
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[4], b[4])
    print('first iteration:', a[1], 'near-edge voxels', int((a[2] == -1).sum()))


def test_growth_that_outlasts_its_schedule_is_repeated_with_the_long_one():
    """After the chase the kill iteration is given 6 launches; a cascade that runs deeper is noticed on the device, everything
    downstream is skipped and the assignment is repeated with the worst-case schedule (which the context then keeps).
    Forced here with a schedule of ONE launch: same map, same maxima, one repeat."""
    shape = (192, 192, 192)
    ctx = _lib.Context(0)
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    n0 = ctx.assign('neargrid')
    want, boxes = ctx.download_labels(np.int32), ctx.box_stats()
    assert ctx.growth_stats() == (0, 6)
    ctx.set_option(_lib.XB_OPT_KILL_LAUNCHES, 1)
    ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
    ctx.vacuum_assign(None, 1.0)
    n1 = ctx.assign('neargrid')
    assert ctx.growth_stats()[0] == 1 and ctx.growth_stats()[1] > 6
    assert n1 == n0 and np.array_equal(ctx.download_labels(np.int32), want) and ctx.box_stats() == boxes
    log = ctx.refine('changed', 2)
    assert log[0][0] > 0
    ctx.close()


def test_brick_uniformity_left_by_the_walkers_equals_the_label_scan():
    """The group trace leaves, per walk-list brick, the one maximum all its 512 voxels ended on (LDS min / max of the
    walkers' results), which replaces k_label_uniform_list's pass over the labels for the edge sweep.  Checked where it
    shows: the edge sweep's flags -- `known` after the first refinement iteration must equal the flags of a run whose
    uniformity came from the label scan (the generic walker, XB_CHECK_GENERIC_WALKER, keeps the scan)."""
    shape = (192, 192, 192)
    ctx = _lib.Context(0)
    dm, tg = matrices(shape, synth.TRICLINIC)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.TRICLINIC, synth.ATOMS8, synth.BACKGROUND)
    res = []
    for lean in (1, 0):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0 if lean else _lib.XB_CHECK_GENERIC_WALKER)
        ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
        ctx.vacuum_assign(None, 1.0)
        n = ctx.assign('neargrid')
        log = ctx.refine('all', 1)
        res.append((n, log, ctx.download_known(), ctx.download_labels(np.int32)))
    ctx.close()
    assert res[0][0] == res[1][0] and res[0][1] == res[1][1]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_host_waits_of_one_gpu_steps():
    """Round 4: the one-GPU pipeline waits for the card once per assignment (neargrid and ongrid), once per fused refinement
    iteration, twice per edge_check (did the chase's LDS queues spill? + the results) and once per retrace pass after it."""
    shape = (128,) * 3
    dm, tg = matrices(shape, synth.CUBIC6)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    ctx.assign('neargrid')                    # (first call: allocations)
    for method, want_assign in (('neargrid', 1), ('ongrid', 1)):
        ctx.set_option(_lib.XB_OPT_DROP_TABLE, 1)
        ctx.vacuum_assign(None, 1.0)
        w0 = ctx.host_waits()
        ctx.assign(method)
        w1 = ctx.host_waits()
        log = ctx.refine('changed', 2)
        w2 = ctx.host_waits()
        assert w1 - w0 == want_assign, (method, w1 - w0)
        if log and log[0][1] and len(log) == 2:          # an iteration through edge_check + retraces
            assert w2 - w1 == 1 + 2 + 1, (method, w2 - w1, log)
        else:                                            # nothing changed: the second iteration is the identity
            assert w2 - w1 == 1, (method, w2 - w1, log)
    ctx.close()



def test_size_limits_fail_loudly():
    """the reference indexes with int64 (refinement.py:409-508, methods.py); this library's voxel indices
    are int32.  The limit is stated at the boundary (include/bader_hip.h) and must come back as an
    error, never as wrapped indices.  (Rounds 1-5 had a second limit, 2^30 voxels for 'changed' refinement: gone, see below.)"""
    ctx = _lib.Context(0)
    dm, tg = matrices((8, 8, 8), synth.CUBIC6)
    with pytest.raises(_lib.BaderHipError, match='int32 index range'):
        ctx.set_grid((2048, 1024, 1024), dm, tg)                      # 2^31 voxels: refused before anything is allocated
    ctx.close()


@pytest.mark.skipif(os.environ.get('XB_BIG_EDGE_CHECK') != '1', reason='1.08 G voxels against the CPU oracle: ~10 min of host time (XB_BIG_EDGE_CHECK=1)')
def test_edge_check_above_2_30_voxels_against_the_oracle():
    """Round 6: `edge_check`'s queue entries no longer keep their flag bits beside the voxel index, so 'changed' refinement runs up
    to the grid limit.  1032 x 1024 x 1024 (2^30 + 2^23 voxels), ongrid assignment + neargrid refinement ('changed', 2) -- the
    combination that relabels voxels and so goes through the dependency chase with voxel indices above 2^30 -- against the CPU
    oracle's map and log.  Run by hand (XB_BIG_EDGE_CHECK=1); the result of the round-6 run is recorded in DESIGN.md."""
    shape = (1032, 1024, 1024)
    lat = synth.CUBIC6 * (np.array(shape, np.float64) / 1024.0)[:, None]
    dm, tg = matrices(shape, lat)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, dm, tg)
    ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)
    rho = ctx.download_density()
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('ongrid')
    log = ctx.refine('changed', 2)
    got = ctx.download_labels(np.int8)
    mx = ctx.maxima()
    ctx.close()
    bmax, want = oracle.bader_calc('ongrid', rho, np.zeros(shape, np.int32), dm, tg, 1)
    wlog = []
    oracle.refine('neargrid', ('changed', 2), rho, want, dm, tg, 1, log=wlog)
    assert n == bmax.shape[0] and np.array_equal(mx, bmax)
    assert [tuple(r) for r in log] == [tuple(r) for r in wlog], (log, wlog)
    high = np.flatnonzero(got.reshape(-1)[1 << 30:] != want.reshape(-1)[1 << 30:].astype(np.int8))
    assert np.array_equal(got, want.astype(np.int8)), f'{int((got != want).sum())} voxels differ ({high.size} of them above index 2^30)'
    assert sum(ch for _, ch in log) > 0, 'the case must relabel voxels, or edge_check never runs'
