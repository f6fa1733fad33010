"""Bader(...) with every analysis flag set at once -- what the README promises and no other test runs.

The input is that of tests/test_gpu_critical.py::test_bader_with_the_flag: 24^3, two unequal atoms, the density rounded to
multiples of 2^-20 (below 16, so also exact in float32), which makes every charge sum exact in any order.  Each profile runs
Bader with weight_flag, multipole_flag, adjacency_flag, critical_flag, laplacian_flag, voronoi_flag and persistence_tol together and
asserts:

 1. every attribute a run with ONE of the flags (plus persistence_tol) sets is there and equal -- bit for bit, except the sums
    that are float atomics (moments, Laplacian sums), which each lie within their feature test's bound of the restatement;
 2. every new attribute equals its numpy restatement (the one its feature's test imports) evaluated on the run's own final
    bader_volumes, atoms_volumes and voronoi_volumes and on the RIGHT field: partitions, surfaces, critical points and the
    Laplacian read `reference`, integrands read `density` / `spin`.  With a reference that is not the charge density the
    restatement on the swapped fields is computed as well and must be reported as different;
 3. atoms_bond_density / atoms_bond_position are bond_surfaces()'s, the bond graph's own stay in atoms_bond_graph;
 4. (default and vacuum + spin) the Bader map before the merge is the oracle's, and the per-atom charges the oracle's sums;
 5. a second __call__ on the same object gives the same attributes.

Wall time on an MI355X, the whole suite in one process: MEASURED below."""
import functools

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:  # pragma: no cover
    torch = None

import oracle
from history_common import cache_facet_areas
from pybader_amd import adjacency, critical, device, laplacian, merge, multipole, synth, thread_handlers, weight
from pybader_amd.interface import Bader, distance_matrix, gradient_transform
from rough_common import own_map, rank_labels
from test_adjacency_cpu import reference_adjacency
from test_critical_cpu import reference_bonds, reference_points
from test_gpu_sums import swapped
from test_laplacian_cpu import grouped as lap_grouped
from test_laplacian_cpu import restated_laplacian, restated_points
from test_laplacian_cpu import sum_bound as lap_sum_bound
from test_merge_cpu import reference_merge
from test_multipole_cpu import bound as moment_bound
from test_multipole_cpu import grouped as moment_grouped
from test_multipole_cpu import reference_terms
from test_voronoi_cpu import reference_labels
from test_weight_cpu import restate

pytestmark = pytest.mark.gpu
MEASURED = ('0.16 s to 0.54 s per profile (default, with 3887 maxima before the merge, 0.54 s).  The slowest test of the '
            'features\' own files in the same run: test_gpu_adjacency.py::test_adjacency[shape1], 2.15 s.')

SHAPE, LAT = (24, 24, 24), synth.CUBIC6
ATOMS5 = np.array([[0.27, 0.31, 0.29, 0.45, 7.5], [0.71, 0.66, 0.73, 0.36, 3.25]])
ATOMS = synth.atoms_cartesian(ATOMS5, LAT)
N_ATOMS = 2
TOL = 2.0 ** -10
PERSISTENCE = 2.0 ** -8        # far below the two atoms' barrier, above the zero persistence of the maxima of the flat tails
FLAGS = ('weight_flag', 'multipole_flag', 'adjacency_flag', 'critical_flag', 'laplacian_flag', 'voronoi_flag')
ATOMICS = {'atoms_moments', 'atoms_dipole', 'atoms_quadrupole', 'atoms_spin_moments', 'bader_moments', 'atoms_laplacian',
           'atoms_laplacian_abs', 'bader_laplacian', 'bader_laplacian_abs'}      # float atomics in any order: bounded, not bit-equal
SKIP = {'_density', '_file_info', 'density', 'reference'} | set(FLAGS)


def q20(a):
    return np.ascontiguousarray(np.round(a * 2.0 ** 20) / 2.0 ** 20)


@functools.lru_cache(maxsize=None)
def field(name):
    """charge: the two atoms.  spin: the same sites, other widths, one amplitude negative.  core: a smooth term on each atom,
    wider than the valence charge (so that surfaces, saddles, critical points and the vacuum of the reference differ from the
    charge's: an all-electron reference adds such a term).  reference = charge + core, a distinct array."""
    if name == 'charge':
        a = q20(synth.synth_density(SHAPE, LAT, ATOMS5, 0.0))
    elif name == 'spin':
        a = q20(synth.synth_density(SHAPE, LAT, np.concatenate([ATOMS5[:, :3], [[0.5, 0.625], [0.4, -0.375]]], axis=1), 0.0))
    elif name == 'core':
        a = q20(synth.synth_density(SHAPE, LAT, np.concatenate([ATOMS5[:, :3], [[0.6, 4.0], [0.5, 2.5]]], axis=1), 0.0))
    else:
        a = q20(field('charge') + field('core'))
    a.flags.writeable = False
    return a


PROFILES = {
    'default': {},
    'vacuum and spin': {'vacuum_tol': TOL, 'spin_flag': True, 'spin': True},
    'reference': {'reference': True},
    'reference and vacuum': {'reference': True, 'vacuum_tol': TOL},
    'speed_flag, ongrid': {'speed_flag': True, 'method': 'ongrid', 'refine_mode': ('changed', 3)},
    'two calls': {'fused': False},
    'permuted float32 tensor': {'tensor': True},
}


def make(profile, **flags):
    kw = dict(PROFILES[profile])
    charge = field('charge').copy()
    if kw.pop('tensor', False):
        charge = torch.as_tensor(np.ascontiguousarray(charge.astype(np.float32).transpose(2, 0, 1)), device='cuda').permute(1, 2, 0)
        assert tuple(charge.shape) == SHAPE and not charge.is_contiguous()
    dens = {'charge': charge}
    if kw.pop('spin', False):
        dens['spin'] = field('spin').copy()
    if kw.pop('reference', False):
        kw['reference'] = field('reference').copy()
    return Bader(dens, LAT, ATOMS, persistence_tol=PERSISTENCE, **kw, **flags)


def fields_of(profile):
    """(reference, density, spin, vacuum_tol) as host float64 arrays"""
    p = PROFILES[profile]
    return (field('reference') if p.get('reference') else field('charge'), field('charge'),
            field('spin') if p.get('spin') else None, p.get('vacuum_tol'))


def host(a):
    if isinstance(a, device.DeviceArray):
        return a.to_host()
    if torch is not None and isinstance(a, torch.Tensor):
        return a.cpu().numpy()
    return a


_memo = {}


def memo(fn, *args):
    """fn(*args), computed once per content of the array arguments (the restatements are Python loops)"""
    key = (fn.__name__,) + tuple((a.shape, a.dtype.str, a.tobytes()) if isinstance(a, np.ndarray) else a for a in args)
    if key not in _memo:
        _memo[key] = fn(*args)
    return _memo[key]


def differs(got, want, key, strict=True):
    """-> None if equal (arrays: dtype -- with `strict` --, shape and every value, NaN == NaN; objects: every attribute), else
    what differs"""
    got, want = host(got), host(want)
    if isinstance(want, np.ndarray):
        if not isinstance(got, np.ndarray) or (strict and got.dtype != want.dtype) or got.shape != want.shape:
            return f'{key}: {getattr(got, "dtype", type(got))}{getattr(got, "shape", "")} for {want.dtype}{want.shape}'
        same = np.array_equal(got, want, equal_nan=True) if want.dtype.kind == 'f' else np.array_equal(got, want)
        return None if same else f'{key}: {int((got != want).sum())} of {want.size} values differ'
    if isinstance(want, (adjacency.Adjacency, critical.CriticalPoints, critical.BondGraph, merge.Merge, laplacian.PointProperties)):
        for k, w in vars(want).items():
            msg = differs(getattr(got, k), w, f'{key}.{k}')
            if msg:
                return msg
        return None
    if isinstance(want, (tuple, list)) and any(isinstance(w, np.ndarray) for w in want):
        return next((m for m in (differs(g, w, key) for g, w in zip(got, want)) if m), None)
    return None if got == want else f'{key}: {got!r} for {want!r}'


def eq(got, want, key):
    """a result against its restatement: the values (the restatements do not all return the library's dtypes)"""
    return differs(got, want, key, strict=False)


def within(got, want, lim, key):
    got = np.asarray(host(got), np.float64)
    if got.shape != np.shape(want):
        return f'{key}: shape {got.shape} for {np.shape(want)}'
    err = np.abs(got - want)
    return None if np.all(err <= lim) else f'{key}: off by {float(np.max(err - lim)):.3e} beyond the bound'


# ---- the restatements, each on the run's own maps --------------------------------------------------------------------------------
def lin_of(vox):
    return np.ravel_multi_index(tuple(np.asarray(vox, dtype=np.int64).reshape(-1, 3).T), SHAPE)


def check_weight(b, ref, dens, spin, tol):
    vv = b.voxel_volume
    al = weight.voronoi_weights(LAT / np.array(SHAPE, dtype=np.float64)[:, None])
    labels = np.asarray(host(b.atoms_volumes)) if tol is not None else None
    m, A, V, _ = memo(restate, ref, dens, al, labels)
    vox = np.stack(np.unravel_index(m, SHAPE), axis=1).astype(np.int64)
    out = [eq(b.weight_maxima, vox, 'weight_maxima'), eq(b.weight_charge, A * vv, 'weight_charge'),
           eq(b.weight_volume, V * vv, 'weight_volume')]
    wa, _ = oracle.atom_assign(np.dot(np.divide(np.add(vox, b.voxel_offset_fractional), SHAPE), LAT), ATOMS, LAT)
    out.append(eq(b.weight_atoms, wa, 'weight_atoms'))
    for name, per_max in (('atoms_weight_charge', A * vv), ('atoms_weight_volume', V * vv)):
        want = np.zeros(N_ATOMS)
        np.add.at(want, wa, per_max)
        out.append(eq(getattr(b, name), want, name))
    if spin is not None:
        _, S, _, _ = memo(restate, ref, spin, al, labels)
        want = np.zeros(N_ATOMS)
        np.add.at(want, wa, S * vv)
        out.append(eq(b.atoms_weight_spin, want, 'atoms_weight_spin'))
    return [m for m in out if m]


def check_multipole(b, ref, dens, spin, tol):
    vv, out = b.voxel_volume, []
    centres = ATOMS - b.voxel_offset
    jobs = [('atoms_moments', dens, b.atoms_volumes, centres)]
    if spin is not None:
        jobs.append(('atoms_spin_moments', spin, b.atoms_volumes, centres))
    if hasattr(b, 'bader_volumes'):
        jobs.append(('bader_moments', dens, b.bader_volumes, b.bader_maxima - b.voxel_offset))
    for name, rho, lab, cen in jobs:
        cen = np.ascontiguousarray(cen)
        terms, _, label = memo(reference_terms, rho, np.asarray(host(lab)), LAT, cen)
        s, cnt, mag = moment_grouped(terms, label, cen.shape[0])
        out.append(within(getattr(b, name), s * vv, moment_bound(cnt, mag, vv), name))
    out.append(eq(b.atoms_dipole, multipole.dipole(b.atoms_moments), 'atoms_dipole'))
    out.append(eq(b.atoms_quadrupole, multipole.quadrupole(b.atoms_moments), 'atoms_quadrupole'))
    return [m for m in out if m]


def check_adjacency(b, ref, dens, spin, tol):
    out = []
    dirs, areas = adjacency.active_directions(LAT / 24.0)
    jobs = [('atoms_adjacency', b.atoms_volumes, N_ATOMS)]
    if hasattr(b, 'bader_volumes'):
        jobs.append(('bader_adjacency', b.bader_volumes, b.bader_maxima.shape[0]))
    for name, lab, n in jobs:
        adj = getattr(b, name)
        want = memo(reference_adjacency, ref, np.asarray(host(lab)), n, dirs)
        out += [eq(adj.pairs, want[0], name + '.pairs'), eq(adj.facets, want[1], name + '.facets'),
                eq(adj.saddle_density.view(np.uint64), want[2].view(np.uint64), name + '.saddle_density'),
                eq(adj.saddle_facet, want[3], name + '.saddle_facet'),
                eq(adj.area, adjacency.facet_area(want[1], areas), name + '.area')]
        voxels, pos = adjacency.saddle_geometry(want[3], dirs, SHAPE, LAT, b.voxel_offset)
        out += [eq(adj.saddle_voxels, voxels, name + '.saddle_voxels'), eq(adj.saddle_position, pos, name + '.saddle_position')]
    if hasattr(b, 'bader_volumes'):
        vox = b._bader_maxima_voxels
        top = ref[vox[:, 0], vox[:, 1], vox[:, 2]]
        want = adjacency.persistence(*memo(reference_adjacency, ref, np.asarray(host(b.bader_volumes)), len(top), dirs)[0:3:2], top)
        out.append(eq(b.bader_persistence, want, 'bader_persistence'))
    return [m for m in out if m]


def _bonds(g):
    return g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin


def check_critical(b, ref, dens, spin, tol):
    want = memo(reference_points, ref, tol)
    cp = b.critical_points
    out = [eq(g, w, 'critical_points.' + k) for k, g, w in zip(('counts', 'lin', 'masks', 'ring', 'bond'),
                                                                      (cp.counts, cp.lin, cp.masks, cp.ring, cp.bond), want)]
    vox = np.stack(np.unravel_index(want[1], SHAPE), axis=1).astype(np.int64)
    out += [eq(b.critical_counts, want[0], 'critical_counts'), eq(b.critical_voxels, vox, 'critical_voxels'),
            eq(b.critical_kinds, cp.kinds, 'critical_kinds'),
            eq(b.critical_positions, critical.positions(vox, SHAPE, LAT) + b.voxel_offset, 'critical_positions')]
    jobs = [('atoms_bond_graph', b.atoms_volumes, N_ATOMS)]
    if hasattr(b, 'bader_volumes'):
        jobs.append(('bader_bond_graph', b.bader_volumes, b.bader_maxima.shape[0]))
    for name, lab, n in jobs:
        w = memo(reference_bonds, ref, np.asarray(host(lab)), n, tol)
        out.append(eq(_bonds(getattr(b, name))[:4], w[:4], name))
        out.append(eq(getattr(b, name).same_basin, w[4], name + '.same_basin'))
    g = b.atoms_bond_graph
    out += [eq(b.atoms_bonds, g.pairs, 'atoms_bonds'), eq(b.atoms_bond_saddles, g.saddles, 'atoms_bond_saddles')]
    if hasattr(b, 'bader_volumes'):
        out.append(eq(b.bader_bonds, b.bader_bond_graph.pairs, 'bader_bonds'))
    return [m for m in out if m]


def check_laplacian(b, ref, dens, spin, tol):
    vv, out = b.voxel_volume, []
    lap = memo(restated_laplacian, ref, LAT)
    jobs = [('atoms', b.atoms_volumes, N_ATOMS)]
    if hasattr(b, 'bader_volumes'):
        jobs.append(('bader', b.bader_volumes, b.bader_maxima.shape[0]))
    for name, lab, n in jobs:
        s, cnt, mag = lap_grouped(lap, np.asarray(host(lab)), n)
        lim = lap_sum_bound(cnt, mag, vv)
        out += [within(getattr(b, name + '_laplacian'), s * vv, lim, name + '_laplacian'),
                within(getattr(b, name + '_laplacian_abs'), mag * vv, lim, name + '_laplacian_abs')]
    if b.critical_flag:
        p, lin = b.critical_properties, b.critical_points.lin
        ten = restated_points(ref, LAT, lin)
        got = np.column_stack([p.rho, p.gradient, p.hessian[:, [0, 0, 0, 1, 1, 2], [0, 1, 2, 1, 2, 2]]])
        out += [eq(np.ascontiguousarray(got).view(np.uint64), ten.view(np.uint64), 'critical_properties'),
                eq(b.critical_laplacian.view(np.uint64), lap.reshape(-1)[lin].view(np.uint64), 'critical_laplacian'),
                eq(b.critical_hessian, p.hessian, 'critical_hessian'), eq(b.critical_eigenvalues, p.eigenvalues, 'critical_eigenvalues'),
                eq(b.critical_ellipticity, p.ellipticity, 'critical_ellipticity'),
                eq(b.atoms_bond_laplacian.view(np.uint64), lap.reshape(-1)[b.atoms_bond_graph.voxel].view(np.uint64), 'atoms_bond_laplacian')]
    return [m for m in out if m]


def check_voronoi(b, ref, dens, spin, tol):
    vv = b.voxel_volume
    want = memo(reference_labels, SHAPE, LAT, np.ascontiguousarray(ATOMS - b.voxel_offset))
    if tol is not None:
        want = np.where(ref <= tol, -1, want)
    got = np.asarray(host(b.voronoi_volumes))
    out = [None if np.array_equal(got, want) else f'voronoi_volumes: {int((got != want).sum())} voxels differ']
    counts = np.bincount(want[want >= 0], minlength=N_ATOMS)
    out.append(eq(b.voronoi_volume, counts.astype(np.float64) * vv, 'voronoi_volume'))
    # (exact sums of multiples of 2^-20, one multiply: tests/test_gpu_voronoi.py compares the same way)
    out.append(eq(b.voronoi_charge, np.array([dens[want == a].sum() for a in range(N_ATOMS)]) * vv, 'voronoi_charge'))
    if spin is not None:
        out.append(eq(b.voronoi_spin, np.array([spin[want == a].sum() for a in range(N_ATOMS)]) * vv, 'voronoi_spin'))
    return [m for m in out if m]


def check_sums(b, ref, dens, spin, tol):
    """the charge sums of the run itself on its final maps: they integrate `density` (exact on this input)"""
    vv, out = b.voxel_volume, []
    jobs = [('atoms', b.atoms_volumes, N_ATOMS)]
    if hasattr(b, 'bader_volumes'):
        jobs.append(('bader', b.bader_volumes, b.bader_maxima.shape[0]))
    for name, lab, n in jobs:
        lab = np.asarray(host(lab)).astype(np.int32)
        for what, rho in (('charge', dens), ('spin', spin)):
            if rho is None:
                continue
            ch, vo = np.zeros(n), np.zeros(n)
            oracle.charge_sum(ch, vo, vv, rho, lab)
            out += [eq(getattr(b, f'{name}_{what}'), ch, f'{name}_{what}'), eq(getattr(b, f'{name}_volume'), vo, f'{name}_volume')]
    return [m for m in out if m]


CHECKS = {'weight_flag': check_weight, 'multipole_flag': check_multipole, 'adjacency_flag': check_adjacency,
          'critical_flag': check_critical, 'laplacian_flag': check_laplacian, 'voronoi_flag': check_voronoi}


def verify(b, profile, what):
    """every feature whose flag is set on `b`, and the run's own sums, against the restatements on the right fields"""
    f = fields_of(profile)
    bad = check_sums(b, *f)
    for flag, fn in CHECKS.items():
        if getattr(b, flag):
            bad += fn(b, *f)
    assert not bad, f'{profile}, {what}: ' + ' | '.join(bad[:5])


def same_exact_attributes(a, b, what, skip=()):
    """every attribute of `b` is an attribute of `a`, equal bit for bit unless it is a sum of float atomics"""
    for key, want in vars(b).items():
        if key in SKIP or key in ATOMICS or key in skip:
            continue
        assert hasattr(a, key), f'{what}: {key} is missing'
        msg = differs(getattr(a, key), want, key)
        assert msg is None, f'{what}: {msg}'
    for key in ATOMICS & set(vars(b)):
        assert hasattr(a, key) and np.shape(host(getattr(a, key))) == np.shape(host(getattr(b, key))), f'{what}: {key}'


def unmerged_of(profile):
    """the Bader map before the merge and its maxima's voxels, by the steps _run takes (as tests/test_gpu_merge.py gets them)"""
    keep = make(profile, adjacency_flag=True)
    keep.persistence_tol = None
    keep.adjacency_flag = True
    keep.volumes_init()
    if keep.speed_flag:
        keep.bader_calc()
    elif keep.fused:
        keep.bader_calc_refine()
    else:
        keep.bader_calc()
        keep.refine_volumes(keep.bader_volumes)
    return np.asarray(host(keep.bader_volumes)), keep._bader_maxima_voxels.copy(), keep


def oracle_map(ref, tol, mode):
    vl = np.divide(LAT, SHAPE)
    dm, tg = distance_matrix(vl), gradient_transform(vl)
    vol0 = np.zeros(SHAPE, np.int32)
    vol0, _, _ = oracle.vacuum_assign(ref, vol0, float('nan') if tol is None else tol, ref, 1.0)
    lab, maxima = rank_labels(own_map(ref, vol0, dm, tg, main_ties=True))
    v = lab.astype(np.int32).copy()
    oracle.refine('neargrid', mode, ref, v, dm, tg, 1)
    return v, maxima


@pytest.mark.parametrize('profile', list(PROFILES))
def test_bader_with_every_flag(profile, monkeypatch):
    cache_facet_areas(monkeypatch)
    if PROFILES[profile].get('tensor') and not (torch is not None and torch.cuda.is_available()):
        pytest.skip('torch sees no device')
    monkeypatch.setattr(thread_handlers, 'VERBOSE', False)
    ref, dens, spin, tol = fields_of(profile)
    every = make(profile, **{f: True for f in FLAGS})
    every()
    # 2: the restatements, on the right fields -- and with another reference the swapped fields must be told apart
    verify(every, profile, 'every flag')
    if PROFILES[profile].get('reference'):
        for flag, fn in CHECKS.items():
            assert fn(every, dens, ref, spin, tol), f'{profile}: {flag} does not tell the reference from the density'
        assert check_sums(every, dens, ref, spin, tol)
    # 3: the documented precedence
    a = every.atoms_adjacency
    assert every.atoms_bond_density is a.saddle_density and every.atoms_bond_position is a.saddle_position
    assert every.atoms_bond_area is a.area
    assert every.atoms_bond_density.shape == (len(a),) and every.atoms_bond_graph.rho_b.shape == (len(every.atoms_bond_graph),)
    # the merge, against the restatement on the unmerged map
    unmerged, vox, keep = unmerged_of(profile)
    n = vox.shape[0]
    dirs, _ = adjacency.active_directions(LAT / 24.0)
    want = memo(reference_merge, ref, unmerged, n, dirs, lin_of(vox), PERSISTENCE, 64)
    m = every.bader_merge
    assert np.array_equal(m.root, want['root']) and np.array_equal(m.merge_round, want['merge_round'])
    assert np.array_equal(m.merge_persistence.view(np.uint64), want['merge_persistence'].view(np.uint64))
    assert (m.rounds, m.converged, len(m)) == (want['rounds'], want['converged'], want['n_survivors'])
    assert np.array_equal(every._bader_maxima_voxels, vox[m.survivors])
    if not every.speed_flag:
        assert np.array_equal(host(every.bader_volumes), swapped(unmerged, m.swap))
    print(profile, ':', n, 'maxima before the merge,', len(m), 'after', m.rounds, 'rounds')
    # 4: the oracle's map and sums
    if profile in ('default', 'vacuum and spin'):
        v, maxima = oracle_map(ref, tol, every.refine_mode)
        assert np.array_equal(unmerged, v) and np.array_equal(lin_of(vox), maxima), 'the Bader map before the merge is not the oracle\'s'
        merged = swapped(v, np.searchsorted(np.flatnonzero(want['merge_round'] < 0), want['root']))
        cart = np.dot(np.divide(np.add(vox[m.survivors], every.voxel_offset_fractional), SHAPE), LAT)
        ba, bd, atoms_map = oracle.assign_to_atoms(cart, ATOMS, LAT, merged)
        assert np.array_equal(every.bader_atoms, ba) and np.array_equal(every.bader_distance, bd)
        assert np.array_equal(host(every.atoms_volumes), atoms_map)
        ch, vo = np.zeros(N_ATOMS), np.zeros(N_ATOMS)
        oracle.charge_sum(ch, vo, every.voxel_volume, dens, atoms_map.astype(np.int32))
        assert np.array_equal(every.atoms_charge, ch) and np.array_equal(every.atoms_volume, vo)
    # 1: every attribute of a run with one flag
    for flag in FLAGS:
        one = make(profile, **{flag: True})
        one()
        verify(one, profile, flag + ' alone')
        # (with adjacency_flag as well, atoms_bond_density and atoms_bond_position are bond_surfaces()'s: see 3)
        skip = ('atoms_bond_density', 'atoms_bond_position') if flag == 'critical_flag' else ()
        same_exact_attributes(every, one, f'{profile}: every flag against {flag} alone', skip)
        if flag == 'critical_flag':
            assert differs(every.atoms_bond_graph, one.atoms_bond_graph, 'atoms_bond_graph') is None
            assert differs(one.atoms_bond_density, every.atoms_bond_graph.rho_b, 'atoms_bond_density') is None
    # 5: a second call on the same object
    first = {k: v for k, v in vars(every).items()}
    every()
    verify(every, profile, 'every flag, second call')
    assert set(vars(every)) == set(first)
    for key, wanted in first.items():
        if key in SKIP or key in ATOMICS:
            continue
        msg = differs(getattr(every, key), wanted, key)
        assert msg is None, f'{profile}: the second call differs: {msg}'
