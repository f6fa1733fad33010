"""Shared by tests/test_history_cpu.py and tests/test_gpu_history.py: the inputs, the expectation of every public call and the
comparison of a result with it, for tests that run the calls one after another on one context.

Every expectation comes from what the feature's own test file imports (the oracle, or that file's numpy restatement) and every
comparison is the one that file makes: `==` (or equal bits) where it compares so, its rounding bound with its arguments elsewhere.
Nothing is restated a second time and no tolerance is new.  Expectations are memoised on (kind, grid, the inputs the kind reads).
The Hirshfeld, ISA, NCI, isosurface and regions kinds stand on tests/test_hirshfeld_cpu.py, test_isa_cpu.py, test_nci_cpu.py,
test_isosurface_cpu.py and test_regions_cpu.py, the MBIS, stockholder-moments, DORI and IGM kinds on test_mbis_cpu.py,
test_stockmom_cpu.py, test_dori_cpu.py and test_igm_cpu.py, which also hold the comparisons their GPU files make (check_s,
check_sums, first_difference, sums_difference, same_rows, info_of, regions_difference, ...): those files import
tests/test_gpu_history.py, so the helpers cannot live there.

    GRIDS, density(grid, name), labels(grid, name), n_of(grid, name)   the inputs
    KINDS                                                               call kind -> (reads the density, reads the map)
    expect(kind, grid, dname, mname)                                    what the call must return
    check(kind, got, (grid, dname, mname))                              None, or a message naming the kind and the first difference
    walk(seed, steps)                                                   the seeded step list of test_seeded_walks (pure Python)"""
import functools
import math
import random

import numpy as np

import oracle
import test_dori_cpu as TD
import test_hirshfeld_cpu as THS
import test_igm_cpu as TI
import test_isa_cpu as TISA
import test_isosurface_cpu as TISO
import test_mbis_cpu as TM
import test_nci_cpu as TN
import test_regions_cpu as TR
import test_stockmom_cpu as TS
from oracle_context import OracleContext
from pybader_amd import isa, mbis, synth
from pybader_amd.hirshfeld import ProAtoms
from pybader_amd.adjacency import active_directions
from pybader_amd.interface import distance_matrix, gradient_transform
from pybader_amd.weight import voronoi_weights
from rough_common import own_map, rank_labels
from test_adjacency_cpu import reference_adjacency
from test_critical_cpu import noise_labels, reference_bonds, reference_points
from test_gpu_isa import restated_sums as isa_sums
from test_gpu_sums import bound as sum_bound_any_order
from test_gpu_sums import grouped as sum_grouped
from test_gpu_sums import swapped
from test_laplacian_cpu import cell_sum_bound, coefficients, restated_laplacian, restated_points
from test_laplacian_cpu import grouped as lap_grouped
from test_laplacian_cpu import sum_bound as lap_sum_bound
from test_merge_cpu import maxima_of, reference_merge
from test_multipole_cpu import VV, reference_terms
from test_multipole_cpu import bound as moment_bound
from test_multipole_cpu import grouped as moment_grouped
from test_voronoi_cpu import reference_labels
from test_weight_cpu import restate

# G1: no whole 8^3 bricks, one partial 8 x 8 x 32 tile in z.  G2: two axes below a brick, z one voxel past a tile.  G3: larger
# than G1 along x, smaller along y and z: G1 -> G2 -> G3 -> G1 makes every buffer kept "while the shape stays" shrink and regrow.
GRIDS = {'G1': (24, 20, 28), 'G2': (9, 7, 33), 'G3': (40, 12, 16)}
ORDER = ('G1', 'G2', 'G3')
LAT = synth.TRICLINIC
# (frac_x, frac_y, frac_z, sigma, amplitude): three unequal atoms each, at different places
ATOMS_A = np.array([[0.231, 0.269, 0.247, 0.42, 7.50], [0.773, 0.261, 0.739, 0.45, 5.00], [0.257, 0.743, 0.629, 0.37, 3.25]])
ATOMS_B = np.array([[0.761, 0.738, 0.271, 0.36, 5.25], [0.243, 0.233, 0.757, 0.49, 8.00], [0.651, 0.247, 0.233, 0.40, 2.75]])
SITES = {'A': np.ascontiguousarray(ATOMS_A[:, :3] @ LAT), 'B': np.ascontiguousarray(ATOMS_B[:, :3] @ LAT)}   # Cartesian
SITES8 = synth.atoms_cartesian(synth.ATOMS8, LAT)      # surface_distance: a site for every label any map carries
NOISE = 0.02            # amplitude of the hash noise on density N (G1): ripples that the merge removes
VAC_TOL = 0.05          # vacuum tolerance of the calls that take one
MERGE_TOL = 0.03
SWAP = np.array([2, 0, 3, 1], np.int64)                 # volume_assign: labels >= 4 and -1 stay
MASK_LABEL = 1
N_POINTS = 24
REFINE_MODE = ('changed', -1)
SPECIES = np.arange(3, dtype=np.int32)                  # Hirshfeld: a pro-atom per atom
PRO_R_CUT, PRO_KNOTS = 2.5, 256
ISA = dict(r_cut=2.5, shells=8, tol=0.0, max_iter=5, check_every=2)        # three library calls: 2 + 2 + 1 iterations
NCI_CUTS, NCI_EDGES = TN.HISTORY_CUTS, TN.HISTORY_EDGES
ISO_QUANTILE = 0.7
FIELD_LEVEL = 0.0                                       # the *_of_field kinds: the zero envelope of the other density's Laplacian
MBIS_SHELLS = np.array([1, 2, 1], np.int32)
MBIS = dict(r_cut=2.5, tol=0.0, max_iter=5, check_every=2)                 # three library calls: 2 + 2 + 1 iterations
MBIS_KNOTS, MBIS_X_MAX = 256, 48
DORI_RHO_MIN = 1e-3                                     # dori_fields
DORI_CUTS = TD.SUM_CUTS                                 # (d_cut, rho_min, rho_split) of dori_regions, dori_domains, dori_isosurface
FRAGMENTS = np.array([0, 1, 0], np.int32)               # IGM: the second atom against the two others
IGM_RHO_SPLIT = NCI_CUTS[2]
IGM_QUANTILE = 0.25


def shape_of(grid):
    return GRIDS[grid]


@functools.lru_cache(maxsize=None)
def geometry(grid):
    vl = np.divide(LAT, GRIDS[grid])
    return distance_matrix(vl), gradient_transform(vl)


def voxel_volume(grid):
    """the cell's volume over the voxel count, formed as weight.weight_sum forms it"""
    return np.abs(np.dot(LAT[0], np.cross(*LAT[1:]))) / np.prod(GRIDS[grid])


@functools.lru_cache(maxsize=None)
def density(grid, dname):
    """A, B: synthetic atoms.  N (G1): A + hash noise.  X32: X rounded to float32 (what a float32 device tensor of X holds).
    Never written: the tests that edit a density in place work on a copy."""
    if dname.endswith('+'):
        rho = edited(density(grid, dname[:-1]).copy(), 'density')
    elif dname.endswith('32'):
        rho = density(grid, dname[:-2]).astype(np.float32).astype(np.float64)
    elif dname == 'N':
        rho = density(grid, 'A') + NOISE * synth.hash_noise(GRIDS[grid], 9)
    else:
        rho = synth.synth_density(GRIDS[grid], LAT, {'A': ATOMS_A, 'B': ATOMS_B}[dname])
    rho = np.ascontiguousarray(rho)
    rho.flags.writeable = False
    return rho


def densities(grid):
    return ('A', 'B', 'N') if grid == 'G1' else ('A', 'B')


@functools.lru_cache(maxsize=None)
def bader(grid, dname):
    """the library-independent Bader partition of a density, as tests/soak_vs_oracle.py builds it: the own-trajectory map ranked
    by first voxel, then the oracle's refinement of it"""
    rho, (dm, tg) = density(grid, dname), geometry(grid)
    shape = rho.shape
    vol0 = np.zeros(shape, np.int32)
    lab, maxima = rank_labels(own_map(rho, vol0, dm, tg, main_ties=True))
    v, log = lab.astype(np.int32).copy(), []
    oracle.refine('neargrid', REFINE_MODE, rho, v, dm, tg, 1, log=log)
    vox = np.stack(np.unravel_index(maxima, shape), axis=1).astype(np.int64).reshape(-1, 3)
    out = {'assign': lab.astype(np.int32), 'maxima': maxima, 'voxels': vox, 'refined': v, 'log': [tuple(int(x) for x in r) for r in log]}
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.flags.writeable = False
    return out


def maxima_cart(grid, dname='A'):
    return np.dot(np.ascontiguousarray(np.divide(bader(grid, dname)['voxels'].astype(np.float64), GRIDS[grid])), LAT)


def maps(grid):
    return ('bader', 'atoms', 'noise', 'baderN') if grid == 'G1' else ('bader', 'atoms', 'noise')


@functools.lru_cache(maxsize=None)
def labels(grid, mname):
    """bader: the refined Bader map of A.  atoms: its atom map.  noise: test_critical_cpu.noise_labels (labels -1 and >= n).
    baderN (G1): the refined Bader map of the noisy density.  int32, never written."""
    if mname.endswith('+'):
        lab = edited(labels(grid, mname[:-1]).copy(), 'labels')
    elif mname == 'bader':
        lab = bader(grid, 'A')['refined']
    elif mname == 'baderN':
        lab = bader(grid, 'N')['refined']
    elif mname == 'atoms':
        ba, _ = oracle.atom_assign(maxima_cart(grid), SITES['A'], LAT)
        lab = swapped(bader(grid, 'A')['refined'], ba)
    else:
        lab = noise_labels(GRIDS[grid])
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    lab.flags.writeable = False
    return lab


def n_of(grid, mname):
    """the number of labels a call on this map is told"""
    mname = mname.rstrip('+')
    if mname == 'noise':
        return 5
    if mname == 'atoms':
        return 3
    return int(bader(grid, 'N' if mname == 'baderN' else 'A')['maxima'].shape[0])


def centres(grid, mname):
    """moment_sum: a Cartesian centre per label"""
    mname = mname.rstrip('+')
    n = n_of(grid, mname)
    if mname in ('bader', 'baderN'):
        return maxima_cart(grid, 'N' if mname == 'baderN' else 'A')
    return np.ascontiguousarray(np.resize(SITES8, (n, 3)))


@functools.lru_cache(maxsize=None)
def vacuum_map(grid, dname):
    vol, _, _ = oracle.vacuum_assign(density(grid, dname), np.zeros(GRIDS[grid], np.int32), VAC_TOL, density(grid, dname), 1.0)
    vol.flags.writeable = False
    return vol


def other(dname):
    """the second field of the calls that take two: another density of the same grid"""
    return 'B32' if dname == 'A32' else {'A': 'B', 'B': 'A', 'N': 'B'}.get(dname.rstrip('+'), 'A')


@functools.lru_cache(maxsize=None)
def alpha(grid):
    return voronoi_weights(LAT / np.array(GRIDS[grid], dtype=np.float64)[:, None])


@functools.lru_cache(maxsize=None)
def directions(grid):
    return active_directions(LAT / np.array(GRIDS[grid], dtype=np.float64)[:, None])[0]


@functools.lru_cache(maxsize=None)
def point_list(grid):
    """point_properties: the corners of the grid and hashed voxels (repeats allowed)"""
    n = int(np.prod(GRIDS[grid]))
    return np.concatenate([[0, n - 1], np.floor(synth.hash_noise((N_POINTS - 2,), 17) * n).astype(np.int64)]).astype(np.int64)


def cache_facet_areas(monkeypatch):
    """weight.voronoi_areas is a pure host function of the voxel lattice that takes 0.2 s of Python; weight_sum, adjacency and
    merge_basins each call it once per call.  For the duration of a test it is computed once per lattice (a copy per call, as
    the function itself returns a fresh array): the calls under test and what they read on the device are untouched."""
    from pybader_amd import adjacency, weight
    plain, seen = weight.voronoi_areas, {}

    def cached(voxel_lattice, who='voronoi_areas'):
        key = (np.asarray(voxel_lattice, dtype=np.float64).tobytes(), who)
        if key not in seen:
            seen[key] = plain(voxel_lattice, who)
        return seen[key].copy()
    monkeypatch.setattr(weight, 'voronoi_areas', cached)
    monkeypatch.setattr(adjacency, 'voronoi_areas', cached)


# ---- the call kinds: name -> (reads the density, reads the map) --------------------------------------------------------------
KINDS = {
    'vacuum_assign': (True, False), 'bader_calc': (True, False), 'refine': (True, False), 'bader_calc_refine': (True, False),
    'assign_to_atoms': (False, True), 'surface_distance': (False, True), 'charge_sum': (True, True), 'volume_mask': (True, True),
    'volume_assign': (False, True),
    'weight_own': (True, False), 'weight_other': (True, False), 'weight_vacuum': (True, False),
    'moment_sum': (True, True), 'adjacency': (True, True), 'merge': (True, True),
    'voronoi': (True, False), 'voronoi_full': (True, False), 'voronoi_vacuum': (True, False), 'voronoi_full_vacuum': (True, False),
    'critical': (True, False), 'critical_flood': (True, False), 'critical_vacuum': (True, False), 'critical_flood_vacuum': (True, False),
    'bond_graph': (True, True),
    'laplacian': (True, False), 'laplacian_gather': (True, False), 'basin_laplacian': (True, True), 'point_properties': (True, False),
    'hirshfeld_charges': (True, False), 'hirshfeld_charges_full': (True, False), 'promolecule': (False, False), 'deformation': (True, False),
    'isa_charges': (True, False), 'isa_charges_direct': (True, False), 'isa_residual': (True, False),
    'nci_fields': (True, False), 'nci_fields_gather': (True, False), 'nci_regions': (True, True), 'nci_histogram': (True, False),
    'nci_domains': (True, True),
    'isosurface': (True, True), 'isosurface_gather': (True, True), 'isosurface_of_field': (True, True),
    'regions': (True, True), 'regions_below': (True, True), 'regions_global': (True, True), 'regions_of_field': (True, True),
    'mbis_charges': (True, False), 'mbis_charges_direct': (True, False), 'mbis_promolecule': (False, False), 'mbis_residual': (True, False),
    'hirshfeld_moments': (True, False), 'hirshfeld_moments_direct': (True, False), 'isa_moments': (True, False),
    'mbis_moments': (True, False),
    'dori_fields': (True, False), 'dori_fields_gather': (True, False), 'dori_regions': (True, True), 'dori_domains': (True, True),
    'dori_isosurface': (True, False),
    'igm_fields': (True, False), 'igm_fields_pro': (True, False), 'igm_fields_isa': (True, False), 'igm_regions': (True, True),
    'igm_domains': (True, True), 'igm_isosurface': (True, False),
}
# surface_distance takes the density and its result does not depend on it (the edge voxels are the map's).
# voronoi_assign without a tolerance reads no density: its second input is the atom set, which goes with the density's name;
# so do the atoms and pro-atoms of the Hirshfeld kinds and the atoms of the ISA kinds (promolecule reads nothing else).
# The *_of_field kinds take the Laplacian of other(density name) as a host field beside the density: the mesh and the members
# come from that field, the volumes' shares from the map, top and the sums from the density, which must stay the resident one.
# The atoms of the MBIS, moments and IGM kinds go with the density's name as well; mbis_promolecule reads nothing else, and is
# handed the restated shells of that name's own density.  mbis_residual, isa_moments, mbis_moments and igm_fields_isa are handed
# results built from the restatement of the density they are called on (mbis_result, isa_result): no GPU run made them.
# dori_isosurface and igm_isosurface take no label map (dori.dori_isosurface, igm.igm_isosurface have no such argument): their
# meshes depend on the density alone, so they are (True, False)
LABEL_WRITERS = ('voronoi', 'voronoi_full', 'voronoi_vacuum', 'voronoi_full_vacuum', 'volume_assign')


def sites_of(dname):
    return SITES['B' if dname.startswith('B') else 'A']


def map_for(kind, mname):
    """the map a call of this kind gets when the step names `mname`: surface_distance indexes its eight sites by label, so the
    noisy density's Bader map (hundreds of labels) is replaced by the atom map there"""
    return 'atoms' + '+' * mname.endswith('+') if kind == 'surface_distance' and mname.startswith('baderN') else mname


def maxima_for(grid, mname):
    """assign_to_atoms: the Cartesian maxima that go with the map (the noisy density's for its own Bader map)"""
    return maxima_cart(grid, 'N' if mname.startswith('baderN') else 'A')


def _key(kind, grid, dname, mname):
    reads_d, reads_m = KINDS[kind]
    mname = map_for(kind, mname)
    if kind in ('voronoi', 'voronoi_full', 'promolecule', 'mbis_promolecule'):
        dname = 'B' if dname.startswith('B') else 'A'
    return kind, grid, dname if reads_d or kind in ('promolecule', 'mbis_promolecule') else None, mname if reads_m else None


def expect(kind, grid, dname, mname):
    return _expect(*_key(kind, grid, dname, mname))


@functools.lru_cache(maxsize=None)
def _laplacian(grid, dname):
    lap = restated_laplacian(density(grid, dname), LAT)
    lap.flags.writeable = False
    return lap


def atoms_of(dname):
    return 'B' if dname.startswith('B') else 'A'


@functools.lru_cache(maxsize=None)
def proatoms(which):
    return THS.synth_proatoms({'A': ATOMS_A, 'B': ATOMS_B}[which], PRO_R_CUT, PRO_KNOTS)


@functools.lru_cache(maxsize=None)
def _promolecule(grid, which):
    """(P, p) of test_hirshfeld_cpu.restate for the atoms and pro-atoms `which` on a grid"""
    P, p = THS.restate(GRIDS[grid], LAT, SITES[which], SPECIES, proatoms(which))
    P.flags.writeable = False
    p.flags.writeable = False
    return P, p


@functools.lru_cache(maxsize=None)
def _isa(grid, dname):
    """the ISA run of a density restated by tests/test_isa_cpu.py: geometry, exponent, the qsum rows and the tables after each of
    the iterations -> (g, e, rows, tables after the last, max |rho|)"""
    rho = density(grid, dname)
    g = _isa_geometry(grid, atoms_of(dname))
    bound = float(np.max(np.abs(rho)))
    e = TISA.exponent(bound, g.count.max())
    rows, tabs = TISA.run(g, rho.reshape(-1), e, ISA['max_iter'])
    tabs[-1].flags.writeable = False
    return g, e, rows, tabs[-1], bound


@functools.lru_cache(maxsize=None)
def _isa_geometry(grid, which):
    return TISA.geometry(GRIDS[grid], LAT, SITES[which], ISA['r_cut'], ISA['shells'])


def isa_result(grid, dname):
    """an IsaResult with the restated tables (no GPU run made it): what isa_residual is handed"""
    _, _, _, tables, bound = _isa(grid, dname)
    return isa.IsaResult(tables=tables, r_cut=np.full(3, ISA['r_cut']), shells=ISA['shells'], rho_bound=bound)


@functools.lru_cache(maxsize=None)
def _nci(grid, dname):
    return TN.restated(density(grid, dname), LAT)


def iso_level(grid, dname):
    return float(np.quantile(density(grid, dname), ISO_QUANTILE))


def field_of(grid, dname):
    """the second field of the *_of_field kinds: the Laplacian of the other density of the grid, a host array"""
    return _laplacian(grid, other(dname))


def _components(mask, rho, lab, n):
    """the expectation of the regions kinds and of nci_domains from test_regions_cpu's restatement"""
    reg, seeds = TR.components(mask)
    count, top, terms = TR.per_component(reg, seeds.size, rho)
    return {'reg': reg, 'seeds': seeds, 'count': count, 'top': top, 's1': TR.sums(terms)[0], 's2': TR.sums([t * t for t in terms])[0],
            'shares': TR.shares(reg, lab, n), 'rho': rho}


@functools.lru_cache(maxsize=None)
def _mbis_geometry(grid, which):
    return TM.geometry(GRIDS[grid], LAT, SITES[which], MBIS['r_cut'])


@functools.lru_cache(maxsize=None)
def _mbis(grid, dname):
    """the MBIS run of a density restated by tests/test_mbis_cpu.py from mbis.default_initial -> (g, e, the rows of the five
    iterations, (N, sigma) after the last, max |rho|)"""
    rho = density(grid, dname)
    g = _mbis_geometry(grid, atoms_of(dname))
    bound = float(np.max(np.abs(rho)))
    e = TM.exponents(bound, g.count.max(), MBIS['r_cut'], g.N)
    N0, s0 = mbis.default_initial(MBIS_SHELLS)
    rows, pars = TM.run(g, TM.Table(TM.table(MBIS_KNOTS, MBIS_X_MAX), MBIS_KNOTS), MBIS_SHELLS, rho, N0, s0, bound, e, MBIS['max_iter'], VV)
    for a in pars[-1]:
        a.flags.writeable = False
    return g, e, rows, pars[-1], bound


def mbis_result(grid, dname):
    """an MbisResult with the restated shells (no GPU run made it): what mbis_promolecule, mbis_residual and mbis_moments are handed"""
    _, _, _, (N, sigma), bound = _mbis(grid, dname)
    return mbis.MbisResult(populations=N, widths=sigma, shells=MBIS_SHELLS, r_cut=np.full(3, MBIS['r_cut']), rho_bound=bound,
                           knots_per_unit=MBIS_KNOTS, x_max=MBIS_X_MAX, voxel_volume=VV)


def _mbis_total(grid, dname):
    g, _, _, (N, sigma), _ = _mbis(grid, dname)
    return TM.total(g, TM.Table(TM.table(MBIS_KNOTS, MBIS_X_MAX), MBIS_KNOTS), MBIS_SHELLS, N, sigma)


@functools.lru_cache(maxsize=None)
def _stock_geometry(grid, which):
    """the pairs of the three kinds of setup: one cutoff for every atom and a species per atom, so they are the same pairs"""
    assert PRO_R_CUT == ISA['r_cut'] == MBIS['r_cut'] and (proatoms(which).r_cut == PRO_R_CUT).all()
    return TS.geometry(GRIDS[grid], LAT, SITES[which], SPECIES, proatoms(which).r_cut)


def _moments(kind, grid, dname):
    """(bins, info, moments) of tests/test_stockmom_cpu.py's restatement at rho_bound = max |rho|, on the setup of the kind"""
    rho, which = density(grid, dname), atoms_of(dname)
    g = _stock_geometry(grid, which)
    if kind.startswith('hirshfeld'):
        term = TS.table_term(proatoms(which), SPECIES)
    elif kind.startswith('isa'):
        term = TS.isa_term(_isa(grid, dname)[3], np.full(3, ISA['r_cut']))
    else:
        term = TS.mbis_term(TM.Table(TM.table(MBIS_KNOTS, MBIS_X_MAX), MBIS_KNOTS), MBIS_SHELLS, *_mbis(grid, dname)[3])
    bound = float(np.max(np.abs(rho)))
    E = TS.exponents(bound, g.count.max(), PRO_R_CUT)
    b, beyond, _, _ = TS.bins(g, term, rho, bound, E)
    return b, TS.info_of(g, E, beyond), TS.moments(E, b, VV)


@functools.lru_cache(maxsize=None)
def _dori(grid, dname, rho_min):
    return TD.restated(density(grid, dname), LAT, rho_min)


@functools.lru_cache(maxsize=None)
def _igm_sums(grid, which):
    t = TI.table_sums(GRIDS[grid], LAT, SITES[which], SPECIES, proatoms(which))
    for a in t.values():
        a.flags.writeable = False
    return t


@functools.lru_cache(maxsize=None)
def _igm(grid, dname, mode='stockholder', on_isa=False):
    """the two fields of tests/test_igm_cpu.py's restatement for the fragments FRAGMENTS -> (dg, dgi), of the grid's shape"""
    rho, which = density(grid, dname), atoms_of(dname)
    if on_isa:          # (the ISA tables are piecewise constant: ProAtoms with a last column of zeros and flat=True, as test_gpu_igm.py)
        tables = _isa(grid, dname)[3]
        pro = ProAtoms(np.concatenate([tables, np.zeros((3, 1))], axis=1), np.full(3, ISA['r_cut']))
        v = TI.restate(GRIDS[grid], LAT, SITES[which], SPECIES, pro, rho, FRAGMENTS, TI.MODES[mode], flat=True)
    else:
        v = TI.restate(GRIDS[grid], LAT, SITES[which], SPECIES, proatoms(which), rho, FRAGMENTS, TI.MODES[mode], sums=_igm_sums(grid, which))
    out = v['dg'].reshape(GRIDS[grid]), v['dgi'].reshape(GRIDS[grid])
    for a in out:
        a.flags.writeable = False
    return out


def igm_cut(grid, dname):
    """the bound of igm_regions, igm_domains and igm_isosurface, picked from the restated delta-g_inter as tests/test_gpu_igm.py's
    igm_call picks its own (the field peaks near the cutoffs): a quantile of its positive values.  igm_call takes the median on
    (A, atoms); on (G2, B, noise) the median leaves 42 voxels with a label the sums count, fewer than the 50 the comparison asks
    for, so the lower quartile is taken here: tests/test_history_cpu.py asserts the 50 on every input a walk can draw"""
    dgi = _igm(grid, dname)[1]
    return float(np.quantile(dgi[dgi > 0], IGM_QUANTILE))


@functools.lru_cache(maxsize=None)
def _expect(kind, grid, dname, mname):
    shape = GRIDS[grid]
    rho = density(grid, dname) if dname is not None else None
    lab = labels(grid, mname) if mname is not None else None
    n = n_of(grid, mname) if mname is not None else None
    if kind == 'vacuum_assign':
        vol = vacuum_map(grid, dname)
        x = rho[vol == -1]
        return vol, math.fsum(x), int(x.size), math.fsum(np.abs(x))
    if kind == 'bader_calc':
        b = bader(grid, dname)
        return b['voxels'], b['assign']
    if kind == 'refine':
        b = bader(grid, dname)
        return b['refined'], b['log']
    if kind == 'bader_calc_refine':
        b = bader(grid, dname)
        return b['voxels'], b['refined'], b['log']
    if kind == 'assign_to_atoms':
        ba, bd = oracle.atom_assign(maxima_for(grid, mname), SITES['A'], LAT)
        return ba, bd, swapped(lab, ba)
    if kind == 'surface_distance':
        ref = OracleContext()
        ref.set_grid(shape, *geometry(grid))
        ref.upload_density(density(grid, 'A'))
        ref.upload_labels(lab)
        return ref.surface_distance(LAT, SITES8)
    if kind == 'charge_sum':
        return sum_grouped(rho, lab, n)
    if kind == 'volume_mask':
        return (np.where(lab == MASK_LABEL, rho, 0.0),)
    if kind == 'volume_assign':
        return (swapped(lab, SWAP),)
    if kind.startswith('weight_'):
        q = rho if kind != 'weight_other' else density(grid, other(dname))
        m, A, V, _ = restate(rho, q, alpha(grid), vacuum_map(grid, dname) if kind == 'weight_vacuum' else None)
        return np.stack(np.unravel_index(m, shape), axis=1).astype(np.int64).reshape(-1, 3), A, V
    if kind == 'moment_sum':
        terms, _, label = reference_terms(rho, lab, LAT, centres(grid, mname))
        return moment_grouped(terms, label, n)
    if kind == 'adjacency':
        return reference_adjacency(rho, lab, n, directions(grid))
    if kind == 'merge':
        idx = maxima_of(rho, lab, n)
        want = reference_merge(rho, lab, n, directions(grid), idx, MERGE_TOL, 64)
        survivors = np.flatnonzero(want['merge_round'] < 0)
        return want, swapped(lab, np.searchsorted(survivors, want['root']))
    if kind.startswith('voronoi'):
        want = reference_labels(shape, LAT, sites_of(dname))
        return (np.where(rho <= VAC_TOL, -1, want) if kind.endswith('vacuum') else want,)
    if kind.startswith('critical'):
        return reference_points(rho, VAC_TOL if kind.endswith('vacuum') else None)
    if kind == 'bond_graph':
        return reference_bonds(rho, lab, n)
    if kind in ('laplacian', 'laplacian_gather'):
        return (_laplacian(grid, dname),)
    if kind == 'basin_laplacian':
        return lap_grouped(_laplacian(grid, dname), lab, n)
    if kind == 'point_properties':
        lin = point_list(grid)
        return restated_points(rho, LAT, lin), _laplacian(grid, dname).reshape(-1)[lin]
    if kind.startswith('hirshfeld_charges'):
        return THS.restated_sums(rho, *_promolecule(grid, atoms_of(dname)))
    if kind == 'promolecule':
        return (_promolecule(grid, dname)[0].reshape(shape),)
    if kind == 'deformation':
        return ((rho.reshape(-1) - _promolecule(grid, atoms_of(dname))[0]).reshape(shape),)
    if kind.startswith('isa_charges'):
        g, e, rows, tables, _ = _isa(grid, dname)
        return e, rows, tables, isa_sums(g, rho, tables)
    if kind == 'isa_residual':
        g, _, _, tables, _ = _isa(grid, dname)
        return ((rho.reshape(-1) - TISA.total(g, tables)).reshape(shape),)
    if kind.startswith('nci_fields'):
        return (_nci(grid, dname),)
    if kind == 'nci_regions':
        return TN.sum_reference(_nci(grid, dname), lab, n, NCI_CUTS)
    if kind == 'nci_histogram':
        return (TN.histogram(_nci(grid, dname), *NCI_EDGES),)
    if kind == 'nci_domains':
        v = _nci(grid, dname)
        mask = TN.region(v, *NCI_CUTS[:2])
        out = _components(mask, rho, lab, n)
        cls = np.where(mask, TN.classes(v, NCI_CUTS[2]), -1)
        out['class_count'] = np.stack([np.bincount(out['reg'][cls == k], minlength=out['seeds'].size) for k in range(3)], axis=1).astype(np.int64)
        out['kind'] = cls.reshape(-1)[out['top']].astype(np.int8)
        return out
    if kind in ('isosurface', 'isosurface_gather'):
        return TISO.restate(rho, iso_level(grid, dname), LAT, TISO.colour_field(shape), lab, n)
    if kind == 'isosurface_of_field':
        return TISO.restate(field_of(grid, dname), FIELD_LEVEL, LAT, TISO.colour_field(shape), lab, n)
    if kind in ('regions', 'regions_global'):
        return _components(rho >= TR.sum_level(rho), rho, lab, n)
    if kind == 'regions_below':
        return _components(rho < TR.sum_level(rho), rho, lab, n)
    if kind == 'regions_of_field':
        return _components(field_of(grid, dname) >= FIELD_LEVEL, rho, lab, n)
    if kind.startswith('mbis_charges'):
        _, e, rows, (N, sigma), _ = _mbis(grid, dname)
        return (np.array([TM.results(e, row, VV)[0] for row in rows]), N, sigma) + TM.results(e, rows[-1], VV)
    if kind == 'mbis_promolecule':
        return (_mbis_total(grid, dname).reshape(shape),)
    if kind == 'mbis_residual':
        return ((rho.reshape(-1) - _mbis_total(grid, dname)).reshape(shape),)
    if kind.endswith(('_moments', '_moments_direct')):
        return _moments(kind, grid, dname)
    if kind.startswith('dori_fields'):
        v = _dori(grid, dname, DORI_RHO_MIN)
        return v['gamma'], v['x']
    if kind == 'dori_regions':
        return TD.sum_reference(_dori(grid, dname, DORI_CUTS[1]), lab, n, DORI_CUTS)
    if kind == 'dori_domains':
        v = _dori(grid, dname, DORI_CUTS[1])
        out = _components(v['gamma'] >= DORI_CUTS[0], rho, lab, n)
        out['value'] = v['gamma'].reshape(-1)[out['top']]
        out['kind'] = TD.classes(v, DORI_CUTS[2]).reshape(-1)[out['top']].astype(np.int8)
        return out
    if kind == 'dori_isosurface':
        v = _dori(grid, dname, DORI_CUTS[1])
        return TISO.restate(v['gamma'], DORI_CUTS[0], LAT, v['x'])
    if kind.startswith('igm_fields'):
        return _igm(grid, dname, 'pro' if kind.endswith('pro') else 'stockholder', kind.endswith('isa')) + (_nci(grid, dname)['x'],)
    if kind == 'igm_regions':
        return TI.sum_reference(rho, _igm(grid, dname)[1], _nci(grid, dname)['x'], lab, n, igm_cut(grid, dname), IGM_RHO_SPLIT)
    if kind == 'igm_domains':
        val, x = _igm(grid, dname)[1], _nci(grid, dname)['x']
        out = _components(val >= igm_cut(grid, dname), rho, lab, n)
        out['value'] = val.reshape(-1)[out['top']]
        xt = x.reshape(-1)[out['top']]
        out['kind'] = np.where(xt < -IGM_RHO_SPLIT, 0, np.where(xt > IGM_RHO_SPLIT, 2, 1)).astype(np.int8)
        out['integral'] = lap_grouped(val, out['reg'], out['seeds'].size)
        return out
    if kind == 'igm_isosurface':
        return TISO.restate(_igm(grid, dname)[1], igm_cut(grid, dname), LAT, _nci(grid, dname)['x'])
    raise KeyError(kind)


# ---- comparison ------------------------------------------------------------------------------------------------------------------
def _first(name, got, want, bits=False):
    """None when the two arrays are equal (in bits for floats when asked), else where they first differ"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        return f'{name}: shape {got.shape}, expected {want.shape}'
    if bits:
        got, want = np.ascontiguousarray(got, np.float64).view(np.uint64), np.ascontiguousarray(want, np.float64).view(np.uint64)
    diff = got != want
    if not diff.any():
        return None
    at = tuple(int(i) for i in np.argwhere(diff)[0]) if diff.ndim else ()
    g, w = np.asarray(got)[at], np.asarray(want)[at]
    return f'{name}: {int(diff.sum())} of {diff.size} differ, first at {list(at)}: got {g!r}, expected {w!r}'


def _within(name, got, want, lim):
    got, want, lim = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(lim, np.float64)
    if got.shape != want.shape:
        return f'{name}: shape {got.shape}, expected {want.shape}'
    err = np.abs(got - want)
    bad = ~(err <= lim)
    if not bad.any():
        return None
    at = tuple(int(i) for i in np.argwhere(bad)[0])
    return f'{name}: {int(bad.sum())} of {bad.size} beyond the bound, first at {list(at)}: got {got[at]!r}, expected {want[at]!r}, bound {np.broadcast_to(lim, err.shape)[at]:.3e}'


def _compare(kind, got, want, grid, dname, mname):
    """-> the first complaint, or None.  Each branch compares as the feature's own GPU test does."""
    if kind == 'vacuum_assign':                                   # test_gpu_sums.test_vacuum_assign
        vol, charge, volume = got
        wmap, s, cnt, mag = want
        return (_first('map', vol, wmap) or _first('volume', volume, float(cnt) * VV)
                or _within('charge', [charge], [s * VV], sum_bound_any_order(cnt, mag, VV)))
    if kind == 'bader_calc':                                      # soak_vs_oracle: ==
        return _first('maxima', got[0], want[0]) or _first('map', got[1], want[1])
    if kind == 'refine':
        return _first('map', got[0], want[0]) or (None if list(got[1]) == list(want[1]) else f'log: got {got[1]}, expected {want[1]}')
    if kind == 'bader_calc_refine':
        return (_first('maxima', got[0], want[0]) or _first('map', got[1], want[1])
                or (None if list(got[2]) == list(want[2]) else f'log: got {got[2]}, expected {want[2]}'))
    if kind == 'assign_to_atoms':                                 # test_gpu_parity: atom_assign ==, the swapped map ==
        return _first('bader_atoms', got[0], want[0]) or _first('bader_distance', got[1], want[1]) or _first('map', got[2], want[2])
    if kind == 'surface_distance':                                # test_gpu_sums.test_surface_distance, on the squared distances
        d2, edges = want
        if got is None:
            return None if edges == 0 else f'no edges found, expected {edges}'
        fin = np.isfinite(d2)
        g2 = np.asarray(got) ** 2
        msg = _first('atoms without an edge voxel', got[~fin], np.zeros(int((~fin).sum())))
        return msg or _within('squared distance', g2[fin], d2[fin], 1e-12 * np.abs(d2[fin]) + 1e-12 * np.abs(LAT).max() ** 2)
    if kind == 'charge_sum':                                      # test_gpu_sums.test_charge_sum
        s, cnt, mag = want
        return (_first('volume', got[1], cnt.astype(np.float64) * VV)
                or _within('charge', got[0], s * VV, sum_bound_any_order(cnt, mag, VV))
                or _first('labels nobody carries', got[0][cnt == 0], np.zeros(int((cnt == 0).sum()))))
    if kind in ('volume_mask', 'laplacian', 'laplacian_gather'):  # equal bits
        return _first('field', got[0], want[0], bits=True)
    if kind == 'volume_assign' or kind.startswith('voronoi'):
        return _first('map', got[0], want[0])
    if kind.startswith('weight_'):                                # test_gpu_weight.same
        vv = voxel_volume(grid)
        return _first('maxima', got[0], want[0]) or _first('charge', got[1], want[1] * vv, True) or _first('volume', got[2], want[2] * vv, True)
    if kind == 'moment_sum':                                      # test_gpu_multipole.check
        s, cnt, mag = want
        return (_first('volume', got[1], cnt.astype(np.float64) * VV) or _within('moments', got[0], s * VV, moment_bound(cnt, mag, VV))
                or _first('labels nobody carries', got[0][cnt == 0], np.zeros((int((cnt == 0).sum()), 10))))
    if kind == 'adjacency':                                       # test_adjacency_cpu.same
        return (_first('pairs', got[0], want[0]) or _first('facets', got[1], want[1]) or _first('saddle', got[2], want[2], True)
                or _first('saddle facet', got[3], want[3]))
    if kind == 'merge':                                           # test_gpu_merge.same, and the applied map
        w, wmap = want
        root, rnd, pers, rounds, converged, applied = got
        return (_first('root', root, w['root']) or _first('merge_round', rnd, w['merge_round'])
                or _first('merge_persistence', pers, w['merge_persistence'], True)
                or _first('rounds, converged', [rounds, int(converged)], [w['rounds'], int(w['converged'])])
                or _first('applied map', applied, wmap))
    if kind.startswith('critical'):                               # test_gpu_critical.same_points
        for name, g, w in zip(('counts', 'lin', 'masks', 'ring', 'bond'), got, want):
            msg = _first(name, g, w)
            if msg:
                return msg
        return None
    if kind == 'bond_graph':                                      # test_gpu_critical.same_bonds
        return (_first('pairs', got[0], want[0]) or _first('saddles', got[1], want[1]) or _first('rho_b', got[2], want[2], True)
                or _first('voxel', got[3], want[3]) or _first('same_basin', [got[4]], [want[4]]))
    if kind == 'basin_laplacian':                                 # test_gpu_laplacian.check_sums; the cell's zero where no voxel is left out
        s, cnt, mag = want
        lim = lap_sum_bound(cnt, mag)
        msg = (_first('volume', got[2], cnt.astype(np.float64) * VV) or _within('L', got[0], s * VV, lim)
               or _within('L_abs', got[1], mag * VV, lim))
        if msg is None and int(cnt.sum()) == int(np.prod(GRIDS[grid])):
            _, w6, _ = coefficients(LAT, GRIDS[grid])
            msg = _within('L summed over the cell', [np.sum(got[0])], [0.0], cell_sum_bound(density(grid, dname), w6) * VV)
        return msg
    if kind == 'point_properties':                                # test_gpu_laplacian: equal bits
        return _first('the ten values', got[0], want[0], True) or _first('laplacian', got[1], want[1], True)
    if kind.startswith('hirshfeld_charges'):                      # test_gpu_hirshfeld.check_sums
        s = want
        return (_within('charge', got[0], s['charge'] * VV, THS.sum_bound(s['count'], s['charge_mag'], VV))
                or _within('volume', got[1], s['volume'] * VV, THS.sum_bound(s['count'], s['volume_mag'], VV))
                or _within('the rest\'s charge', got[2][:1], [s['rest'][0] * VV], THS.sum_bound(s['rest'][1], s['rest_mag'], VV))
                or _first('the rest\'s volume', got[2][1:], [s['rest'][1] * VV]))
    if kind in ('promolecule', 'deformation', 'isa_residual'):    # test_gpu_hirshfeld / test_gpu_isa.same_bits
        return _first('field', got[0], want[0], bits=True)
    if kind.startswith('isa_charges'):                            # test_gpu_isa.test_isa_then_hirshfeld_then_isa, check_sums
        e, rows, tables, s = want
        history, got_tables, charge, volume, rest = got
        return (_first('history', history, rows.astype(np.float64) * (2.0 ** -e * VV)) or _first('tables', got_tables, tables, bits=True)
                or _within('charge', charge, s['charge'] * VV, THS.sum_bound(s['count'], s['charge_mag'], VV))
                or _within('volume', volume, s['volume'] * VV, THS.sum_bound(s['count'], s['volume_mag'], VV))
                or _within('the rest\'s charge', rest[:1], [s['rest'][0] * VV], THS.sum_bound(s['rest'][1], s['rest_mag'], VV))
                or _first('the rest\'s volume', rest[1:], [s['rest'][1] * VV]))
    if kind.startswith('nci_fields'):                             # test_gpu_nci: x in equal bits, s within S_REL
        if np.shape(got[0]) != GRIDS[grid] or np.shape(got[1]) != GRIDS[grid]:
            return f'fields of shape {np.shape(got[0])}, {np.shape(got[1])}'
        return TN.fields_difference(np.asarray(got[0]), np.asarray(got[1]), want[0], 'fields')
    if kind == 'nci_regions':
        cnt = want[0][1]
        if any(np.shape(a) != (cnt.size // 3, 3) for a in got):
            return f'sums of shape {np.shape(got[0])}, expected {(cnt.size // 3, 3)}'
        return TN.regions_difference(*got, want, 'regions')
    if kind == 'nci_histogram':
        return TN.histogram_difference(np.asarray(got[0]), want[0], 'histogram')
    if kind == 'nci_domains' or kind.startswith('regions'):       # test_gpu_regions.regions_call
        m, reg, seed, count, top, s1, s2, shares = got[:8]
        least = 2 if kind in ('nci_domains', 'regions', 'regions_global') else 1      # (below the level and on the field: one piece)
        if m != want['seeds'].size or want['seeds'].size < least or not np.array_equal(reg, want['reg']):
            return 'the map differs'
        try:
            TR.check_sums(kind, (seed, count, top, s1, s2), want['reg'], want['seeds'], want['rho'], VV)
        except AssertionError as e:
            return str(e)
        if not all(np.array_equal(g, w) for g, w in zip(shares, want['shares'])) or want['shares'][2].sum() < 50:
            return 'the shares differ'
        if kind == 'nci_domains':                                 # test_gpu_regions.check_domains: the classes' counts, the kinds
            return _first('count per class', got[8], want['class_count']) or _first('kind', got[9], want['kind'])
        return None
    if kind.startswith('isosurface'):                             # test_gpu_isosurface: first_difference, then sums_difference
        if np.shape(got[7]) != want.volume_by_label.shape:
            return f'volume_by_label of shape {np.shape(got[7])}, expected {want.volume_by_label.shape}'
        return TISO.first_difference(got, want, 'mesh') or TISO.sums_difference(got, want, 'mesh')
    if kind.startswith('mbis_charges'):                           # test_gpu_mbis.test_a_device_density_equals_the_host_one: same_bits
        for name, g, w in zip(('history', 'populations', 'widths', 'charge', 'volume', 'rest'), got, want):
            msg = _first(name, g, w, bits=True)
            if msg:
                return msg
        return None
    if kind in ('mbis_promolecule', 'mbis_residual'):             # test_gpu_mbis.same_bits
        return _first('field', got[0], want[0], bits=True)
    if kind.endswith(('_moments', '_moments_direct')):            # test_gpu_stockmom: bins and info ==, the moments in equal bits
        if got[1] != want[1]:
            return f'info: got {got[1]}, expected {want[1]}'
        return _first('bins', got[0], want[0]) or _first('moments', got[2], want[2], bits=True)
    if kind.startswith('dori_fields'):                            # test_gpu_dori.same_bits
        return _first('gamma', got[0], want[0], bits=True) or _first('x', got[1], want[1], bits=True)
    if kind.startswith('igm_fields'):                             # test_gpu_igm.same_bits
        return (_first('dg', got[0], want[0], bits=True) or _first('dg_inter', got[1], want[1], bits=True)
                or _first('x', got[2], want[2], bits=True))
    if kind == 'dori_regions':                                    # test_gpu_dori.dori_call (the NCI sums' comparison, key by key)
        cnt = want[0][1]
        if any(np.shape(a) != (cnt.size // 3, 3) for a in got):
            return f'sums of shape {np.shape(got[0])}, expected {(cnt.size // 3, 3)}'
        return TN.regions_difference(*got, want, 'regions')
    if kind == 'igm_regions':                                     # test_gpu_igm.igm_call
        cnt = want[0][1]
        if any(np.shape(a) != (cnt.size // 3, 3) for a in got):
            return f'sums of shape {np.shape(got[0])}, expected {(cnt.size // 3, 3)}'
        return TI.regions_difference(*got, want, 'regions')
    if kind in ('dori_domains', 'igm_domains'):                   # test_gpu_dori / test_gpu_igm: the domains against the components
        m, reg, seed, count, top, s1, s2, shares, value, cls = got[:10]
        if m != want['seeds'].size or want['seeds'].size < 1 or not np.array_equal(reg, want['reg']):
            return 'the map differs'
        if want['count'].sum() < 50:
            return f'the restated region holds {int(want["count"].sum())} voxels, too few to say anything'
        try:
            TR.check_sums(kind, (seed, count, top, s1, s2), want['reg'], want['seeds'], want['rho'], VV)
        except AssertionError as e:
            return str(e)
        if not all(np.array_equal(g, w) for g, w in zip(shares, want['shares'])):
            return 'the shares differ'
        msg = _first('value', value, want['value'], bits=True) or _first('kind', cls, want['kind'])
        if msg is None and kind == 'igm_domains':                 # (three class sums added: three times the bound of one)
            s, cnt, mag = want['integral']
            msg = _within('integral', got[10], s * VV, 3 * lap_sum_bound(cnt, mag))
        return msg
    if kind in ('dori_isosurface', 'igm_isosurface'):             # the mesh of isosurface.isosurface on the restated fields
        if want.triangles.shape[0] < 1:
            return 'the restated mesh is empty'
        return TISO.first_difference(got, want, 'mesh') or TISO.sums_difference(got, want, 'mesh')
    raise KeyError(kind)


def check(kind, got, inputs):
    """inputs = (grid, density name, map name).  -> None, or a message that names the kind and the first differing element"""
    grid, dname, mname = inputs
    msg = _compare(kind, got, expect(kind, grid, dname, mname), grid, dname, mname)
    return None if msg is None else f'{kind} on {grid} density {dname} map {mname}: {msg}'


def as_result(kind, want, grid):
    """an expectation in the form of the call's result: what check() reports on when handed another input's expectation"""
    if kind == 'vacuum_assign':
        return want[0], want[1] * VV, float(want[2]) * VV
    if kind == 'surface_distance':
        d2, edges = want
        out = np.zeros(d2.shape[0])
        out[np.isfinite(d2)] = d2[np.isfinite(d2)] ** .5
        return None if edges == 0 else out
    if kind == 'charge_sum':
        return want[0] * VV, want[1].astype(np.float64) * VV
    if kind.startswith('weight_'):
        return want[0], want[1] * voxel_volume(grid), want[2] * voxel_volume(grid)
    if kind == 'moment_sum':
        return want[0] * VV, want[1].astype(np.float64) * VV
    if kind == 'merge':
        w, wmap = want
        return w['root'], w['merge_round'], w['merge_persistence'], w['rounds'], w['converged'], wmap
    if kind == 'basin_laplacian':
        return want[0] * VV, want[2] * VV, want[1].astype(np.float64) * VV
    if kind.startswith('hirshfeld_charges'):
        return want['charge'] * VV, want['volume'] * VV, np.array([want['rest'][0] * VV, want['rest'][1] * VV]), None
    if kind.startswith('isa_charges'):
        e, rows, tables, s = want
        return (rows.astype(np.float64) * (2.0 ** -e * VV), tables, s['charge'] * VV, s['volume'] * VV,
                np.array([s['rest'][0] * VV, s['rest'][1] * VV]))
    if kind.startswith('nci_fields'):
        return want[0]['s'], want[0]['x']
    if kind == 'nci_regions':
        (s1, cnt, _), (s2, _, _) = want
        return cnt.reshape(-1, 3), (s1 * VV).reshape(-1, 3), (s2 * VV).reshape(-1, 3)
    if kind == 'nci_domains' or kind.startswith('regions'):
        return ((want['seeds'].size, want['reg'], want['seeds'], want['count'], want['top'], want['s1'] * VV, want['s2'] * VV, want['shares'])
                + ((want['class_count'], want['kind']) if kind == 'nci_domains' else ()))
    if kind.startswith('isosurface') or kind in ('dori_isosurface', 'igm_isosurface'):
        return want.vertices, want.colour, want.triangles, want.wrap, want.cells, want.area, want.volume, want.volume_by_label
    if kind in ('dori_regions', 'igm_regions'):
        (s1, cnt, _), (s2, _, _) = want
        return cnt.reshape(-1, 3), (s1 * VV).reshape(-1, 3), (s2 * VV).reshape(-1, 3)
    if kind in ('dori_domains', 'igm_domains'):
        return ((want['seeds'].size, want['reg'], want['seeds'], want['count'], want['top'], want['s1'] * VV, want['s2'] * VV, want['shares'],
                 want['value'], want['kind']) + ((want['integral'][0] * VV,) if kind == 'igm_domains' else ()))
    return want


# ---- the seeded walks ------------------------------------------------------------------------------------------------------------
EVENTS = ('shape', 'resident', 'mutate', 'fail')
FAILURES = ('density of another shape', 'label map of another shape', 'n < 1', 'non-float device dtype',
            'isa_iterate on a Hirshfeld setup', 'regions_shares without a labelling',
            'mbis_iterate on a Hirshfeld setup', 'stockholder_moments without a setup',
            'stockholder_moments under a rho_bound below max |rho|', 'mbis_iterate under a rho_bound below max |rho|')


def walk(seed, steps=180):
    """-> a list of steps, each a dict with 'op':

        call      kind, grid, dname, mname: one checked call
        enter / leave   dname: utils.resident() of that density of the current grid
        grid      grid: the next calls run there (in the order G1 -> G2 -> G3 -> G1, and by direct jumps), also inside resident()
        mutate    what ('density' | 'labels'), kind, dname, mname: outside resident(), the same host object goes into two calls
                  of `kind` with an in-place edit between them; both are checked
        fail      how (one of FAILURES), then kind, dname, mname of the checked call that follows the refused one

    Pure Python on the seed: the same list on every machine.  Every step is executable as it stands: no test leaves one out."""
    rng = random.Random(seed)
    kinds = list(KINDS)
    grid, inside, out = 'G1', None, []
    # the kinds whose result shows an edit of a corner block on every input (tests/test_history_cpu.py asserts it for the steps
    # drawn): the block lies in the tails, where the sparse results -- surfaces, saddles, bond points -- need not pass.
    # volume_mask shows a density edit only where the map carries MASK_LABEL in the block (the noise map does not);
    # isosurface_of_field takes its mesh from the other density's Laplacian and its shares from the map: the density is only kept.
    # The 0.7 / 0.8 level sets of the density lie at the atoms: a relabelled block in the tails moves no share of theirs on most
    # inputs (below the level, on the field and in the NCI region the block is inside: those kinds stay).
    # Every MBIS, moments, DORI and IGM kind shows both edits on every input (the block lies within the cutoffs of the atoms, in
    # the DORI region and, at the lower quartile, in the IGM region; igm_fields_pro and igm_fields_isa, whose two fields hardly
    # or not at all depend on the density, show it in x = sign(lambda2) rho): they all stay
    reads_d = [k for k in kinds if KINDS[k][0] and k not in ('voronoi', 'voronoi_full', 'adjacency', 'merge', 'critical_vacuum',
                                                             'critical_flood_vacuum', 'volume_mask', 'isosurface_of_field')]
    reads_m = [k for k in kinds if KINDS[k][1] and k not in ('surface_distance', 'merge', 'bond_graph', 'isosurface', 'isosurface_gather',
                                                             'regions', 'regions_global')]
    queue = []
    while len(out) < steps:
        r = rng.random()
        if not queue:
            queue = kinds[:]
            rng.shuffle(queue)
        pick = lambda: (rng.choice(densities(grid)), rng.choice(maps(grid)))
        if r < 0.64:
            d, m = pick()
            out.append({'op': 'call', 'kind': queue.pop(), 'grid': grid, 'dname': d, 'mname': m})
        elif r < 0.72:
            if inside is None:
                inside = rng.choice(('A', 'B'))
                out.append({'op': 'enter', 'grid': grid, 'dname': inside})
            else:
                out.append({'op': 'leave', 'grid': grid, 'dname': inside})
                inside = None
        elif r < 0.82:        # (also inside resident(): the pinned array then belongs to another grid until the walk returns)
            if rng.random() < 0.6:
                grid = ORDER[(ORDER.index(grid) + 1) % 3]
            else:
                grid = rng.choice([g for g in ORDER if g != grid])
            out.append({'op': 'grid', 'grid': grid})
        elif r < 0.91:
            if inside is not None:
                out.append({'op': 'leave', 'grid': grid, 'dname': inside})
                inside = None
            what = rng.choice(('density', 'labels'))
            d, m = pick()
            out.append({'op': 'mutate', 'what': what, 'kind': rng.choice(reads_d if what == 'density' else reads_m),
                        'grid': grid, 'dname': d, 'mname': m})
        else:
            d, m = pick()
            out.append({'op': 'fail', 'how': rng.choice(FAILURES), 'kind': queue.pop(), 'grid': grid, 'dname': d, 'mname': m})
    if inside is not None:
        out.append({'op': 'leave', 'grid': grid, 'dname': inside})
    return out


SEEDS = (11, 23, 47)


def edited(a, what):
    """the in-place edit of a walk's 'mutate' step, on a writable copy the test owns: a constant added to a corner block of a
    density, a corner block of a label map relabelled"""
    if what == 'density':
        a[:4, :3, :5] += 0.75
    else:
        a[:4, :3, :5] = 1
    return a
