"""Every public call after every other, on the default context: the result of a call must not depend on what ran before it.

Each feature's own GPU file pins its kernels from a context the test has just filled.  Which bytes a call reads is decided by
state no kernel sees -- the residency tokens of pybader_amd/utils.py and _lib.Context, the validity flags of the host code, the
buffers kept while the grid's shape stays, the shared scratch -- so here the calls run through the public functions in every
order, with and without utils.resident(), over host arrays and device tensors, across grid changes, in-place edits and refused
calls, and every result is compared with the expectation of tests/history_common.py (the feature's own restatement and bound).

The kinds (history_common.KINDS): the calls of the reference's pipeline, the weight method, moments, adjacency, merge, Voronoi,
critical points and bond graph, the Laplacian; Hirshfeld (hirshfeld_charges, _full, promolecule, deformation), ISA (isa_charges,
_direct, isa_residual), NCI (nci_fields, _gather, nci_regions, nci_histogram, nci_domains), isosurfaces (isosurface, _gather,
isosurface_of_field) and connected regions (regions, _below, _global, regions_of_field), which bring the flags "the result is the
resident density's" of the mesh and the labelling, the Hirshfeld setup that ISA replaces and hirshfeld._setup caches by key, and
the calls whose field "becomes the resident density" unless `density=` names it -- and the four analyses that lean hardest on
such state: MBIS (mbis_charges, _direct, mbis_promolecule, mbis_residual: a third kind of setup in the Hirshfeld block, a
ping-pong index of its parameters on the host, a setup-only call), the stockholder moments (hirshfeld_moments, _direct,
isa_moments, mbis_moments: "whichever setup is current", a counting pass once per Hirshfeld setup, bins in the block of
moment_sum), DORI (dori_fields, _gather, dori_regions, dori_domains, dori_isosurface) and IGM (igm_fields, _pro, _isa,
igm_regions, igm_domains, igm_isosurface), which write the block of the NCI sums and the shared scratch and hand their fields to
the labelling and the mesh.

test_every_call_after_every_other   every ordered pair (X, Y) of call kinds on G1, in five settings; one test id per X
test_seeded_walks                   three seeded walks of about 180 steps over the three grids
test_a_label_only_call_on_another_grid_inside_resident   the regression case of the defect these tests found
test_a_hirshfeld_setup_replaced_by_isa_and_dropped_with_the_shape_inside_resident   the key of the cached setup across both events
test_a_setup_only_mbis_call_on_another_grid_inside_resident   mbis_promolecule on another grid between calls on the pinned density
test_hirshfeld_moments_across_a_shared_block_a_replaced_setup_and_a_change_of_shape   BLK_M, the counting pass, the key

Wall time on an MI355X: MEASURED below."""
import ctypes as C
import warnings

import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:  # pragma: no cover
    torch = None

import history_common as H
from pybader_amd import (_lib, adjacency, critical, device, dori, hirshfeld, igm, isa, isosurface, laplacian, mbis, merge, multipole, nci,
                         regions, stockholder, thread_handlers, utils, voronoi, weight)
from test_isosurface_cpu import colour_field
from test_merge_cpu import maxima_of
from test_regions_cpu import sum_level

pytestmark = pytest.mark.gpu
MEASURED = ('this file alone in one process, 66 kinds, about 1000 calls per id: test_every_call_after_every_other 0.43 s to 1.67 s per id '
            '(vacuum_assign, the first id, 1.67 s with the shared restatements; isosurface_of_field 1.66 s, dori_isosurface 1.62 s, '
            'weight_other 1.39 s, weight_own 1.36 s, isosurface 1.36 s, mbis_charges_direct 1.29 s, isosurface_gather 1.21 s, dori_domains '
            '1.18 s, regions_of_field 1.15 s, regions_below 1.09 s, nci_domains 1.07 s; igm_isosurface 0.94 s, igm_domains 0.90 s, '
            'hirshfeld_moments_direct 0.75 s, mbis_charges 0.69 s, the other MBIS, moments, DORI and IGM ids 0.45 s to 0.55 s); '
            'test_seeded_walks 0.94 s, 0.62 s, 0.69 s for the seeds 11, 23, 47 (180 steps each); the five named cases 0.02 s or less '
            'each; 74 tests in 49.7 s, where the 47 kinds before took 26.2 s.  No id is beyond a few seconds: the iteration counts of '
            'the MBIS kinds are the ones asked for (5 iterations in calls of 2 + 2 + 1), nothing was lowered.  The '
            'slowest test of the four newest features\' own files in a run of theirs: '
            'test_gpu_mbis.py::test_iterates_equal_the_restatement[more_slots_m8-reduced], 1.57 s.')


def have_torch():
    return torch is not None and torch.cuda.is_available()


def host(a):
    if isinstance(a, device.DeviceArray):
        return a.to_host()
    if torch is not None and isinstance(a, torch.Tensor):
        return a.cpu().numpy()
    return a


class Runner:
    """makes one call of a kind through the public functions and returns its result in the form history_common.check takes.
    The host inputs are the memoised (read-only) arrays themselves: the same object goes into every call that names it, as a
    caller's would.  `dev`: float32 device tensors of the densities and int32 device tensors of the maps instead."""

    def __init__(self, dev=False):
        self.dev = dev
        self.tensors = {}

    def _tensor(self, key, make):
        if key not in self.tensors:
            self.tensors[key] = torch.as_tensor(make(), device='cuda')
        return self.tensors[key]

    def rho(self, grid, dname):
        if not self.dev:
            return H.density(grid, dname)
        assert dname.endswith('32')
        return self._tensor(('d', grid, dname), lambda: H.density(grid, dname).astype(np.float32))

    def lab(self, grid, mname):
        if not self.dev:
            return H.labels(grid, mname)
        return self._tensor(('m', grid, mname), lambda: H.labels(grid, mname).copy())

    def fresh(self, a):
        """a writable copy for the calls that update a map in place"""
        if torch is not None and isinstance(a, torch.Tensor):
            return a.clone()
        return np.array(a, copy=True)

    def call(self, kind, grid, dname, mname, rho=None, lab=None):
        shape = H.GRIDS[grid]
        mname = H.map_for(kind, mname)
        reads_d, reads_m = H.KINDS[kind]
        if rho is None:
            rho = self.rho(grid, dname)
        if lab is None and reads_m:
            lab = self.lab(grid, mname)
        n = H.n_of(grid, mname)
        dm, tg = H.geometry(grid)
        zeros = (lambda: None) if self.dev else (lambda: np.zeros(shape, np.int32))
        if kind == 'vacuum_assign':
            v, charge, volume = utils.vacuum_assign(rho, zeros(), H.VAC_TOL, rho, H.VV)
            return host(v), charge, volume
        if kind == 'bader_calc':
            bmax, v = thread_handlers.bader_calc('neargrid', rho, zeros(), dm, tg, 1)
            return bmax, host(v)
        if kind == 'refine':
            start = H.bader(grid, dname)['assign']
            v = torch.as_tensor(start.copy(), device='cuda') if self.dev else start.copy()
            thread_handlers.refine.last_log = None
            thread_handlers.refine('neargrid', H.REFINE_MODE, rho, v, dm, tg, 1)
            return host(v), [tuple(r) for r in (thread_handlers.refine.last_log or [])]
        if kind == 'bader_calc_refine':
            bmax, v = thread_handlers.bader_calc_refine('neargrid', 'neargrid', H.REFINE_MODE, rho, zeros(), dm, tg, 1)
            return bmax, host(v), [tuple(r) for r in thread_handlers.refine.last_log]
        if kind == 'assign_to_atoms':
            ba, bd, av = thread_handlers.assign_to_atoms(H.maxima_for(grid, mname), H.SITES['A'], H.LAT, lab, 1)
            return ba, bd, host(av)
        if kind == 'surface_distance':
            return thread_handlers.surface_distance(rho, lab, H.LAT, H.SITES8, 1)
        if kind == 'charge_sum':
            charge, volume = np.zeros(n), np.zeros(n)
            utils.charge_sum(charge, volume, H.VV, rho, lab)
            return charge, volume
        if kind == 'volume_mask':
            return (host(utils.volume_mask(lab, rho, H.MASK_LABEL)),)
        if kind == 'volume_assign':
            v = self.fresh(lab)
            utils.volume_assign(v, H.SWAP)
            return (host(v),)
        if kind.startswith('weight_'):
            q = rho if kind != 'weight_other' else self.rho(grid, H.other(dname))
            vac = None
            if kind == 'weight_vacuum':
                vac = H.vacuum_map(grid, dname)
                if self.dev:
                    vac = self._tensor(('v', grid, dname), lambda: H.vacuum_map(grid, dname).copy())
            return weight.weight_sum(rho, q, H.LAT, vac)
        if kind == 'moment_sum':
            return multipole.moment_sum(rho, lab, H.LAT, H.centres(grid, mname), H.VV)
        if kind == 'adjacency':
            a = adjacency.adjacency(rho, lab, H.LAT, n)
            return a.pairs, a.facets, a.saddle_density, a.saddle_facet
        if kind == 'merge':
            idx = maxima_of(np.asarray(host(rho), dtype=np.float64), host(lab), n)
            m = merge.merge_basins(rho, lab, H.LAT, np.stack(np.unravel_index(idx, shape), axis=1), H.MERGE_TOL)
            applied = m.apply(self.fresh(lab))
            return m.root, m.merge_round, m.merge_persistence, m.rounds, m.converged, host(applied)
        if kind.startswith('voronoi'):
            v, _ = voronoi.voronoi_assign(rho, H.LAT, H.sites_of(dname), H.VAC_TOL if kind.endswith('vacuum') else None,
                                          full_search='full' in kind)
            return (host(v),)
        if kind.startswith('critical'):
            cp = critical.critical_points(rho, H.VAC_TOL if kind.endswith('vacuum') else None, flood='flood' in kind)
            return cp.counts, cp.lin, cp.masks, cp.ring, cp.bond
        if kind == 'bond_graph':
            g = critical.bond_graph(rho, lab, n)
            return g.pairs, g.saddles, g.rho_b, g.voxel, g.same_basin
        if kind in ('laplacian', 'laplacian_gather'):
            return (host(laplacian.laplacian(rho, H.LAT, gather=kind.endswith('gather'))),)
        if kind == 'basin_laplacian':
            return laplacian.basin_laplacian(rho, lab, H.LAT, n, H.VV)
        if kind == 'point_properties':
            p = laplacian.point_properties(rho, H.LAT, H.point_list(grid))
            ten = np.column_stack([p.rho, p.gradient] + [p.hessian[:, i, j] for i, j in ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))])
            return np.ascontiguousarray(ten), p.laplacian
        if kind in ('hirshfeld_charges', 'hirshfeld_charges_full', 'promolecule', 'deformation'):
            atoms = (H.LAT, H.sites_of(dname), H.SPECIES, H.proatoms(H.atoms_of(dname)))
            if kind.startswith('hirshfeld_charges'):
                return hirshfeld.hirshfeld_charges(rho, *atoms, H.VV, full_search=kind.endswith('full'))
            return (host((hirshfeld.promolecule if kind == 'promolecule' else hirshfeld.deformation_density)(rho, *atoms)),)
        if kind.startswith('isa_charges'):
            r = isa.isa_charges(rho, H.LAT, H.sites_of(dname), H.VV, direct=kind.endswith('direct'), **H.ISA)
            return r.history, r.tables, r.charge, r.volume, r.rest
        if kind == 'isa_residual':
            return (host(isa.isa_residual(rho, H.LAT, H.sites_of(dname), H.isa_result(grid, dname))),)
        if kind.startswith('nci_fields'):
            s, x = nci.nci_fields(rho, H.LAT, gather=kind.endswith('gather'))
            return host(s), host(x)
        if kind == 'nci_regions':
            r = nci.nci_regions(rho, lab, H.LAT, n, H.VV, *H.NCI_CUTS)
            return r.count, r.charge, r.charge2
        if kind == 'nci_histogram':
            return (nci.nci_histogram(rho, H.LAT, *H.NCI_EDGES),)
        if kind == 'nci_domains':
            d = nci.nci_domains(rho, H.LAT, lab, n, H.VV, *H.NCI_CUTS)
            return d.m, host(d.labels), d.seed, d.size, d.top, d.total, d.total2, d.shares, d.count, d.kind
        if kind.startswith('isosurface'):
            if kind == 'isosurface_of_field':       # (the field stays a host array in every setting: the scratch upload is the route)
                m = isosurface.isosurface(H.field_of(grid, dname), H.LAT, H.FIELD_LEVEL, colour=colour_field(shape), volumes=lab, n=n,
                                          density=rho)
            else:
                m = isosurface.isosurface(rho, H.LAT, H.iso_level(grid, dname), colour=colour_field(shape), volumes=lab, n=n,
                                          gather=kind.endswith('gather'))
            return m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label
        if kind.startswith('regions'):
            if kind == 'regions_of_field':
                r = regions.connected_regions(H.field_of(grid, dname), H.FIELD_LEVEL, density=rho, voxel_volume=H.VV, volumes=lab, n=n)
            else:
                r = regions.connected_regions(rho, sum_level(H.density(grid, dname)), below=kind.endswith('below'), voxel_volume=H.VV,
                                              volumes=lab, n=n, global_route=kind.endswith('global'))
            return r.m, host(r.labels), r.seed, r.count, r.top, r.charge, r.charge2, r.shares
        if kind.startswith('mbis_'):
            sites = H.sites_of(dname)
            with warnings.catch_warnings():          # (r_cut = 2.5 truncates the model's tails: mbis_charges says so)
                warnings.simplefilter('ignore', RuntimeWarning)
                if kind.startswith('mbis_charges'):
                    r = mbis.mbis_charges(rho, H.LAT, sites, H.VV, shells=H.MBIS_SHELLS, direct=kind.endswith('direct'), **H.MBIS)
                    return r.history, r.populations, r.widths, r.charge, r.volume, r.rest
                if kind == 'mbis_promolecule':       # (the shells of the atoms' own density; `rho` gives the shape and the side only)
                    return (host(mbis.mbis_promolecule(rho, H.LAT, sites, H.mbis_result(grid, H.atoms_of(dname)))),)
                if kind == 'mbis_residual':
                    return (host(mbis.mbis_residual(rho, H.LAT, sites, H.mbis_result(grid, dname))),)
                m = stockholder.mbis_moments(rho, H.LAT, sites, H.mbis_result(grid, dname))
                return m.bins, m.info, m.moments
        if kind.startswith('hirshfeld_moments'):
            m = stockholder.hirshfeld_moments(rho, H.LAT, H.sites_of(dname), H.SPECIES, H.proatoms(H.atoms_of(dname)), H.VV,
                                              direct=kind.endswith('direct'))
            return m.bins, m.info, m.moments
        if kind == 'isa_moments':
            m = stockholder.isa_moments(rho, H.LAT, H.sites_of(dname), H.isa_result(grid, dname), H.VV)
            return m.bins, m.info, m.moments
        if kind.startswith('dori_'):
            if kind.startswith('dori_fields'):
                g, x = dori.dori_fields(rho, H.LAT, H.DORI_RHO_MIN, gather=kind.endswith('gather'))
                return host(g), host(x)
            if kind == 'dori_regions':
                r = dori.dori_regions(rho, lab, H.LAT, n, H.VV, *H.DORI_CUTS)
                return r.count, r.charge, r.charge2
            if kind == 'dori_domains':
                d = dori.dori_domains(rho, H.LAT, lab, n, H.VV, *H.DORI_CUTS)
                return d.m, host(d.labels), d.seed, d.count, d.top, d.charge, d.charge2, d.shares, d.value, d.kind
            m = dori.dori_isosurface(rho, H.LAT, *H.DORI_CUTS[:2])
            return m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label
        if kind.startswith('igm_'):
            atoms = dict(species=H.SPECIES, proatoms=H.proatoms(H.atoms_of(dname)))
            sites = H.sites_of(dname)
            if kind.startswith('igm_fields'):
                if kind.endswith('isa'):
                    atoms = dict(isa=H.isa_result(grid, dname))
                # (with x = sign(lambda2) rho: in mode 'pro' and on ISA tables it is the one output the density decides)
                dg, dgi, x = igm.igm_fields(rho, H.LAT, sites, H.FRAGMENTS, mode='pro' if kind.endswith('pro') else 'stockholder', **atoms)
                return host(dg), host(dgi), host(x)
            cut = H.igm_cut(grid, dname)
            if kind == 'igm_regions':
                r = igm.igm_regions(rho, lab, H.LAT, sites, H.FRAGMENTS, n, H.VV, cut, H.IGM_RHO_SPLIT, **atoms)
                return r.count, r.charge, r.integral
            if kind == 'igm_domains':
                d = igm.igm_domains(rho, H.LAT, sites, H.FRAGMENTS, lab, n, H.VV, cut, H.IGM_RHO_SPLIT, **atoms)
                return d.m, host(d.labels), d.seed, d.count, d.top, d.charge, d.charge2, d.shares, d.value, d.kind, d.integral
            m = igm.igm_isosurface(rho, H.LAT, sites, H.FRAGMENTS, cut, **atoms)
            return m.vertices, m.colour, m.triangles, m.wrap, m.cells, m.area, m.volume, m.volume_by_label
        raise KeyError(kind)

    def checked(self, kind, grid, dname, mname, **kw):
        """-> None, or history_common.check's message (an exception of the call is a message too: the walk goes on)"""
        try:
            got = self.call(kind, grid, dname, mname, **kw)
        except Exception as e:          # noqa: BLE001 -- reported with the pair that raised it
            if isinstance(e, _lib.BaderHipError) and getattr(e, 'code', 0) not in (_lib.XB_E_ARG, _lib.XB_E_STATE, _lib.XB_E_LIMIT):
                raise                   # an error of the device itself: nothing more is started on it
            return f'{kind} on {grid} density {dname} map {mname}: raised {type(e).__name__}: {e}'
        return H.check(kind, got, (grid, dname, H.map_for(kind, mname)))


@pytest.fixture(autouse=True)
def quiet(monkeypatch):
    H.cache_facet_areas(monkeypatch)
    was, thread_handlers.VERBOSE = thread_handlers.VERBOSE, False
    yield
    thread_handlers.VERBOSE = was
    ctx = _lib.default_context()
    ctx.pinned_density = ctx.resident_density = None
    ctx.drop_label_token()


# ---- the pair matrix -------------------------------------------------------------------------------------------------------------
def pairs_of(x, run, setting, first, second, pinned=None):
    """X on `first` then Y on `second` = (density name, map name), for every Y; a charge_sum on `second` runs before X, so that
    the map and density Y needs were the tracked ones before X ran (X = voronoi_assign or volume_assign rewrites the device
    labels: Y must then upload the earlier map again).  -> the failures"""
    bad = []

    def note(step, msg):
        if msg:
            bad.append(f'[{setting}] {x} then {step}: {msg}')

    def body():
        for y in H.KINDS:
            note(f'{y} (the charge_sum before {x})', run.checked('charge_sum', 'G1', *second))
            note(f'{y} ({x} itself)', run.checked(x, 'G1', *first))
            note(y, run.checked(y, 'G1', *second))
    if pinned is None:
        body()
    else:
        with utils.resident(pinned):
            body()
    return bad


@pytest.mark.parametrize('x', list(H.KINDS))
def test_every_call_after_every_other(x):
    """settings: 1 both calls on (A, bader), outside resident();  2 the same inside resident(A);  3 X on (B, atoms) and Y on
    (A, bader) inside resident(A): B is uploaded over the pinned array and Y must see A again;  4 both on a float32 device tensor
    of A and an int32 device tensor of the map (expectations from A32.astype(float64));  4r the same inside resident(tensor).

    X and Y run over every kind of history_common.KINDS, the Hirshfeld, ISA, NCI, isosurface, regions, MBIS, moments, DORI and IGM
    kinds included: a new analysis after another new one, a Hirshfeld, ISA or MBIS call next to calls that move the tokens, every
    setup of one kind after every setup of another, setting 3 for the calls whose field becomes the resident density, and device
    tensors for all of them.  The *_of_field kinds hand their field over as a host array in settings 4 and 4r too: it goes
    through the scratch upload beside the imported tensor."""
    run = Runner()
    bad = pairs_of(x, run, '1 plain', ('A', 'bader'), ('A', 'bader'))
    bad += pairs_of(x, run, '2 resident(A)', ('A', 'bader'), ('A', 'bader'), pinned=H.density('G1', 'A'))
    bad += pairs_of(x, run, '3 B over the pinned A', ('B', 'atoms'), ('A', 'bader'), pinned=H.density('G1', 'A'))
    if have_torch():
        dev = Runner(dev=True)
        bad += pairs_of(x, dev, '4 device tensors', ('A32', 'bader'), ('A32', 'bader'))
        bad += pairs_of(x, dev, '4r resident(device tensor)', ('A32', 'bader'), ('A32', 'bader'), pinned=dev.rho('G1', 'A32'))
    assert not bad, f'{len(bad)} failures, the first: ' + ' | '.join(bad[:4])
    if not have_torch():
        pytest.skip('settings 1 to 3 passed; torch sees no device for setting 4')


# ---- the seeded walks ------------------------------------------------------------------------------------------------------------
def refused(ctx, how, grid, run):
    """one call that the host refuses (the refusals the features' own error tests make).  Nothing reaches a kernel, except in the
    two refusals under a rho_bound below max |rho|: there the pass runs, finds voxels beyond the bound and the call returns
    XB_E_ARG -- an error return, with BLK_M or the MBIS scratch written, which the checked call after it must survive"""
    rho, lab = H.density(grid, 'A'), H.labels(grid, 'atoms')
    small = np.zeros((3, 3, 3))
    if how == 'density of another shape':
        with pytest.raises(ValueError):
            weight.weight_sum(rho, small, H.LAT)
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.weight_sum(H.alpha(grid), H.voxel_volume(grid), small)
        assert e.value.code == _lib.XB_E_ARG
    elif how == 'label map of another shape':
        with pytest.raises(ValueError):
            critical.bond_graph(rho, small.astype(np.int32), 2)
        with pytest.raises(ValueError):
            laplacian.basin_laplacian(rho, small.astype(np.int32), H.LAT, 2, H.VV)
    elif how == 'n < 1':
        laplacian.laplacian(rho, H.LAT)             # (a density and a map are there: the refusal is the argument's)
        utils.ensure_labels(ctx, lab)
        for call in (lambda: ctx.laplacian_sum(H.LAT, 0, H.VV), lambda: ctx.critical_bonds(0)):
            with pytest.raises(_lib.BaderHipError) as e:
                call()
            assert e.value.code in (_lib.XB_E_ARG, _lib.XB_E_STATE)
    elif how == 'non-float device dtype':
        ints = device.DeviceArray(ctx, H.GRIDS[grid], np.int32)
        with pytest.raises(_lib.BaderHipError) as e:
            critical.critical_points(ints)
        assert e.value.code == _lib.XB_E_ARG
    elif how == 'isa_iterate on a Hirshfeld setup':
        hirshfeld.promolecule(rho, H.LAT, H.SITES['A'], H.SPECIES, H.proatoms('A'))      # (a Hirshfeld setup is no ISA setup)
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.isa_iterate(1)
        assert e.value.code == _lib.XB_E_STATE
    elif how == 'regions_shares without a labelling':
        with pytest.raises(_lib.BaderHipError) as e:                # (connected_regions and nci_domains release theirs on return)
            ctx.regions_shares(H.n_of(grid, 'atoms'))
        assert e.value.code == _lib.XB_E_STATE
    elif how == 'mbis_iterate on a Hirshfeld setup':
        hirshfeld.promolecule(rho, H.LAT, H.SITES['A'], H.SPECIES, H.proatoms('A'))      # (a Hirshfeld setup is no MBIS setup)
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.mbis_iterate(1)
        assert e.value.code == _lib.XB_E_STATE
    elif how == 'stockholder_moments without a setup':
        ctx.hirshfeld_release()
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.stockholder_moments(1.0)
        assert e.value.code == _lib.XB_E_STATE
    elif how == 'stockholder_moments under a rho_bound below max |rho|':
        # (the kernel runs, counts the voxels beyond the bound and the call refuses: BLK_M is written, the output is not)
        stockholder.hirshfeld_moments(rho, H.LAT, H.SITES['A'], H.SPECIES, H.proatoms('A'), H.VV)
        low = 0.5 * float(np.abs(rho).max())
        out = np.full((3, 12), -77, np.int64)
        info, st = (C.c_int64 * 8)(), (C.c_int64 * 3)()
        assert ctx.lib.xb_stockholder_moments(ctx.h, low, 0, out.ctypes.data_as(_lib._pi64), info, st) == _lib.XB_E_ARG
        assert (out == -77).all() and info[7] == int((np.abs(rho) > low).sum()) > 0
        with pytest.raises(_lib.BaderHipError) as e:
            ctx.stockholder_moments(low)
        assert e.value.code == _lib.XB_E_ARG
    elif how == 'mbis_iterate under a rho_bound below max |rho|':
        # (the pass runs into the MBIS scratch and the call refuses: the parameters stay)
        utils.ensure_density(ctx, rho)
        N0, s0 = mbis.default_initial(H.MBIS_SHELLS)
        ctx.mbis_setup(H.LAT, H.SITES['A'], np.full(3, H.MBIS['r_cut']), H.MBIS_SHELLS, mbis.exp_table(H.MBIS_KNOTS, H.MBIS_X_MAX),
                       H.MBIS_KNOTS, N0, s0, 0.5 * float(np.abs(rho).max()), H.VV)
        for iters in (1, 2):
            with pytest.raises(_lib.BaderHipError) as e:
                ctx.mbis_iterate(iters)
            assert e.value.code == _lib.XB_E_ARG
            N, sg, _ = ctx.mbis_params()
            assert np.array_equal(N.view(np.uint64), N0.view(np.uint64)) and np.array_equal(sg.view(np.uint64), s0.view(np.uint64))
    else:
        raise KeyError(how)


def release_all(ctx):
    ctx.adjacency_release()
    ctx.merge_release()
    ctx.critical_release()
    ctx.weight_release()
    ctx.isosurface_release()
    ctx.regions_release()
    ctx.hirshfeld_release()


@pytest.mark.parametrize('seed', H.SEEDS)
def test_seeded_walks(seed):
    """history_common.walk(seed): checked calls on random inputs of the current grid, resident() entered and left, the grid changed
    (also inside resident()), a host array edited in place between two calls on the same object, refused calls.

    Memory: a change to a grid of another voxel count frees everything the context holds for the grid, so right after set_grid
    memory_stats() must equal what it was after the first set_grid of that shape -- at every return to a shape, and at the end
    after the release calls and a last return.  (Between those points the table, the edge buffers and the per-label sum
    buffers grow with use and have no release call of their own: the releases can only be shown not to raise the figure.)"""
    ctx = _lib.default_context()
    run = Runner()
    steps = H.walk(seed)
    bad, base, state = [], {}, {'cm': None, 'waits': ctx.host_waits()}

    def note(k, step, msg):
        if msg:
            bad.append(f'seed {seed} step {k} {step}: {msg}')
        waits, mem = ctx.host_waits(), ctx.memory_stats()
        assert isinstance(waits, int) and waits >= state['waits'], (k, waits)
        assert all(isinstance(v, int) and 0 <= v < 1 << 40 for v in mem) and mem[0] >= mem[1] + mem[2], (k, mem)
        state['waits'] = waits

    def enter_grid(k, grid):
        ctx.set_grid(H.GRIDS[grid], *H.geometry(grid))
        mem = ctx.memory_stats()
        if base.setdefault(grid, mem) != mem:
            bad.append(f'seed {seed} step {k}: memory_stats after returning to {grid} is {mem}, after the first set_grid it was {base[grid]}')

    def leave():
        if state['cm'] is not None:
            state['cm'].__exit__(None, None, None)
            state['cm'] = None

    ctx.set_grid((3, 3, 3), np.zeros(27), np.zeros(9))       # (whatever earlier tests left on the default context goes)
    grid = 'G1'
    enter_grid(-1, grid)
    try:
        for k, s in enumerate(steps):
            op = s['op']
            if op == 'call':
                note(k, s, run.checked(s['kind'], s['grid'], s['dname'], s['mname']))
            elif op == 'enter':
                state['cm'] = utils.resident(H.density(s['grid'], s['dname']))
                state['cm'].__enter__()
            elif op == 'leave':
                leave()
            elif op == 'grid':
                grid = s['grid']
                enter_grid(k, grid)
            elif op == 'mutate':
                assert state['cm'] is None
                d, m = s['dname'], H.map_for(s['kind'], s['mname'])
                kw = {'rho': H.density(grid, d).copy()} if s['what'] == 'density' else {'lab': H.labels(grid, m).copy()}
                note(k, s, run.checked(s['kind'], grid, d, m, **kw))
                H.edited(next(iter(kw.values())), s['what'])
                if s['what'] == 'density':
                    d += '+'
                else:
                    m += '+'
                note(k, f'{s} after the edit', run.checked(s['kind'], grid, d, m, **kw))
            elif op == 'fail':
                refused(ctx, s['how'], grid, run)
                note(k, s, run.checked(s['kind'], grid, s['dname'], s['mname']))
            else:
                raise KeyError(op)
            assert s.get('grid', grid) == grid
    finally:
        leave()
    before = ctx.memory_stats()
    release_all(ctx)
    after = ctx.memory_stats()
    assert after[0] <= before[0] and after[2] <= before[2], (before, after)
    away = 'G2' if grid != 'G2' else 'G3'
    enter_grid(len(steps), away)
    release_all(ctx)
    enter_grid(len(steps) + 1, grid)
    release_all(ctx)
    assert ctx.memory_stats() == base[grid], (ctx.memory_stats(), base[grid])
    assert not bad, f'{len(bad)} failures, the first: ' + ' | '.join(bad[:4])


# ---- the regression case -----------------------------------------------------------------------------------------------------------
def test_a_label_only_call_on_another_grid_inside_resident():
    """inside resident(A of G1): a call on A, then a call that reads no density on a grid of another shape (volume_assign of a G2
    map; voronoi_assign without a tolerance), then the call on A again.  The change of shape drops the device density, so the
    second call must upload A again: Context.set_grid used to keep the `resident_density` token across the change, and the call
    ran on a density buffer nobody had filled (or was refused with "no density on this grid yet")."""
    run = Runner()
    rho = H.density('G1', 'A')
    for between in ('volume_assign', 'voronoi', 'assign_to_atoms'):
        for kind in ('charge_sum', 'critical', 'volume_mask', 'laplacian'):
            with utils.resident(rho):
                assert run.checked(kind, 'G1', 'A', 'bader') is None
                assert run.checked(between, 'G2', 'A', 'atoms') is None
                msg = run.checked(kind, 'G1', 'A', 'bader')
                assert msg is None, f'{kind}, {between} on G2, {kind}: {msg}'


def test_a_hirshfeld_setup_replaced_by_isa_and_dropped_with_the_shape_inside_resident():
    """inside resident(A of G1): hirshfeld_charges, isa_charges (which IS the context's Hirshfeld setup and replaces it),
    hirshfeld_charges again (hirshfeld._setup must not take the ISA tables for its own: Context.isa_setup clears the key it
    remembers), the promolecule on G2 (the change of shape drops the setup and the key), then hirshfeld_charges on G1 once more: the
    setup is made again on a grid that holds no density until the call uploads the pinned one."""
    run = Runner()
    with utils.resident(H.density('G1', 'A')):
        for kind, grid in (('hirshfeld_charges', 'G1'), ('isa_charges', 'G1'), ('hirshfeld_charges', 'G1'), ('promolecule', 'G2'),
                           ('hirshfeld_charges', 'G1')):
            msg = run.checked(kind, grid, 'A', 'atoms')
            assert msg is None, msg


def test_a_setup_only_mbis_call_on_another_grid_inside_resident():
    """inside resident(A of G1): charge_sum on A, then mbis_promolecule on G2 -- it builds a setup and reads the grid's shape
    without uploading a density, as the label-only calls above read no density --, then charge_sum on G1 again: the change of
    shape dropped the device density, so A must be uploaded again.  The promolecule itself is checked too, and the same with a
    call in between that leans on the setup (hirshfeld_moments) in the place of charge_sum."""
    run = Runner()
    _lib.default_context().set_grid(H.GRIDS['G1'], *H.geometry('G1'))
    with utils.resident(H.density('G1', 'A')):          # (the setup-only call as the first call inside the block)
        msg = run.checked('mbis_promolecule', 'G2', 'A', 'atoms') or run.checked('charge_sum', 'G1', 'A', 'bader')
        assert msg is None, f'mbis_promolecule on G2, charge_sum: {msg}'
    with utils.resident(H.density('G1', 'A')):
        for kind in ('charge_sum', 'hirshfeld_moments', 'mbis_residual'):
            assert run.checked(kind, 'G1', 'A', 'bader') is None
            msg = run.checked('mbis_promolecule', 'G2', 'A', 'atoms')
            assert msg is None, msg
            msg = run.checked(kind, 'G1', 'A', 'bader')
            assert msg is None, f'{kind}, mbis_promolecule on G2, {kind}: {msg}'


def test_hirshfeld_moments_across_a_shared_block_a_replaced_setup_and_a_change_of_shape():
    """hirshfeld_moments, moment_sum (the owner of BLK_M, where the moments' bins go), hirshfeld_moments (the counting pass ran
    once for this setup: sm_cmax is kept), isa_charges (which replaces the setup: hirshfeld._setup's key and sm_cmax must go),
    hirshfeld_moments, a change to G2 and back (the setup and the key go with the shape), hirshfeld_moments: every result
    checked.  Outside resident() and inside it."""
    run = Runner()
    ctx = _lib.default_context()

    def sequence(where):
        for kind in ('hirshfeld_moments', 'moment_sum', 'hirshfeld_moments', 'isa_charges', 'hirshfeld_moments'):
            msg = run.checked(kind, 'G1', 'A', 'atoms')
            assert msg is None, f'{where}: {msg}'
        ctx.set_grid(H.GRIDS['G2'], *H.geometry('G2'))
        ctx.set_grid(H.GRIDS['G1'], *H.geometry('G1'))
        msg = run.checked('hirshfeld_moments', 'G1', 'A', 'atoms')
        assert msg is None, f'{where}, after G2 and back: {msg}'

    sequence('plain')
    with utils.resident(H.density('G1', 'A')):
        sequence('resident(A)')


# ---- the label token at the level of the Context -----------------------------------------------------------------------------------
def test_every_label_writer_of_the_context_drops_the_token():
    """inside resident(A): charge_sum on a map (which leaves that host array tracked as the device labels), then a Context
    method that rewrites the device labels, then charge_sum on the same array again: it must be uploaded again.  Through the
    public functions a forgotten drop_label_token() in such a method cannot show, because utils.fetch_labels releases the token
    itself before it tracks the result; callers of the Context (pybader_amd/slab.py, the tests) have only the method's own."""
    ctx = _lib.default_context()
    run = Runner()
    rho, lab = H.density('G1', 'A'), H.labels('G1', 'bader')
    other = H.labels('G1', 'noise')
    writers = {
        'voronoi_assign': lambda: ctx.voronoi_assign(H.LAT, H.SITES['B']),
        'volume_assign': lambda: ctx.volume_assign(H.SWAP),
        'vacuum_assign': lambda: ctx.vacuum_assign(H.VAC_TOL, H.VV),
        'upload_labels': lambda: ctx.upload_labels(other),
        'assign': lambda: ctx.assign('neargrid'),
        'refine': lambda: (ctx.upload_labels(H.bader('G1', 'B')['assign']), ctx.refine(*H.REFINE_MODE)),
        'assign_refine': lambda: ctx.assign_refine('neargrid', *H.REFINE_MODE),
    }
    with utils.resident(rho):
        for name, write in writers.items():
            ctx.set_grid(H.GRIDS['G1'], *H.geometry('G1'))
            assert run.checked('charge_sum', 'G1', 'A', 'bader') is None
            assert utils.labels_resident(ctx, lab), 'the map is the tracked one'
            write()
            assert not utils.labels_resident(ctx, lab), f'Context.{name} left the label token in place'
            msg = run.checked('charge_sum', 'G1', 'A', 'bader')
            assert msg is None, f'charge_sum, Context.{name}, charge_sum: {msg}'
