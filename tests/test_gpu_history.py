"""Every public call after every other, on the default context: the result of a call must not depend on what ran before it.

Each feature's own GPU file pins its kernels from a context the test has just filled.  Which bytes a call reads is decided by
state no kernel sees -- the residency tokens of pybader_amd/utils.py and _lib.Context, the validity flags of the host code, the
buffers kept while the grid's shape stays, the shared scratch -- so here the calls run through the public functions in every
order, with and without utils.resident(), over host arrays and device tensors, across grid changes, in-place edits and refused
calls, and every result is compared with the expectation of tests/history_common.py (the feature's own restatement and bound).

test_every_call_after_every_other   every ordered pair (X, Y) of call kinds on G1, in five settings; one test id per X
test_seeded_walks                   three seeded walks of about 80 steps over the three grids
test_a_label_only_call_on_another_grid_inside_resident   the regression case of the defect these tests found

Wall time on an MI355X, the whole suite in one process: MEASURED below."""
import numpy as np
import pytest
try:
    import torch          # before anything loads libbader_hip.so (tests/conftest.py says why)
except Exception:  # pragma: no cover
    torch = None

import history_common as H
from pybader_amd import _lib, adjacency, critical, device, laplacian, merge, multipole, thread_handlers, utils, voronoi, weight
from test_merge_cpu import maxima_of

pytestmark = pytest.mark.gpu
MEASURED = ('test_every_call_after_every_other: 0.20 s to 0.62 s per id (weight_other, weight_own 0.6 s; vacuum_assign, the first id, '
            '0.47 s with the shared restatements); test_seeded_walks: 0.30 s to 0.34 s per seed; the two named cases below 0.05 s.  '
            'The slowest test of the features\' own files in the same run: test_gpu_adjacency.py::test_adjacency[shape1], 2.15 s.')


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
    of A and an int32 device tensor of the map (expectations from A32.astype(float64));  4r the same inside resident(tensor)"""
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
    """one call that the host refuses (the refusals the features' own test_error_codes tests make: nothing reaches a kernel)"""
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
    else:
        ints = device.DeviceArray(ctx, H.GRIDS[grid], np.int32)
        with pytest.raises(_lib.BaderHipError) as e:
            critical.critical_points(ints)
        assert e.value.code == _lib.XB_E_ARG


def release_all(ctx):
    ctx.adjacency_release()
    ctx.merge_release()
    ctx.critical_release()
    ctx.weight_release()


@pytest.mark.parametrize('seed', H.SEEDS)
def test_seeded_walks(seed):
    """history_common.walk(seed): checked calls on random inputs of the current grid, resident() entered and left, the grid changed
    (also inside resident()), a host array edited in place between two calls on the same object, refused calls.

    Memory: a change to a grid of another voxel count frees everything the context holds for the grid, so right after set_grid
    memory_stats() must equal what it was after the first set_grid of that shape -- at every return to a shape, and at the end
    after the four release calls and a last return.  (Between those points the table, the edge buffers and the per-label sum
    buffers grow with use and have no release call of their own: the four releases can only be shown not to raise the figure.)"""
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
