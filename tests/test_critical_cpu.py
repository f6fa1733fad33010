"""The host side of the critical points (pybader_amd/critical.py, xb_critical_lut) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 17 that tests/test_gpu_critical.py compares the kernels with, record by
record with ==.

`components` counts the connected components of a mask by flood fill over the link graph, `components_union_find` again by
union-find, and `euler` gives V - E + F of the induced subcomplex: three statements of one fact, checked against each other on
all 16 384 masks.  `reference_points` forms the lower masks with np.roll (the wrap of the definition) and classifies them
through the restated table; `reference_bonds` walks the bond voxels one by one in Python.  The invariant no restatement error
can fake: minima - sum ring + sum bond - maxima == 0 on every field whose axes all have four voxels."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, critical, synth
from pybader_amd.adjacency import key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 0x3fff
OFFSETS = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]
OFFSETS += [tuple(-x for x in d) for d in OFFSETS]
ADJACENT = [[tuple(q - p for p, q in zip(a, b)) in OFFSETS for b in OFFSETS] for a in OFFSETS]
EDGES = [(a, b) for a in range(14) for b in range(a + 1, 14) if ADJACENT[a][b]]
TRIANGLES = [(a, b, c) for a, b in EDGES for c in range(b + 1, 14) if ADJACENT[a][c] and ADJACENT[b][c]]


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def component_list(m):
    """the connected components of the set bits of m, each a mask, by flood fill"""
    out, rem = [], m
    while rem:
        comp = rem & -rem
        while True:
            grown = comp
            for a in range(14):
                if comp >> a & 1:
                    for b in range(14):
                        if ADJACENT[a][b] and m >> b & 1:
                            grown |= 1 << b
            if grown == comp:
                break
            comp = grown
        out.append(comp)
        rem &= ~comp
    return out


def components(m):
    return len(component_list(m))


def components_union_find(m):
    parent = list(range(14))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in EDGES:
        if m >> a & 1 and m >> b & 1:
            parent[find(a)] = find(b)
    return len({find(a) for a in range(14) if m >> a & 1})


def euler(m):
    """V - E + F of the subcomplex of the link that the set bits of m induce"""
    v = bin(m).count('1')
    e = sum(1 for a, b in EDGES if m >> a & 1 and m >> b & 1)
    f = sum(1 for a, b, c in TRIANGLES if m >> a & 1 and m >> b & 1 and m >> c & 1)
    return v - e + f


@functools.lru_cache(maxsize=None)
def reference_lut():
    """ring | bond << 4 per lower mask; 0 for the two extrema"""
    tab = np.zeros(1 << 14, np.uint8)
    for m in range(1, FULL):
        tab[m] = (components(m) - 1) | ((components(~m & FULL) - 1) << 4)
    tab.flags.writeable = False
    return tab


def lower_masks(rho):
    """L(v) for every voxel: bit k set iff the wrapped neighbour at OFFSETS[k] is below v in (key, lin) order"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    k = key(rho).reshape(rho.shape)
    lin = np.arange(rho.size, dtype=np.int64).reshape(rho.shape)
    low = np.zeros(rho.shape, np.uint16)
    for bit, d in enumerate(OFFSETS):
        ku = np.roll(k, tuple(-x for x in d), axis=(0, 1, 2))      # ku[v] = k[v + d], wrapped
        lu = np.roll(lin, tuple(-x for x in d), axis=(0, 1, 2))
        below = (ku < k) | ((ku == k) & (lu < lin))
        low |= (below.astype(np.uint16) << np.uint16(bit))
    return low


def reference_points(rho, vacuum_tol=None):
    """-> (counts int64[6], lin int64[P] ascending, L uint16[P], ring uint8[P], bond uint8[P])"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    low = lower_masks(rho).reshape(-1)
    code = reference_lut()[low]
    crit = (low == 0) | (low == FULL) | (code != 0)
    if vacuum_tol is not None:
        crit &= ~(rho.reshape(-1) <= vacuum_tol)
    lin = np.flatnonzero(crit).astype(np.int64)
    L, ring, bond = low[lin], code[lin] & 15, code[lin] >> 4
    counts = np.array([(L == FULL).sum(), (bond > 0).sum(), bond.sum(), (ring > 0).sum(), ring.sum(), (L == 0).sum()], np.int64)
    return counts, lin, L, ring.astype(np.uint8), bond.astype(np.uint8)


def reference_bonds(rho, labels, n, vacuum_tol=None):
    """-> (pairs int32[P, 2], saddles int64[P], rho_b f64[P], voxel int64[P], same_basin), one bond voxel at a time"""
    rho = np.ascontiguousarray(rho, dtype=np.float64)
    shape = rho.shape
    flat, lab = rho.reshape(-1), np.asarray(labels).reshape(-1)
    kflat = key(flat)
    _, lin, low, _, bond = reference_points(rho, vacuum_tol)
    found, same = {}, 0
    for v, L in zip(lin[bond > 0].tolist(), low[bond > 0].tolist()):
        p = np.unravel_index(v, shape)
        basins = set()
        for comp in component_list(~L & FULL):
            nb = [int(np.ravel_multi_index(tuple((p[j] + OFFSETS[k][j]) % shape[j] for j in range(3)), shape))
                  for k in range(14) if comp >> k & 1]
            top = max(nb, key=lambda u: (int(kflat[u]), u))
            if 0 <= int(lab[top]) < n:
                basins.add(int(lab[top]))
        if len(basins) == 1:
            same += 1
        for a in basins:
            for b in basins:
                if a < b:
                    e = found.setdefault((a, b), [0, None])
                    e[0] += 1
                    cand = (-int(kflat[v]), v)
                    if e[1] is None or cand < e[1]:
                        e[1] = cand
    pairs = sorted(found)
    return (np.array(pairs, np.int32).reshape(-1, 2), np.array([found[p][0] for p in pairs], np.int64),
            np.array([flat[found[p][1][1]] for p in pairs], np.float64), np.array([found[p][1][1] for p in pairs], np.int64), same)


def euler_sum(counts):
    return int(counts[5] - counts[4] + counts[2] - counts[0])


# ---- inputs (shared with tests/test_gpu_critical.py) ----------------------------------------------------------------------------
# one wide Gaussian (sigma a quarter of the cell: its tail never underflows to the flat background, so no plateau arises)
ONE_ATOM = np.array([[0.2310, 0.2690, 0.2470, 1.5, 7.5]])
# eight atoms on a 2 x 2 x 2 arrangement: the positions of synth.ATOMS8 pulled halfway towards their regular sites (1/4 or 3/4 on
# every axis) and shifted off the grid planes, one width for all, the amplitudes of ATOMS8 -- every atom has six nearest
# neighbours, two periodic images of each of three atoms
_SITES = np.rint(synth.ATOMS8[:, :3] * 4) / 4
ATOMS_2X2X2 = np.concatenate([_SITES + 0.5 * (synth.ATOMS8[:, :3] - _SITES) + 0.013, np.full((8, 1), 0.8), synth.ATOMS8[:, 4:]], axis=1)
TRIC24 = np.array([[6.0, 0.0, 0.0], [1.5, 5.5, 0.0], [0.7, 1.1, 6.2]])


def _spike(shape):
    """+0.0 and -0.0 in a checkerboard of the linear index's parity bits, and one spike: only key() tells the zeros apart"""
    n = int(np.prod(shape))
    a = np.where((np.arange(n) * 2654435761 >> 7) & 1, -0.0, 0.0).reshape(shape)
    a[2, 3, 1] = 1.0
    return a


@functools.lru_cache(maxsize=None)
def case(name):
    """one input of the GPU tests, made once and never written"""
    make = {
        'gauss8': lambda: synth.synth_density((8, 8, 8), synth.CUBIC6, ONE_ATOM),
        'gauss12x10x16': lambda: synth.synth_density((12, 10, 16), synth.CUBIC6, ONE_ATOM),
        'constant': lambda: np.full((5, 6, 7), 0.25),
        'atoms8_24': lambda: synth.synth_density((24, 24, 24)),
        'grid2x2x2': lambda: synth.synth_density((24, 24, 24), synth.CUBIC6, ATOMS_2X2X2),
        'synth8': lambda: synth.synth_density((8, 8, 8)),
        'synth40x36x44': lambda: synth.synth_density((40, 36, 44)),
        'tric24': lambda: synth.synth_density((24, 24, 24), TRIC24),
        'rough': lambda: synth.rough_density((24, 20, 28), noise=0.4),
        'plateau': lambda: synth.rough_density((24, 20, 28), noise=0.4, quantum=0.125),
        'noise20x9x33': lambda: synth.hash_noise((20, 9, 33), 3),
        'noise3': lambda: synth.hash_noise((3, 3, 3), 4),
        'noise2': lambda: synth.hash_noise((2, 2, 2), 5),
        'noise1x2x9': lambda: synth.hash_noise((1, 2, 9), 6),
        'zeros_spike': lambda: _spike((6, 7, 5)),
    }[name]
    a = np.ascontiguousarray(make(), dtype=np.float64)
    a.flags.writeable = False
    return a


GPU_CASES = ['synth8', 'synth40x36x44', 'tric24', 'rough', 'plateau', 'constant', 'noise20x9x33', 'noise3', 'noise2', 'noise1x2x9',
             'zeros_spike']
VACUUM_CASE, VACUUM_TOL = 'rough', 0.2


@functools.lru_cache(maxsize=None)
def reference(name, vacuum_tol=None):
    out = reference_points(case(name), vacuum_tol)
    for a in out:
        a.flags.writeable = False
    return out


def noise_labels(shape, n=5, seed=11):
    """a label map from hash_noise: blobs of 4 x 4 x 4 voxels with labels -1 .. n (both ends count for nothing)"""
    coarse = tuple(-(-s // 4) for s in shape)
    lab = np.floor(synth.hash_noise(coarse, seed) * (n + 2)).astype(np.int32) - 1
    lab = np.repeat(np.repeat(np.repeat(lab, 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]]
    return np.ascontiguousarray(lab)


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
def test_the_link_is_a_triangulated_sphere():
    assert len(OFFSETS) == 14 and len(set(OFFSETS)) == 14 and len(EDGES) == 36 and len(TRIANGLES) == 24
    assert all(ADJACENT[a][b] == ADJACENT[b][a] for a in range(14) for b in range(14))
    assert sum(sum(row) for row in ADJACENT) == 72 and not any(ADJACENT[a][a] for a in range(14))
    assert 14 - len(EDGES) + len(TRIANGLES) == 2
    assert np.array_equal(critical.OFFSETS, np.array(OFFSETS))


def test_three_counts_of_the_components_agree_on_every_mask():
    bad = 0
    for m in range(1, FULL):
        c_low, c_up = components(m), components(~m & FULL)
        assert c_low == components_union_find(m)
        bad += euler(m) != c_low - (c_up - 1)      # Alexander duality on the sphere: chi(K) = b0(K) - (b0(complement) - 1)
    assert bad == 0
    assert max(components(m) for m in range(1 << 14)) == 6


def test_library_table_equals_the_restatement():
    """fails without the feature: the library has no xb_critical_lut"""
    from pybader_amd import build
    build.build_library()
    got = _lib.critical_lut()
    want = reference_lut()
    assert got.dtype == np.uint8 and got.shape == (16384,) and np.array_equal(got, want)
    assert got[0] == 0 and got[FULL] == 0 and (got != 0).sum() == (want != 0).sum() > 8000


@pytest.mark.parametrize('name', ['gauss8', 'gauss12x10x16', 'constant'])
def test_one_maximum_on_the_torus_has_three_bonds_three_rings_and_a_cage(name):
    counts, lin, L, ring, bond = reference_points(case(name))
    assert counts.tolist() == [1, 3, 3, 3, 3, 1], counts
    assert lin.size == 8 and np.all(np.diff(lin) > 0)


def test_eight_atoms_give_8_24_24_8():
    counts = reference('grid2x2x2')[0]
    assert counts.tolist() == [8, 24, 24, 24, 24, 8], counts


@pytest.mark.parametrize('name', sorted(set(GPU_CASES + ['atoms8_24', 'grid2x2x2', 'gauss8', 'gauss12x10x16'])))
def test_euler_identity_on_every_input_with_axes_of_four(name):
    rho = case(name)
    counts, lin, L, ring, bond = reference(name)
    print(name, rho.shape, counts.tolist(), 'max multiplicity', int(max(ring.max(initial=0), bond.max(initial=0))),
          'both', int(((ring > 0) & (bond > 0)).sum()))
    if min(rho.shape) >= 4:
        assert euler_sum(counts) == 0
    if min(rho.shape) >= 2:      # (on an axis of one voxel every voxel is its own neighbour twice, and those bits stay clear)
        assert counts[0] >= 1 and counts[5] >= 1     # a total order on a finite torus has a top and a bottom


def test_the_inputs_exercise_what_they_are_for():
    _, _, _, ring, bond = reference('rough')
    assert max(ring.max(), bond.max()) >= 3 and ((ring > 0) & (bond > 0)).any()
    rho = case('plateau')
    k = key(rho).reshape(rho.shape)
    assert any((np.roll(k, -1, axis=ax) == k).sum() > 1000 for ax in range(3)), 'plateaus: index ties decide'
    z = case('zeros_spike')
    assert (np.signbit(z) & (z == 0)).sum() > 20 and ((~np.signbit(z)) & (z == 0)).sum() > 20
    assert not np.array_equal(reference_points(z)[1], reference_points(np.abs(z))[1]), '-0.0 below +0.0 changes the points'
    counts, lin = reference('noise20x9x33')[:2]
    assert lin.size * 3 > case('noise20x9x33').size, 'more than a third of the voxels of pure noise are critical'
    vac = reference(VACUUM_CASE, VACUUM_TOL)
    assert 0 < vac[1].size < reference(VACUUM_CASE)[1].size


def test_vacuum_voxels_still_enter_their_neighbours_masks():
    rho = case(VACUUM_CASE)
    full, vac = reference(VACUUM_CASE), reference(VACUUM_CASE, VACUUM_TOL)
    keep = rho.reshape(-1)[full[1]] > VACUUM_TOL
    for a, b in zip(full[1:], vac[1:]):
        assert np.array_equal(a[keep], b)


def test_reference_bonds_on_the_eight_atoms_with_a_steepest_ascent_map():
    """the 2 x 2 x 2 arrangement: the 12 nearest-neighbour pairs, two saddles each (one towards each periodic image)"""
    rho = case('grid2x2x2')
    lab = steepest_ascent_labels(rho)
    assert lab.max() == 7
    pairs, saddles, rho_b, voxel, same = reference_bonds(rho, lab, 8)
    cells = np.rint(ATOMS_2X2X2[:, :3] * 2 - 0.5).astype(int)       # which of the 2 x 2 x 2 cells each atom sits in
    # labels are numbered by the maxima's voxel order; map them to atoms through the voxel of each maximum
    _, lin, L, _, _ = reference('grid2x2x2')
    maxima = lin[L == FULL]
    atom_of = {}
    for m in maxima.tolist():
        f = np.array(np.unravel_index(m, rho.shape)) / 24.0
        atom_of[int(lab.reshape(-1)[m])] = int(np.argmin(np.abs(((ATOMS_2X2X2[:, :3] - f + 0.5) % 1.0) - 0.5).sum(axis=1)))
    assert sorted(atom_of.values()) == list(range(8))
    want = sorted((min(a, b), max(a, b)) for a in range(8) for b in range(a + 1, 8) if np.abs(cells[a] - cells[b]).sum() == 1)
    got = sorted((min(atom_of[a], atom_of[b]), max(atom_of[a], atom_of[b])) for a, b in pairs.tolist())
    assert len(want) == 12 and got == want and saddles.tolist() == [2] * 12 and same == 0
    assert np.all(rho_b > synth.BACKGROUND) and np.all(np.diff(pairs[:, 0] * 8 + pairs[:, 1]) > 0)


def steepest_ascent_labels(rho):
    """every voxel to the maximum its steepest 14-neighbour ascent (in (key, lin) order) reaches; labels by maximum voxel order"""
    shape = rho.shape
    n = rho.size
    k = key(rho).reshape(shape)
    lin = np.arange(n, dtype=np.int64).reshape(shape)
    best_k, best_l = k.copy(), lin.copy()
    for d in OFFSETS:
        ku = np.roll(k, tuple(-x for x in d), axis=(0, 1, 2))
        lu = np.roll(lin, tuple(-x for x in d), axis=(0, 1, 2))
        take = (ku > best_k) | ((ku == best_k) & (lu > best_l))
        best_k, best_l = np.where(take, ku, best_k), np.where(take, lu, best_l)
    up = best_l.reshape(-1)
    for _ in range(64):
        nxt = up[up]
        if np.array_equal(nxt, up):
            break
        up = nxt
    tops = np.unique(up)
    return np.searchsorted(tops, up).astype(np.int32).reshape(shape)


def test_positions_use_the_expression_of_surface_dist():
    shape, lat = (5, 6, 7), synth.TRICLINIC
    vox = np.array([[0, 0, 0], [4, 5, 6], [1, 2, 3]])
    pos = critical.positions(vox, shape, lat)
    for v, p in zip(vox.tolist(), pos):
        for j in range(3):
            c = lat[0, j] * v[0] / 5
            c += lat[1, j] * v[1] / 6
            c += lat[2, j] * v[2] / 7
            assert c == p[j]
    assert np.array_equal(critical.positions(np.ravel_multi_index(vox.T, shape), shape, lat), pos)


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_critical_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_CRITICAL_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_CRITICAL_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert declared['XB_CRITICAL_FLOOD'] == 1 and declared['XB_CRITICAL_FULL'] == FULL and declared['XB_CRITICAL_LUT_SIZE'] == 1 << 14
    assert [declared['XB_CRITICAL_' + k] for k in ('MAXIMA', 'BOND_VOXELS', 'BOND_SUM', 'RING_VOXELS', 'RING_SUM', 'MINIMA', 'COUNTS')] == list(range(7))
    want = {
        'xb_critical_lut': ['uint8_t out[16384]'],
        'xb_critical_points': ['xb_ctx *c', 'double vac_tol', 'int flags', 'int64_t counts[6]', 'int64_t *n_list'],
        'xb_critical_fetch': ['xb_ctx *c', 'int64_t *lin', 'uint16_t *lower_mask', 'uint8_t *ring', 'uint8_t *bond', 'int64_t capacity'],
        'xb_critical_bonds': ['xb_ctx *c', 'int64_t n', 'int64_t *n_pairs', 'int64_t *same_basin'],
        'xb_critical_bonds_fetch': ['xb_ctx *c', 'int32_t *a', 'int32_t *b', 'int64_t *saddles', 'double *rho_b', 'int64_t *voxel',
                                    'int64_t capacity'],
        'xb_critical_release': ['xb_ctx *c'],
    }
    vp, pi, i64 = C.c_void_p, C.POINTER(C.c_int64), C.c_int64
    types = {
        'xb_critical_lut': [vp], 'xb_critical_points': [vp, C.c_double, C.c_int, pi, pi], 'xb_critical_fetch': [vp, vp, vp, vp, vp, i64],
        'xb_critical_bonds': [vp, i64, pi, pi], 'xb_critical_bonds_fetch': [vp, vp, vp, vp, vp, vp, i64], 'xb_critical_release': [vp],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, 'include/bader_hip.h does not declare ' + name
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types[name], name
    for method in ('critical_points', 'critical_bonds', 'critical_release'):
        assert callable(getattr(_lib.Context, method))
    # the definition is written down where the issue asks for it, and no timer slot or option key came with it
    assert 'd_{7+k} = -d_k' in text and 'minima - sum ring + sum bond - maxima == 0' in text
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert re.search(r'^## 17\.', design, flags=re.M)
    assert _lib.XB_TIMER_COUNT == 11 and not hasattr(_lib, 'XB_TIMER_CRITICAL') and not hasattr(_lib, 'XB_OPT_CRITICAL')


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.critical_flag is False and callable(Bader.critical_analysis)


def test_the_calls_need_the_gpu():
    from pybader_amd import build
    build.build_library()
    if _lib.load().xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.ones((4, 4, 4))
    with pytest.raises(_lib.BaderHipError):
        critical.critical_points(rho)
    with pytest.raises(_lib.BaderHipError):
        critical.bond_graph(rho, np.zeros((4, 4, 4), np.int32), 1)
