"""Connected regions without a GPU: the numpy restatement of the definition (include/bader_hip.h), checks of
the restatement itself -- against scipy.ndimage.label and on hand-made masks whose component count is known --, the host-side
derivations of pybader_amd.regions, the ABI and the argument errors that need no device.  tests/test_gpu_regions.py compares the
library with the functions of this file.

The restatement: min-label propagation over the 14 np.roll shifts to a fixed point (shifts that map every voxel onto itself
dropped; between two sweeps every member also takes the label of the voxel its label names -- a member of its own component --,
which only shortens the way to the same fixed point), renumbering by np.unique of the seeds, sums by math.fsum, shares by
np.unique on the keys."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest

from pybader_amd import _lib, build, nci, regions, synth
from test_multipole_cpu import U, VV, bound
import test_nci_cpu as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORWARD = [(0, 0, 1), (0, 1, 0), (0, 1, 1), (1, 0, 0), (1, 0, 1), (1, 1, 0), (1, 1, 1)]      # d_0 .. d_6 of the definition
OFFSETS = FORWARD + [tuple(-c for c in d) for d in FORWARD]
SHAPES = [(13, 17, 19), (20, 9, 33), (1, 2, 5), (2, 1, 40), (16, 16, 64), (8, 8, 32), (24, 16, 96)]
TILE = (8, 8, 32)


# ---- 1. the restatement ------------------------------------------------------------------------------------------------------------
def components(mask):
    """(regions int32 of the mask's shape: the component of every voxel, -1 outside; seeds int64[m], ascending)"""
    mask = np.asarray(mask, dtype=bool)
    shape, n = mask.shape, mask.size
    lin = np.arange(n, dtype=np.int64).reshape(shape)
    lab = np.where(mask, lin, n)
    shifts = [d for d in OFFSETS if any(d[i] % shape[i] for i in range(3))]      # (a shift that is the identity joins nothing)
    while True:
        new = lab
        for d in shifts:
            new = np.minimum(new, np.roll(lab, d, axis=(0, 1, 2)))
        new = np.where(mask, new, n)
        flat = np.append(new.reshape(-1), n)
        new = np.where(mask, flat[new], n)                                        # the label of the voxel the label names
        if np.array_equal(new, lab):
            break
        lab = new
    seeds = np.unique(lab[mask])
    out = np.full(shape, -1, np.int32)
    out[mask] = np.searchsorted(seeds, lab[mask]).astype(np.int32)
    return out, seeds.astype(np.int64)


def key(x):
    """the total order of the critical points on float64 bits"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return b ^ np.where(b >> np.uint64(63), np.uint64(0xffffffffffffffff), np.uint64(1) << np.uint64(63))


def per_component(reg, m, rho):
    """count int64[m], top int64[m] (the greatest key of rho, ties to the greater index) and, per component, the terms rho of its
    voxels in ascending index (a list of m arrays)"""
    r, flat = reg.reshape(-1), np.asarray(rho, dtype=np.float64).reshape(-1)
    members = np.flatnonzero(r >= 0)
    order = members[np.argsort(r[members], kind='stable')]
    starts = np.searchsorted(r[order], np.arange(m + 1))
    k = key(flat)
    count, top, terms = np.zeros(m, np.int64), np.zeros(m, np.int64), []
    for i in range(m):
        vox = order[starts[i]:starts[i + 1]]
        count[i] = vox.size
        top[i] = vox[np.lexsort((vox, k[vox]))[-1]]
        terms.append(flat[vox])
    return count, top, terms


def sums(terms):
    """(fsum, fsum of magnitudes) per entry of `terms`"""
    return np.array([math.fsum(t) for t in terms]), np.array([math.fsum(np.abs(t)) for t in terms])


def shares(reg, labels, n):
    """the triplets (component, label, count), ascending, over the members with a label in [0, n)"""
    r, lab = reg.reshape(-1).astype(np.int64), np.asarray(labels).reshape(-1).astype(np.int64)
    keep = (r >= 0) & (lab >= 0) & (lab < n)
    keys, cnt = np.unique(r[keep] * n + lab[keep], return_counts=True)
    return (keys // n).astype(np.int32), (keys % n).astype(np.int32), cnt.astype(np.int64)


def atoms_of(m, triplets):
    """regions.atoms_from_shares in plain loops"""
    out = np.full((m, 2), -1, np.int64)
    per = {}
    for c, a, k in zip(*triplets):
        per.setdefault(int(c), []).append((-int(k), int(a)))
    for c, rows in per.items():
        rows.sort()
        for j, (_, a) in enumerate(rows[:2]):
            out[c, j] = a
    return out


# the comparison of tests/test_gpu_regions.py (here, so that tests/history_common.py can make it too)
def check_sums(what, got, reg, seeds, rho, vv=VV):
    """seed, count, top with ==; the sums of rho and rho^2 under the bound (the worst figure printed before it is asserted)"""
    seed, count, top, s1, s2 = got[:5]
    m = seeds.size
    want_count, want_top, terms = per_component(reg, m, rho)
    assert seed.dtype == count.dtype == top.dtype == np.int64 and s1.dtype == s2.dtype == np.float64
    assert np.array_equal(seed, seeds), f'{what}: seeds'
    assert np.array_equal(count, want_count), f'{what}: counts'
    assert np.array_equal(top, want_top), f'{what}: tops'
    for name, g, tt in (('sum of rho', s1, terms), ('sum of rho^2', s2, [t * t for t in terms])):
        w, mag = sums(tt)
        lim = bound(want_count, mag[:, None], vv)[:, 0] if m else np.zeros(0)
        err = np.abs(g - w * vv)
        if m:
            k = int(np.argmax(err - lim))
            print(f'{what}: {name}, worst component {k} ({want_count[k]} voxels): off by {err[k]:.3e}, bound {lim[k]:.3e}')
        assert np.all(err <= lim), f'{what}: {name}'


# ---- 2. the masks both files use ---------------------------------------------------------------------------------------------------
def voxels(shape, *points):
    m = np.zeros(shape, bool)
    for p in points:
        m[tuple(c % s for c, s in zip(p, shape))] = True
    return m


def snake(shape=(24, 16, 96)):
    """a one-voxel-wide path through every 8 x 8 x 32 tile of `shape` that closes through the periodic wrap of y"""
    m = np.zeros(shape, bool)
    nx, ny, nz = shape
    xs = list(range(4, nx, 8))
    z_up = True
    cols = [(x, 4) for x in xs] + [(x, 12) for x in reversed(xs)]
    for i, (x, y) in enumerate(cols):
        m[x, y, :] = True
        if i + 1 < len(cols):
            x2, y2 = cols[i + 1]
            z = nz - 1 if z_up else 0
            m[min(x, x2):max(x, x2) + 1, min(y, y2):max(y, y2) + 1, z] = True
            z_up = not z_up
    z = nz - 1 if z_up else 0                          # where the last column ends: back to the first through the wrap of y
    m[xs[0], 12:, z] = True
    m[xs[0], :5, z] = True
    return m


def hand_masks():
    """(name, mask, the number of components) of the hand-made cases"""
    out = []
    for shape in SHAPES:
        out.append((f'nothing{shape}', np.zeros(shape, bool), 0))
        out.append((f'everything{shape}', np.ones(shape, bool), 1))
    for shape in [(16, 16, 64), (8, 8, 32), (24, 16, 96)]:
        m = np.zeros(shape, bool)
        m[::2, ::2, ::2] = True
        out.append((f'isolated{shape}', m, int(m.sum())))
    big = (16, 16, 64)
    out.append(('(1,-1,0)', voxels(big, (3, 4, 5), (4, 3, 5)), 2))
    out.append(('(1,-1,0) across a tile face', voxels(big, (7, 8, 5), (8, 7, 5)), 2))
    out.append(('(1,1,-1)', voxels(big, (3, 3, 5), (4, 4, 4)), 2))
    out.append(('(1,1,-1) across a tile corner', voxels(big, (7, 7, 32), (8, 8, 31)), 2))
    out.append(('(1,1,1) across a tile corner', voxels(big, (7, 7, 31), (8, 8, 32)), 1))
    for shape in [(16, 16, 64), (13, 17, 19), (8, 8, 32), (24, 16, 96)]:
        out.append((f'(1,1,1) across the periodic corner{shape}', voxels(shape, tuple(s - 1 for s in shape), (0, 0, 0)), 1))
        for ax in range(3):
            lo, hi = [3, 5, 6], [3, 5, 6]
            lo[ax], hi[ax] = 0, shape[ax] - 1
            out.append((f'the two sides of the wrap of axis {ax}{shape}', voxels(shape, lo, hi), 1))
    out.append(('snake', snake(), 1))
    return out


def random_mask(shape, density, seed=11):
    return np.random.default_rng(seed + int(1000 * density) + sum(shape)).random(shape) < density


@functools.lru_cache(maxsize=None)
def hand_reference(i):
    return components(hand_masks()[i][1])


# the inputs of the GPU sums: (name, density, mask) -- the islands of the synthetic density above its 0.8 quantile (one per atom or
# pair of atoms), the same with noise, and the NCI region of the 'holes' density on both lattices
def sum_level(rho):
    return float(np.quantile(rho, 0.8))


@functools.lru_cache(maxsize=None)
def sum_inputs():
    out = []
    for shape in [(13, 17, 19), (20, 9, 33)]:
        for kind in ('synth', 'rough'):
            rho = tn.density(kind, shape, 'cubic')
            out.append((f'{kind}{shape}', rho, rho >= sum_level(rho)))
        for lname in tn.LATS:
            v = tn.values('holes', shape, lname)
            out.append((f'holes{shape}{lname}', tn.density('holes', shape, lname), tn.region(v, *tn.SUM_CUTS[:2])))
    return out


# ---- 3. the restatement against scipy and the hand-made masks --------------------------------------------------------------------
@pytest.mark.parametrize('density', [0.1, 0.3, 0.6])
@pytest.mark.parametrize('shape', [(13, 17, 19), (20, 9, 33), (6, 5, 40)])
def test_the_restatement_is_scipy_label_inside_the_cell(shape, density):
    ndimage = pytest.importorskip('scipy.ndimage')
    mask = random_mask(shape, density)
    mask[0], mask[-1], mask[:, 0], mask[:, -1], mask[:, :, 0], mask[:, :, -1] = (False,) * 6     # nothing touches the boundary
    structure = np.zeros((3, 3, 3), bool)
    structure[1, 1, 1] = True
    for d in OFFSETS:
        structure[1 + d[0], 1 + d[1], 1 + d[2]] = True
    assert structure.sum() == 15
    lab, m = ndimage.label(mask, structure)
    reg, seeds = components(mask)
    assert m == seeds.size and (m > 1 or density > 0.5)      # (above the percolation threshold one piece may hold everything)
    # scipy's labels as a partition, numbered by the smallest index of each piece
    lin = np.arange(mask.size).reshape(shape)
    first = np.full(m + 1, mask.size)
    np.minimum.at(first, lab.reshape(-1), lin.reshape(-1))
    order = np.argsort(first[1:])
    rank = np.empty(m, np.int64)
    rank[order] = np.arange(m)
    want = np.where(lab > 0, rank[np.maximum(lab, 1) - 1], -1)
    assert np.array_equal(reg, want) and np.array_equal(seeds, np.sort(first[1:]))


@pytest.mark.parametrize('i', range(len(hand_masks())))
def test_hand_made_masks_have_the_known_component_count(i):
    name, mask, want = hand_masks()[i]
    reg, seeds = hand_reference(i)
    assert seeds.size == want, name
    assert np.array_equal(reg >= 0, mask)
    if want:
        assert reg.reshape(-1)[seeds].tolist() == list(range(want)) and seeds[0] == np.flatnonzero(mask)[0]
        lin = np.arange(mask.size).reshape(mask.shape)
        assert all(lin[reg == k].min() == seeds[k] for k in range(min(want, 5)))
    if want == 1:
        assert (reg[mask] == 0).all()


def test_the_snake_visits_every_tile_and_is_thin():
    m = snake()
    tiles = m.reshape(3, 8, 2, 8, 3, 32).any(axis=(1, 3, 5))
    assert tiles.all() and m.sum() < m.size // 50


def test_isolated_voxels_meet_through_an_odd_wrap():
    """all coordinates even on (13, 17, 19): the last plane of every axis is even too and touches the first through the wrap"""
    shape = (13, 17, 19)
    m = np.zeros(shape, bool)
    m[::2, ::2, ::2] = True
    reg, seeds = components(m)
    assert seeds.size < m.sum() and reg[0, 0, 0] == reg[12, 0, 0] == reg[0, 16, 0] == reg[0, 0, 18] == reg[12, 16, 18] == 0
    assert reg[2, 2, 2] != 0


def test_short_axes():
    """an axis of length 1 joins nothing along itself; an axis of length 2 joins both ways to the same voxel"""
    assert components(np.ones((1, 1, 1), bool))[1].tolist() == [0]
    reg, seeds = components(voxels((1, 2, 5), (0, 0, 0), (0, 0, 2), (0, 1, 3)))      # (0,1,1) joins (0,0,2) and (0,1,3)
    assert seeds.tolist() == [0, 2] and reg[0, 1, 3] == 1
    reg, seeds = components(voxels((2, 1, 40), (0, 0, 0), (1, 0, 39), (1, 0, 20)))   # (1,0,1) across the wrap of z
    assert seeds.tolist() == [0, 60]


def test_random_masks_are_partitions_closed_under_the_adjacency():
    for shape in [(13, 17, 19), (2, 1, 40), (1, 2, 5)]:
        for density in (0.1, 0.3, 0.6):
            mask = random_mask(shape, density)
            reg, seeds = components(mask)
            assert np.array_equal(reg >= 0, mask)
            for d in OFFSETS:
                other = np.roll(reg, d, axis=(0, 1, 2))
                both = (reg >= 0) & (other >= 0)
                assert np.array_equal(reg[both], other[both])
            assert np.array_equal(np.unique(reg[mask]), np.arange(seeds.size))


# ---- 4. the host-side derivations ---------------------------------------------------------------------------------------------------
def test_atoms_from_shares_ties_and_missing():
    comp = np.array([0, 0, 0, 1, 3, 3, 3, 3], np.int32)
    lab = np.array([2, 5, 7, 4, 9, 1, 6, 0], np.int32)
    cnt = np.array([3, 9, 3, 1, 5, 5, 5, 2], np.int64)
    got = regions.atoms_from_shares(5, (comp, lab, cnt))
    assert got.tolist() == [[5, 2], [4, -1], [-1, -1], [1, 6], [-1, -1]]
    assert np.array_equal(got, atoms_of(5, (comp, lab, cnt)))
    assert regions.atoms_from_shares(0, (comp[:0], lab[:0], cnt[:0])).shape == (0, 2)
    assert regions.atoms_from_shares(2, (comp[:0], lab[:0], cnt[:0])).tolist() == [[-1, -1], [-1, -1]]
    rng = np.random.default_rng(3)
    reg = rng.integers(-1, 6, 4000)
    labels = rng.integers(-1, 5, 4000)
    t = shares(reg, labels, 4)
    assert np.array_equal(regions.atoms_from_shares(6, t), atoms_of(6, t))
    assert t[2].sum() == ((reg >= 0) & (labels >= 0) & (labels < 4)).sum()


def test_the_bound_notices_a_voxel_in_the_wrong_component():
    """one voxel counted in another component moves both components' sums of rho and of rho^2 by more than the bound, on every
    input of the GPU sums -- and the voxel is a typical one of its component (the median density), not the largest"""
    seen = 0
    for name, rho, mask in sum_inputs():
        reg, seeds = components(mask)
        m = seeds.size
        assert m >= 2, name
        flat = np.asarray(rho, dtype=np.float64).reshape(-1)
        for terms_all in (flat, flat * flat):
            count, _, terms = per_component(reg, m, terms_all)
            s, mag = sums(terms)
            lim = bound(count, mag[:, None], VV)[:, 0]
            a = int(np.argmax(count))
            b = (a + 1) % m
            mine = np.flatnonzero(reg.reshape(-1) == a)
            vox = mine[np.argsort(terms_all[mine])[mine.size // 2]]
            wrong = reg.copy()
            wrong.reshape(-1)[vox] = b
            count2, _, terms2 = per_component(wrong, m, terms_all)
            s2, _ = sums(terms2)
            for k in (a, b):
                assert abs(s2[k] - s[k]) * VV > lim[k], (name, k)
                assert count2[k] != count[k]
        seen += 1
    assert seen == 8 and U == 2.0 ** -53


# ---- 5. ABI and errors ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


def test_header_and_binding_agree_on_the_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_DOMAINS_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_DOMAINS_')}
    assert declared and declared == mirrored, set(declared.items()) ^ set(mirrored.items())
    assert declared == {'XB_DOMAINS_ABOVE': 0, 'XB_DOMAINS_BELOW': 1, 'XB_DOMAINS_NCI': 2, 'XB_DOMAINS_GLOBAL': 1,
                        'XB_DOMAINS_SHARES_LIST': 2, 'XB_DOMAINS_GATHER': 4, 'XB_DOMAINS_TIMES': 8, 'XB_DOMAINS_SHARE_CELLS': 1 << 24}
    vp, pd, pi, i64, dbl, i = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int64), C.c_int64, C.c_double, C.c_int
    types = {'xb_regions_label': [vp, i, vp, dbl, pd, dbl, dbl, i, pi],
             'xb_regions_sums': [vp, dbl, dbl, pi, pi, pi, pd, pd, pi, pd, pd, i64],
             'xb_regions_shares': [vp, i64, i, pi], 'xb_regions_shares_fetch': [vp, vp, vp, pi, i64],
             'xb_regions_fetch_map': [vp, i, vp], 'xb_regions_times': [vp, pd], 'xb_regions_release': [vp]}
    for name, argtypes in types.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m and len(m.group(1).split(',')) == len(argtypes), name
        assert _lib.SYMBOLS[name] == (C.c_int, argtypes), name
    for method in ('regions_label', 'regions_sums', 'regions_shares', 'regions_map', 'regions_release'):
        assert callable(getattr(_lib.Context, method))
    assert 'd_0 .. d_6 = (0,0,1)' in text and 'ascending seed' in text
    assert re.search(r'^## 22\.', open(os.path.join(ROOT, 'DESIGN.md')).read(), flags=re.M)
    # the tile's parents and the staged density leave four workgroups to a compute unit
    assert (10 * 10 * 34 * 8 + 8 * 8 * 32 * 4) * 4 <= 160 * 1024 and TILE == (8, 8, 32)


def test_the_library_exports_the_calls_and_refuses_a_null_context(lib):
    m = C.c_int64(-7)
    out = np.full(8, -7, np.int64)
    f = np.full(8, -7.0)
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int64)
    assert lib.xb_regions_label(None, 0, None, 0.5, None, 0.0, 0.0, 0, C.byref(m)) == _lib.XB_E_STATE
    assert lib.xb_regions_sums(None, 1.0, float('nan'), out.ctypes.data_as(pi), out.ctypes.data_as(pi), out.ctypes.data_as(pi),
                               f.ctypes.data_as(pd), f.ctypes.data_as(pd), None, None, None, 8) == _lib.XB_E_STATE
    assert lib.xb_regions_shares(None, 2, 0, C.byref(m)) == _lib.XB_E_STATE
    assert lib.xb_regions_shares_fetch(None, out.ctypes.data, out.ctypes.data, out.ctypes.data_as(pi), 8) == _lib.XB_E_STATE
    assert lib.xb_regions_fetch_map(None, 0, out.ctypes.data) == _lib.XB_E_STATE
    assert lib.xb_regions_times(None, f.ctypes.data_as(pd)) == _lib.XB_E_STATE
    assert lib.xb_regions_release(None) == _lib.XB_E_ARG
    assert m.value == -7 and (out == -7).all() and (f == -7.0).all(), 'a refused call writes nothing'


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.nci_domains_flag is False and callable(Bader.nci_domain_analysis)
    assert callable(nci.nci_domains) and callable(regions.connected_regions)


def test_the_calls_need_the_gpu(lib):
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.full((4, 4, 4), 0.02)
    for call in (lambda: regions.connected_regions(rho, 0.01), lambda: nci.nci_domains(rho, np.eye(3))):
        with pytest.raises(_lib.BaderHipError):
            call()
