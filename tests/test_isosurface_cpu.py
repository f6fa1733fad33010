"""The host side of the isosurfaces (pybader_amd/isosurface.py, xb_isosurface_table) and the plain numpy restatement of the
definition in include/bader_hip.h / DESIGN.md section 21 that tests/test_gpu_isosurface.py compares the kernels with: the
integers and the vertices with ==, the sums with math.fsum of the restated terms under the bound of tests/test_laplacian_cpu.py.

`restate` marches every tetrahedron of every cube with numpy: np.roll-free wrapped index tables for the neighbours, the table of
`restated_table` (built from midpoints and a float cross product, not from the library's integer code) for the corner order.
What no restatement error can fake: every mesh edge lies in exactly two triangles, once in each direction; V equals the number of
crossing lattice edges; and the Euler characteristic of the mesh is twice the alternating sum of the critical points of
tests/test_critical_cpu.py above the level -- an independent piece of code."""
import ctypes as C
import functools
import itertools
import math
import os
import re
import types

import numpy as np
import pytest

from pybader_amd import _lib, build, isosurface, synth
from test_critical_cpu import FULL, case, reference_points
from test_laplacian_cpu import geometry, sum_bound
from test_multipole_cpu import U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PERMS = list(itertools.permutations(range(3)))                    # lexicographic
CV = np.array([((c >> 2) & 1, (c >> 1) & 1, c & 1) for c in range(8)], dtype=np.int64)    # corner 4 cx + 2 cy + cz
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
LAT = {'synth40x36x44': synth.TRICLINIC, 'tric24': np.array([[6.0, 0.0, 0.0], [1.5, 5.5, 0.0], [0.7, 1.1, 6.2]]), 'rough': synth.TRICLINIC,
       'plateau': synth.CUBIC6, 'noise20x9x33': synth.TRICLINIC, 'gauss12x10x16': synth.CUBIC6}


def corner(tau, i):
    """corner P_i of tetrahedron tau as cube corner bits: the path 0 -> e_a -> e_a + e_b -> (1, 1, 1)"""
    c = 0
    for j in range(i):
        c |= 4 >> PERMS[tau][j]
    return c


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def restated_table():
    """uint8[6, 16, 8]: the number of triangles and their corners as (owner corner) << 3 | k per tetrahedron and inside mask"""
    tab = np.full((6, 16, 8), 255, np.uint8)
    tab[:, :, 0] = 0
    for tau in range(6):
        P = np.array([CV[corner(tau, i)] for i in range(4)], dtype=np.float64)
        for m in range(1, 15):
            ins = [i for i in range(4) if m >> i & 1]
            outs = [i for i in range(4) if not m >> i & 1]
            if len(ins) in (1, 3):
                apex = ins[0] if len(ins) == 1 else outs[0]
                tris = [[tuple(sorted((apex, j))) for j in range(4) if j != apex]]
            else:
                (i, j), (k, l) = ins, outs
                ik, il, jl, jk = (tuple(sorted(e)) for e in ((i, k), (i, l), (j, l), (j, k)))
                tris = [[ik, il, jl], [ik, jl, jk]]
            away = P[outs].mean(axis=0) - P[ins].mean(axis=0)
            for t, tri in enumerate(tris):
                q = [(P[a] + P[b]) / 2 for a, b in tri]
                dot = float(np.dot(np.cross(q[1] - q[0], q[2] - q[0]), away))
                assert dot != 0.0
                if dot < 0:
                    tri[1], tri[2] = tri[2], tri[1]
                for v, (a, b) in enumerate(tri):
                    lo, hi = corner(tau, a), corner(tau, b)
                    tab[tau, m, 1 + 3 * t + v] = lo << 3 | ((hi ^ lo) - 1)
            tab[tau, m, 0] = len(tris)
    tab.flags.writeable = False
    return tab


def voxel_lattice(lattice, shape):
    """(A as nested float64, |det A| / 6), the determinant in the order of the Laplacian block"""
    A, _, _ = geometry(lattice, shape)
    c00 = A[1][1] * A[2][2] - A[1][2] * A[2][1]
    c01 = A[1][2] * A[2][0] - A[1][0] * A[2][2]
    c02 = A[1][0] * A[2][1] - A[1][1] * A[2][0]
    det = (A[0][0] * c00 + A[0][1] * c01) + A[0][2] * c02
    return A, abs(det) / np.float64(6.0)


def restate(f, level, lattice, g=None, labels=None, n=0):
    """The whole definition -> a namespace: vertices, colour, triangles, wrap, cells, tau (per triangle), crossing (the number of
    crossing lattice edges), area_terms [T], frac [N, 6] (the inside fraction per tetrahedron), tet (|det A| / 6), shares (per
    label a list of arrays of fraction / inside corners), area, volume, volume_by_label (math.fsum of the terms)"""
    f = np.ascontiguousarray(f, dtype=np.float64)
    shape, N = f.shape, f.size
    nvec = np.array(shape, dtype=np.int64)
    level = np.float64(level)
    with np.errstate(invalid='ignore'):
        il = (f >= level).reshape(-1)
    fl = f.reshape(-1)
    idx = np.indices(shape).reshape(3, -1).T.astype(np.int64)
    NB = []
    for c in range(8):
        p = (idx + CV[c]) % nvec
        NB.append((p[:, 0] * shape[1] + p[:, 1]) * shape[2] + p[:, 2])
    NB = np.stack(NB)
    cross = np.stack([il != il[NB[k + 1]] for k in range(7)], axis=1)
    vid = np.full((N, 7), -1, np.int64)
    vid[cross] = np.arange(int(cross.sum()))                 # C order of [N, 7]: ascending 7 lin + k
    t = np.full((N, 7), np.nan)
    with np.errstate(all='ignore'):
        for k in range(7):
            a, b = fl, fl[NB[k + 1]]
            t[:, k] = np.where(cross[:, k], (level - a) / (b - a), np.nan)
    vv, kk = np.nonzero(cross)
    tt = t[vv, kk]
    vertices = np.where(CV[kk + 1] != 0, idx[vv].astype(np.float64) + tt[:, None], idx[vv].astype(np.float64))
    colour = None
    if g is not None:
        gl = np.ascontiguousarray(g, dtype=np.float64).reshape(-1)
        ga, gb = gl[vv], gl[NB[kk + 1, vv]]
        with np.errstate(all='ignore'):
            colour = ga + tt * (gb - ga)
    A, tet = voxel_lattice(lattice, shape)
    tab = restated_table()
    frac = np.zeros((N, 6))
    lab = None if labels is None else np.asarray(labels).reshape(-1).astype(np.int64)
    share_lab, share_val = [], []
    parts = []
    for tau in range(6):
        pc = [corner(tau, i) for i in range(4)]
        m = sum(il[NB[pc[i]]].astype(np.int64) << i for i in range(4))
        te = {(lo, hi): t[NB[pc[lo]], (pc[hi] ^ pc[lo]) - 1] for lo, hi in PAIRS}
        for mm in range(1, 16):
            sel = np.flatnonzero(m == mm)
            if sel.size == 0:
                continue
            ins = [i for i in range(4) if mm >> i & 1]
            outs = [i for i in range(4) if not mm >> i & 1]

            def u(a, b):
                return te[(a, b)][sel] if a < b else 1.0 - te[(b, a)][sel]
            with np.errstate(all='ignore'):
                if len(ins) == 4:
                    fr = np.ones(sel.size)
                elif len(ins) == 1:
                    fr = (u(ins[0], outs[0]) * u(ins[0], outs[1])) * u(ins[0], outs[2])
                elif len(ins) == 3:
                    fr = 1.0 - (u(outs[0], ins[0]) * u(outs[0], ins[1])) * u(outs[0], ins[2])
                else:
                    (i, j), (k, l) = ins, outs
                    uik, uil, ujk, ujl = u(i, k), u(i, l), u(j, k), u(j, l)
                    fr = (uik * uil + (uik * ujl) * (1.0 - uil)) + (ujk * ujl) * (1.0 - uik)
                frac[sel, tau] = fr
                each = fr / np.float64(len(ins))
            if lab is not None and n >= 1:
                for i in ins:
                    share_lab.append(lab[NB[pc[i]][sel]])
                    share_val.append(each)
            for tr in range(int(tab[tau, mm, 0])):
                ids, wrap, q = [], np.zeros(sel.size, np.int64), []
                for v in range(3):
                    code = int(tab[tau, mm, 1 + 3 * tr + v])
                    c, k = code >> 3, code & 7
                    vi = vid[NB[c][sel], k]
                    assert (vi >= 0).all()
                    bit = (CV[c][None, :] != 0) & (idx[sel] + 1 >= nvec)
                    for j in range(3):
                        wrap |= bit[:, j].astype(np.int64) << (3 * v + j)
                    ids.append(vi)
                    q.append(np.where(bit, vertices[vi] + nvec.astype(np.float64), vertices[vi]))
                parts.append((sel, np.full(sel.size, tau), np.full(sel.size, tr), np.stack(ids, axis=1), wrap, np.stack(q, axis=1)))
    out = types.SimpleNamespace(shape=shape, level=float(level), vertices=vertices, colour=colour, crossing=int(cross.sum()), frac=frac, tet=tet)
    if parts:
        cell, tau_, tr_, ids, wrap, q = (np.concatenate([p[i] for p in parts]) for i in range(6))
        order = np.lexsort((tr_, tau_, cell))
        cell, tau_, ids, wrap, q = cell[order], tau_[order], ids[order], wrap[order], q[order]
    else:
        cell, tau_, ids, wrap, q = np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros((0, 3), np.int64), np.zeros(0, np.int64), np.zeros((0, 3, 3))
    out.triangles, out.wrap, out.cells, out.tau, out.corners_voxel = ids, wrap.astype(np.uint16), cell, tau_, q
    with np.errstate(all='ignore'):
        e1, e2 = q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]
        E1 = [(e1[:, 0] * A[0][j] + e1[:, 1] * A[1][j]) + e1[:, 2] * A[2][j] for j in range(3)]
        E2 = [(e2[:, 0] * A[0][j] + e2[:, 1] * A[1][j]) + e2[:, 2] * A[2][j] for j in range(3)]
        cx, cy, cz = E1[1] * E2[2] - E1[2] * E2[1], E1[2] * E2[0] - E1[0] * E2[2], E1[0] * E2[1] - E1[1] * E2[0]
        out.area_terms = 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)
    out.area = math.fsum(out.area_terms)
    out.volume = math.fsum(frac.reshape(-1)) * tet
    out.n = int(n)
    out.share_sum, out.share_count = np.zeros(max(n, 0)), np.zeros(max(n, 0), np.int64)
    if share_lab:
        sl, sv = np.concatenate(share_lab), np.concatenate(share_val)
        keep = (sl >= 0) & (sl < n)
        sl, sv = sl[keep], sv[keep]
        order = np.argsort(sl, kind='stable')
        sl, sv = sl[order], sv[order]
        vals, starts = np.unique(sl, return_index=True)
        for a, lo, hi in zip(vals, starts, list(starts[1:]) + [sl.size]):
            out.share_sum[a], out.share_count[a] = math.fsum(sv[lo:hi]), hi - lo
    out.volume_by_label = out.share_sum * tet
    return out


def as_mesh(r, lattice):
    return isosurface.Mesh(r.shape, r.level, lattice, r.vertices, r.colour, r.triangles, r.wrap, r.cells, r.area, r.volume, r.volume_by_label)


# ---- the comparisons of tests/test_gpu_isosurface.py (here, so that tests/history_common.py can make them too) ---------------------
def first_difference(got, want, what):
    """None, or where the mesh `got` (the tuple of Context.isosurface) first differs from the restatement `want`"""
    vert, col, tri, wrap, cell = got[:5]
    if (vert.shape[0], tri.shape[0]) != (want.vertices.shape[0], want.triangles.shape[0]):
        return f'{what}: {vert.shape[0]} vertices and {tri.shape[0]} triangles, restated {want.vertices.shape[0]} and {want.triangles.shape[0]}'
    for name, a, b in (('triangles', tri, want.triangles), ('wrap', wrap, want.wrap), ('cells', cell, want.cells)):
        if not np.array_equal(a, b):
            return f'{what}: {name} differ at {int(np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))[0])}'
    for name, a, b in (('vertices', vert, want.vertices), ('colour', col, want.colour)):
        if b is None:
            continue
        if not np.array_equal(a.view(np.uint64), b.view(np.uint64)):
            bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(axis=1))
            return f'{what}: {name} differ in {bad.shape[0]} rows, first {int(bad[0])}: {a[bad[0]]!r} against {b[bad[0]]!r}'
    return None


def sums_difference(got, want, what):
    """None, or which of area, volume and volume_by_label lies outside the bound of the sums around math.fsum of the terms"""
    area, volume, vbl = got[5:]
    one = np.ones(1, np.int64)
    mag_a = np.array([math.fsum(want.area_terms)])
    if not abs(area - want.area) <= sum_bound(one * want.area_terms.shape[0], mag_a, 1.0)[0]:
        return f'{what}: area {area!r} against {want.area!r}'
    frac = want.frac.reshape(-1)
    terms = frac[frac != 0.0]
    mag_v = np.array([math.fsum(np.abs(terms))])
    if not abs(volume - want.volume) <= sum_bound(one * terms.shape[0], mag_v, float(want.tet))[0]:
        return f'{what}: volume {volume!r} against {want.volume!r}'
    if want.n:
        lim = sum_bound(want.share_count, want.share_sum, float(want.tet))
        off = np.abs(vbl - want.volume_by_label) > lim
        if vbl.shape != want.volume_by_label.shape or off.any():
            return f'{what}: volume_by_label differs for {int(off.sum())} labels, first {int(np.flatnonzero(off)[0])}'
    return None


def alternating_sum(rho, level):
    """maxima - sum bond + sum ring - minima over the critical points with rho >= level"""
    _, lin, L, ring, bond = reference_points(rho)
    keep = rho.reshape(-1)[lin] >= level
    L, ring, bond = L[keep], ring[keep].astype(np.int64), bond[keep].astype(np.int64)
    return int((L == FULL).sum() - bond.sum() + ring.sum() - (L == 0).sum())


# ---- inputs (shared with tests/test_gpu_isosurface.py) -----------------------------------------------------------------------------
TOPOLOGY_CASES = ['synth40x36x44', 'tric24', 'rough', 'plateau', 'noise20x9x33', 'gauss12x10x16']
QUANTILES = (0.3, 0.6, 0.9)
PLATEAU_VALUE = 0.375


def levels(name):
    """(what, level) of one case: its three quantiles, and for `plateau` a level that equals voxel values exactly"""
    out = [(f'q{q}', float(np.quantile(case(name), q))) for q in QUANTILES]
    if name == 'plateau':
        out.append(('value', PLATEAU_VALUE))
    return out


LEVEL_SETS = [(name, what) for name in TOPOLOGY_CASES for what, _ in levels(name)]


@functools.lru_cache(maxsize=None)
def restated_case(name, what, with_colour=False):
    rho = case(name)
    g = colour_field(rho.shape) if with_colour else None
    return restate(rho, dict(levels(name))[what], LAT[name], g)


@functools.lru_cache(maxsize=None)
def colour_field(shape):
    a = synth.hash_noise(shape, 17) - 0.5
    a.flags.writeable = False
    return a


# ---- the table -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


def test_library_table_equals_the_restatement(lib):
    assert np.array_equal(_lib.isosurface_table(), restated_table())


def test_the_table_has_one_two_or_no_triangles():
    tab = restated_table()
    for tau in range(6):
        for m in range(16):
            assert tab[tau, m, 0] == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[bin(m).count('1')]
            used = tab[tau, m, 1:1 + 3 * tab[tau, m, 0]]
            assert (used < 64).all() and (tab[tau, m, 1 + 3 * tab[tau, m, 0]:] == 255).all()
            for code in used:       # the owner corner and the offset do not share an axis: the other end is a corner of the cube
                assert (int(code) >> 3) & ((int(code) & 7) + 1) == 0


# ---- watertightness, orientation, the Euler identity ----------------------------------------------------------------------------------
@pytest.mark.parametrize('name,what', LEVEL_SETS)
def test_the_mesh_is_closed_oriented_and_has_the_euler_characteristic_of_the_critical_points(name, what):
    r = restated_case(name, what)
    rho = case(name)
    T, V = r.triangles.shape[0], r.vertices.shape[0]
    assert T > 0 and V == r.crossing and np.unique(r.triangles).shape[0] == V
    assert np.isfinite(r.vertices).all()
    # every directed edge once, and its reverse as well: every edge in exactly two triangles, once in each direction
    t = r.triangles
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    assert (e[:, 0] != e[:, 1]).all()
    fwd = e[:, 0] * V + e[:, 1]
    assert np.unique(fwd).shape[0] == fwd.shape[0]
    assert np.array_equal(np.sort(fwd), np.sort(e[:, 1] * V + e[:, 0]))
    # the normal in voxel coordinates points away from the tetrahedron's inside corners (a level that equals voxel values puts
    # vertices onto voxels, t = 0: a triangle whose corners coincide there has no normal and claims nothing)
    q = r.corners_voxel
    normal = np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0])
    base = np.stack(np.unravel_index(r.cells, rho.shape), axis=1)
    inside = rho >= r.level
    for tau in range(6):
        sel = np.flatnonzero(r.tau == tau)
        P = base[sel, None, :] + np.array([CV[corner(tau, i)] for i in range(4)])[None]          # [S, 4, 3], unwrapped
        ins = inside[tuple((P % np.array(rho.shape)).transpose(2, 0, 1))]                      # [S, 4]
        assert (ins.any(axis=1) & ~ins.all(axis=1)).all()
        mean_in = (P * ins[:, :, None]).sum(axis=1) / ins.sum(axis=1)[:, None]
        mean_out = (P * ~ins[:, :, None]).sum(axis=1) / (~ins).sum(axis=1)[:, None]
        assert (((normal[sel] * (mean_out - mean_in)).sum(axis=1) > 0) | (normal[sel] == 0).all(axis=1)).all()
    assert (normal != 0).any(axis=1).all() or name == 'plateau'
    m = as_mesh(r, LAT[name])
    assert m.euler == V - 3 * T // 2 + T and T % 2 == 0
    assert m.euler == 2 * alternating_sum(rho, r.level)


COUNTS = [('synth40x36x44', 'q0.6', 67944, 33974, 2), ('rough', 'q0.3', 72872, 34662, -1774), ('plateau', 'value', 69568, 33788, -996),
          ('noise20x9x33', 'q0.9', 14040, 7538, 518)]


@pytest.mark.parametrize('name,what,T,V,chi', COUNTS)
def test_counts_of_an_independent_marcher(name, what, T, V, chi):
    r = restated_case(name, what)
    assert (r.triangles.shape[0], r.vertices.shape[0], as_mesh(r, LAT[name]).euler) == (T, V, chi)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------
def cell_volume(lattice):
    return abs(float(np.linalg.det(np.asarray(lattice, dtype=np.float64))))


def test_a_constant_field():
    rho, lat = case('constant'), synth.TRICLINIC
    r = restate(rho, 0.25, lat)
    assert r.triangles.shape[0] == 0 and r.vertices.shape[0] == 0 and r.area == 0.0 and (r.frac == 1.0).all()
    assert abs(r.volume - cell_volume(lat)) <= 1e-14 * cell_volume(lat)
    r = restate(rho, 0.5, lat)
    assert r.triangles.shape[0] == 0 and r.volume == 0.0 and (r.frac == 0.0).all()


@pytest.mark.parametrize('level', [0.0, -0.0])
def test_both_zeros_are_inside_at_level_zero(level):
    r = restate(case('zeros_spike'), level, synth.CUBIC6)
    assert r.triangles.shape[0] == 0 and r.crossing == 0 and (r.frac == 1.0).all()


def test_a_nan_voxel_is_outside():
    rho = np.ones((5, 6, 7))
    rho[2, 3, 4] = np.nan
    r = restate(rho, 0.5, synth.CUBIC6)
    assert r.crossing == 14 and r.vertices.shape[0] == 14          # the 14 lattice edges at the voxel
    assert r.triangles.shape[0] == 24 and (r.frac == 1.0).sum() == r.frac.size - 24      # one triangle in each of its 24 tetrahedra
    assert np.isnan(r.frac).sum() == 24 and np.isnan(r.vertices).any(axis=1).all()         # t = (level - NaN) / ...: the definition stands


@pytest.mark.parametrize('level,t_up,t_wrap', [(2.5, 0.5, 0.5), (2.25, 0.25, 0.55)])
def test_a_ramp_along_x_by_hand(level, t_up, t_wrap):
    """f = x on 6 x 4 x 4: inside is 3 <= x <= 5; the surface crosses between x = 2 and 3 at t = level - 2, and between x = 5 and
    the wrapped x = 0 at t = (level - 5) / (0 - 5).  Two flat sheets: area 2 |a_y x a_z|; volume (3 - t_up + t_wrap) planes"""
    shape, lat = (6, 4, 4), synth.TRICLINIC
    rho = np.broadcast_to(np.arange(6.0)[:, None, None], shape).copy()
    r = restate(rho, level, lat)
    owner_x = np.floor(r.vertices[:, 0])
    t = r.vertices[:, 0] - owner_x
    assert set(owner_x.tolist()) == {2.0, 5.0}
    assert np.array_equal(t[owner_x == 2.0], np.full((owner_x == 2.0).sum(), t_up))
    assert np.allclose(t[owner_x == 5.0], t_wrap, rtol=0, atol=4 * U * 6)
    assert r.vertices.shape[0] == 2 * 16 * 4 and r.triangles.shape[0] == 2 * 16 * 8     # x, xz, xy, xyz edges; per cube 1 + 1 + 2 + 2 + 1 + 1 triangles
    A = np.asarray(lat) / np.array(shape)[:, None]
    sheet = 16 * float(np.linalg.norm(np.cross(A[1], A[2])))
    assert abs(r.area - 2 * sheet) <= 1e-13 * sheet
    want = (3.0 - t_up + t_wrap) * 16 * abs(float(np.linalg.det(A)))
    assert abs(r.volume - want) <= 1e-13 * want
    m = as_mesh(r, lat)
    assert m.euler == 0 and (m.wrap[owner_x[m.triangles].max(axis=1) == 5.0] != 0).any()      # two tori; the upper sheet's cubes wrap


@pytest.mark.parametrize('name', ['rough', 'noise20x9x33', 'gauss12x10x16'])
def test_inside_and_outside_fill_the_cell(name):
    """volume(f, level) + volume(-f, -level) is the cell when no voxel equals the level: the same t on every edge, the inside
    fractions complementary.  Each fraction is a few roundings of numbers in [0, 1] (at most 8 operations): 16 u per tetrahedron
    on top of the two sums' own bounds"""
    rho, lat = case(name), LAT[name]
    level = float(np.quantile(rho, 0.6))
    assert not (rho == level).any()
    a, b = restate(rho, level, lat), restate(-rho, -level, lat)
    n_tet = 6 * rho.size
    assert np.array_equal(a.vertices, b.vertices) and a.triangles.shape == b.triangles.shape
    assert abs((a.volume + b.volume) - n_tet * a.tet) <= (16 + 4) * U * n_tet * a.tet
    assert abs(a.area - b.area) <= 8 * U * a.triangles.shape[0] * float(a.area_terms.max())


@pytest.mark.parametrize('name', ['rough', 'gauss12x10x16'])
def test_the_labels_share_the_whole_volume(name):
    """sum volume_by_label == volume: a share is fraction / k, one more rounding per share"""
    rho, lat = case(name), LAT[name]
    lab = (np.arange(rho.size) % 7).reshape(rho.shape).astype(np.int32)
    r = restate(rho, float(np.quantile(rho, 0.3)), lat, labels=lab, n=7)
    assert abs(math.fsum(r.volume_by_label) - r.volume) <= 8 * U * r.volume


def test_a_voxel_with_all_24_tetrahedra_inside_gets_one_voxel_volume():
    shape, lat = (6, 7, 5), synth.TRICLINIC
    rho = np.zeros(shape)
    rho[1:4, 2:5, 1:4] = 1.0                    # a 3 x 3 x 3 block: its centre has every neighbour inside
    lab = np.arange(rho.size, dtype=np.int32).reshape(shape)
    r = restate(rho, 0.5, lat, labels=lab, n=rho.size)
    centre = int(np.ravel_multi_index((2, 3, 2), shape))
    assert r.share_count[centre] == 24 and r.share_sum[centre] == 6.0
    vv = cell_volume(lat) / rho.size          # (numpy's LU determinant: a few roundings of its own, as 6 (|det A| / 6) has)
    assert r.volume_by_label[centre] == 6.0 * r.tet and abs(r.volume_by_label[centre] - vv) <= 16 * U * vv
    assert r.share_count[int(np.ravel_multi_index((1, 2, 1), shape))] == 24 and r.share_sum[int(np.ravel_multi_index((1, 2, 1), shape))] < 6.0


def test_colour_is_interpolated_with_the_same_t():
    rho = case('gauss12x10x16')
    g = np.indices(rho.shape)[2].astype(np.float64)           # g = z: the colour of a vertex is its z coordinate, away from the wrap
    r = restate(rho, float(np.quantile(rho, 0.6)), synth.CUBIC6, g=g)
    away = r.vertices[:, 2] < rho.shape[2] - 1
    assert away.any() and np.array_equal(r.colour[away], r.vertices[away, 2])


# ---- the Python layer ---------------------------------------------------------------------------------------------------------------
def read_ply(path):
    with open(path, 'rb') as f:
        raw = f.read()
    head, body = raw.split(b'end_header\n', 1)
    lines = head.decode('ascii').splitlines()
    assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0'
    nv = int(next(ln for ln in lines if ln.startswith('element vertex')).split()[-1])
    nf = int(next(ln for ln in lines if ln.startswith('element face')).split()[-1])
    props = [ln.split()[-1] for ln in lines if ln.startswith('property double')]
    v = np.frombuffer(body, dtype=[(p, '<f8') for p in props], count=nv)
    f = np.frombuffer(body, dtype=[('n', 'u1'), ('v', '<i4', (3,))], count=nf, offset=v.nbytes)
    assert v.nbytes + f.nbytes == len(body) and (f['n'] == 3).all()
    return v, f['v']


@pytest.mark.parametrize('with_colour', [False, True])
def test_write_ply_round_trips(tmp_path, with_colour):
    name = 'gauss12x10x16'
    m = as_mesh(restated_case(name, 'q0.3', with_colour), LAT[name])
    assert (m.wrap != 0).any()
    path = tmp_path / 'mesh.ply'
    m.write_ply(path)
    v, faces = read_ply(path)
    pos = np.stack([v['x'], v['y'], v['z']], axis=1)
    assert np.array_equal(pos[faces], m.corners())                 # the unwrapped triangles, corner by corner
    assert m.vertices.shape[0] < v.shape[0] <= m.vertices.shape[0] + 3 * int((m.wrap != 0).sum())     # duplicates only at the wrap
    if with_colour:
        assert np.array_equal(v['colour'][faces], m.colour[m.triangles])
    edge = np.linalg.norm(m.corners()[:, 1] - m.corners()[:, 0], axis=1)
    assert edge.max() < 0.5 * np.linalg.norm(LAT[name], axis=1).min()        # no triangle spans the cell


def test_positions_use_the_expression_of_critical_positions():
    from pybader_amd import critical
    shape, lat = (5, 7, 11), synth.TRICLINIC
    vox = np.array([[0, 0, 0], [4, 6, 10], [2, 3, 5]], dtype=np.int64)
    assert np.array_equal(isosurface.cartesian(vox.astype(np.float64), shape, lat), critical.positions(vox, shape, lat))


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_isosurface_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_ISO_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_ISO_')}
    assert declared == mirrored == {'XB_ISO_GATHER': 1, 'XB_ISO_TABLE_SIZE': 768}
    assert float(re.search(r'^#define XB_ISO_NCI_RAISED (\S+)', hdr, re.M).group(1)) == _lib.ISO_NCI_RAISED
    want = {
        'xb_isosurface_table': ['uint8_t *out'],
        'xb_isosurface': ['xb_ctx *c', 'const void *field_dev', 'const void *colour_dev', 'const double lattice[9]', 'double level',
                          'int64_t n_labels', 'int flags', 'int64_t counts[2]'],
        'xb_isosurface_fetch': ['xb_ctx *c', 'int on_device', 'void *vertices', 'void *colour', 'void *triangles', 'void *wrap', 'void *cell',
                                'int64_t cap_vertices', 'int64_t cap_triangles', 'double scalars[2]', 'double *volume_by_label',
                                'int64_t cap_labels'],
        'xb_isosurface_release': ['xb_ctx *c'],
        'xb_isosurface_nci_mask': ['xb_ctx *c', 'void *s_dev', 'double rho_cut'],
        'xb_device_write': ['xb_ctx *c', 'void *dev_ptr', 'const void *src_host', 'int64_t bytes'],
        'xb_stream_wait': ['xb_ctx *c', 'void *stream'],
    }
    vp, pi, pd, i64, dbl, i = C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.c_int64, C.c_double, C.c_int
    types_ = {
        'xb_isosurface_table': [vp], 'xb_isosurface': [vp, vp, vp, pd, dbl, i64, i, pi],
        'xb_isosurface_fetch': [vp, i, vp, vp, vp, vp, vp, i64, i64, pd, pd, i64], 'xb_isosurface_release': [vp],
        'xb_isosurface_nci_mask': [vp, vp, dbl], 'xb_device_write': [vp, vp, vp, i64], 'xb_stream_wait': [vp, vp],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, 'include/bader_hip.h does not declare ' + name
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args
        res, argtypes = _lib.SYMBOLS[name]
        assert res is C.c_int and argtypes == types_[name], name
    for method in ('isosurface', 'isosurface_fetch', 'isosurface_release', 'isosurface_nci_mask', 'device_copy'):
        assert callable(getattr(_lib.Context, method))
    assert 'rank of 7 lin(v) + k' in text and re.search(r'^## 21\.', open(os.path.join(ROOT, 'DESIGN.md')).read(), flags=re.M)
    assert _lib.XB_TIMER_COUNT == 11 and not hasattr(_lib, 'XB_TIMER_ISOSURFACE') and not hasattr(_lib, 'XB_OPT_ISOSURFACE')


def test_the_calls_refuse_a_null_context(lib):
    lat = (C.c_double * 9)(*np.eye(3).reshape(-1))
    counts, sc = (C.c_int64 * 2)(), (C.c_double * 2)()
    buf = (C.c_double * 8)()
    assert lib.xb_isosurface(None, None, None, lat, 0.5, 0, 0, counts) == _lib.XB_E_STATE
    assert lib.xb_isosurface_fetch(None, 0, buf, None, buf, buf, buf, 0, 0, sc, None, 0) == _lib.XB_E_STATE
    assert lib.xb_isosurface_release(None) == _lib.XB_E_ARG
    assert lib.xb_isosurface_nci_mask(None, buf, 0.05) == _lib.XB_E_STATE
    assert lib.xb_device_write(None, buf, buf, 8) == _lib.XB_E_ARG
    assert lib.xb_isosurface_table(None) == _lib.XB_E_ARG
    assert lib.xb_stream_wait(None, None) == _lib.XB_E_ARG


def test_bader_has_the_option_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.isosurface_level is None and callable(Bader.isosurface_analysis)


def test_the_calls_need_the_gpu(lib):
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    from pybader_amd import nci
    rho = np.ones((4, 4, 4))
    with pytest.raises(_lib.BaderHipError):
        isosurface.isosurface(rho, np.eye(3), 0.5)
    with pytest.raises(_lib.BaderHipError):
        nci.nci_isosurface(rho, np.eye(3))
