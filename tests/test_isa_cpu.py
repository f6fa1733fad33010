"""The iterative stockholder atoms (pybader_amd/isa.py, xb_isa_setup / xb_isa_iterate) restated in plain numpy from the
definition in include/bader_hip.h / DESIGN.md section 23, and what can be said of the iteration without a GPU.
tests/test_gpu_isa.py compares the kernels with this restatement: counts, qsum rows, tables and the field with ==.

Everything the definition takes from section 19 -- positions, the canonical image list, d2, u, k -- comes from
tests/test_hirshfeld_cpu.py's restatement, operation by operation.  `geometry` keeps, per image of the list, the voxels with
d2 < rc2 and their shells; `iterate` is one iteration: P as the running sum in list order, q = rint(ldexp(rho * (term / P), e)) per
pair into int64 bins, the next tables from bins and counts."""
import ctypes as C
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from pybader_amd import _lib, build, isa, synth
from test_hirshfeld_cpu import LATTICES, U, _positions, image_list

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    build.build_library()
    return _lib.load()


# ---- the definition, restated ---------------------------------------------------------------------------------------------------
def ceil_log2_frexp(x):
    m, ex = math.frexp(x)
    return ex - 1 if m == 0.5 else ex


def exponent(rho_bound, cmax):
    """e = 61 - ceil_log2(rho_bound) - ceil_log2(cmax + 1), with frexp and integers only"""
    return 61 - ceil_log2_frexp(float(rho_bound)) - int(cmax).bit_length()   # ((v - 1).bit_length() of v = cmax + 1)


class Geometry:
    pass


def geometry(shape, lattice, atoms, r_cut, K, widen=0, prefilter=False):
    """-> Geometry: n, K, N, images (a list, in the canonical order, of (a, vox int64[], k int64[]): the voxels with d2 < rc2[a] and
    their shells; images that reach no voxel are left out: they add exact zeros), count i64[n, K].  `prefilter` as
    test_hirshfeld_cpu.restate's: it only saves time on long thin grids."""
    lat = np.asarray(lattice, dtype=np.float64).reshape(9)
    atoms = np.asarray(atoms, dtype=np.float64).reshape(-1, 3)
    n = atoms.shape[0]
    r_cut = np.broadcast_to(np.asarray(r_cut, dtype=np.float64), (n,))
    pc = _positions(shape, lat)
    N = pc[0].size
    rc2 = r_cut * r_cut
    ih2 = np.float64(K) / rc2
    if prefilter:
        B = 256
        nb = -(-N // B)
        pad = [np.concatenate([c, np.full(nb * B - N, c[-1])]).reshape(nb, B) for c in pc]
        centre = [c.mean(axis=1) for c in pad]
        radius = np.sqrt(sum((pad[j] - centre[j][:, None]) ** 2 for j in range(3))).max(axis=1)
    g = Geometry()
    g.n, g.K, g.N, g.images = n, int(K), N, []
    g.count = np.zeros((n, int(K)), np.int64)
    for a, x, y, z in image_list(lattice, atoms, np.arange(n), r_cut, widen):
        q = [atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        if prefilter:
            reach = r_cut[a] + radius
            near = np.sqrt(sum((centre[j] - q[j]) ** 2 for j in range(3))) <= reach + 1e-9 * (1.0 + reach)
            if not near.any():
                continue
            at = np.flatnonzero(np.repeat(near, B)[:N])
        else:
            at = np.arange(N)
        e = [pc[j][at] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        inside = np.flatnonzero(d2 < rc2[a])
        if inside.size:
            u = d2[inside] * ih2[a]
            k = np.minimum(u.astype(np.int64), int(K) - 1)
            g.images.append((int(a), at[inside].astype(np.int64), k))
            g.count[a] += np.bincount(k, minlength=int(K))
    return g


def total(g, A):
    """P: the running sum of the terms A[a][k] in list order (a voxel occurs at most once per image)"""
    P = np.zeros(g.N)
    for a, vox, k in g.images:
        P[vox] = P[vox] + A[a][k]
    return P


def iterate(g, rho, A, e):
    """one iteration -> (A' f64[n, K], bins i64[n, K], qsum i64[n], P of the OLD tables)"""
    rho = np.asarray(rho, dtype=np.float64).reshape(-1)
    P = total(g, A)
    bins = np.zeros(g.n * g.K, np.int64)
    for a, vox, k in g.images:
        term = A[a][k]
        Pv = P[vox]
        sel = (Pv > 0) & (term > 0)
        c = rho[vox[sel]] * (term[sel] / Pv[sel])
        q = np.rint(np.ldexp(c, e)).astype(np.int64)
        np.add.at(bins, a * g.K + k[sel], q)
    bins = bins.reshape(g.n, g.K)
    nxt = np.zeros((g.n, g.K))
    pos = bins > 0
    nxt[pos] = np.ldexp(bins[pos].astype(np.float64) / g.count[pos].astype(np.float64), -e)
    with np.errstate(over='ignore'):
        qsum = bins.sum(axis=1, dtype=np.int64)
    return nxt, bins, qsum, P


def run(g, rho, e, iters, A=None):
    """-> (the qsum rows i64[iters, n], the tables after each iteration)"""
    A = np.ones((g.n, g.K)) if A is None else np.asarray(A, dtype=np.float64)
    rows, tabs = [], []
    for _ in range(iters):
        A, _, qsum, _ = iterate(g, rho, A, e)
        rows.append(qsum)
        tabs.append(A)
    return np.array(rows), tabs


def iterate_scalar(shape, lattice, atoms, r_cut, K, rho, A, e, images):
    """the same, one voxel and image at a time in Python floats and ints -> (A', bins, count)"""
    lat = [float(x) for x in np.asarray(lattice, dtype=np.float64).reshape(9)]
    atoms = [[float(x) for x in at] for at in np.asarray(atoms, dtype=np.float64).reshape(-1, 3)]
    nx, ny, nz = shape
    n = len(atoms)
    rho = np.asarray(rho).reshape(shape)
    bins = [[0] * K for _ in range(n)]
    count = [[0] * K for _ in range(n)]
    for p0 in range(nx):
        for p1 in range(ny):
            for p2 in range(nz):
                pc = []
                for j in range(3):
                    c = lat[j] * p0 / nx
                    c += lat[3 + j] * p1 / ny
                    c += lat[6 + j] * p2 / nz
                    pc.append(c)
                P, pairs = 0.0, []
                for a, x, y, z in images:
                    rc = float(r_cut[a])
                    rc2 = rc * rc
                    ee = [pc[j] - (atoms[a][j] + ((lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z)) for j in range(3)]
                    d2 = (ee[0] * ee[0] + ee[1] * ee[1]) + ee[2] * ee[2]
                    if d2 >= rc2:
                        continue
                    u = d2 * (K / rc2)
                    k = min(int(u), K - 1)
                    term = float(A[a][k])
                    count[a][k] += 1
                    P += term
                    pairs.append((a, k, term))
                if P > 0:
                    for a, k, term in pairs:
                        if term > 0:
                            c = float(rho[p0, p1, p2]) * (term / P)
                            bins[a][k] += int(np.rint(math.ldexp(c, e)))   # (np.rint: to nearest, ties to even)
    nxt = [[math.ldexp(float(bins[a][k]) / float(count[a][k]), -e) if bins[a][k] > 0 else 0.0 for k in range(K)] for a in range(n)]
    return np.array(nxt), np.array(bins, np.int64), np.array(count, np.int64)


# ---- inputs (shared with tests/test_gpu_isa.py) -------------------------------------------------------------------------------
# name -> (shape, lattice, atoms, r_cut, K, the route its tiles take)
CASES = {
    'cubic_r2_k16': ((24, 24, 24), 'cubic', 'atoms8', 2.0, 16, 'candidate'),
    'tric_r2_k64': ((24, 24, 24), 'tric', 'atoms8', 2.0, 64, 'candidate'),
    'cubic_r3_k64': ((24, 24, 24), 'cubic', 'atoms8', 3.0, 64, 'candidate'),
    'tric_r3_k16': ((24, 24, 24), 'tric', 'atoms8', 3.0, 16, 'candidate'),
    'tric_r3_k64': ((24, 24, 24), 'tric', 'atoms8', 3.0, 64, 'candidate'),      # (the CPU tests' second ML-EM input)
    # many more shells than a wave's LDS window has bins (ISA_WIN, csrc/k_isa.h): pairs beyond the window go out directly
    'wide_k2048': ((24, 24, 24), 'tric', 'atoms8', 3.0, 2048, 'candidate'),
    'odd_k1': ((20, 9, 33), 'cubic', 'atoms8', 3.0, 1, 'candidate'),
    'three': ((3, 3, 3), 'tric', 'atoms8', 3.0, 16, 'candidate'),
    'thin': ((1, 2, 9), 'cubic', 'atoms8', 2.0, 16, 'candidate'),
    'one': ((1, 1, 1), 'tric', 'atoms8', 3.0, 8, 'candidate'),
    'more_overflow': ((16, 16, 16), 'cubic', 'grid343', 3.0, 32, 'overflow'),
    'more_candidate': ((24, 24, 24), 'cubic', 'grid343', 1.0, 32, 'candidate'),
    'line': ((1, 1, 160000), 'cubic', 'atoms8', 2.2, 64, 'candidate'),
    'negative': ((24, 24, 24), 'tric', 'atoms8', 3.0, 64, 'candidate'),
}
LONG = ('line',)


@functools.lru_cache(maxsize=None)
def case(name):
    """one input of the GPU tests: shape, lattice, atoms (Cartesian), r_cut, K, rho, bound -- built once, never written"""
    shape, lname, kind, r_cut, K, route = CASES[name]
    c = Geometry()
    c.name, c.shape, c.lattice, c.route, c.K = name, shape, LATTICES[lname], route, K
    if kind == 'grid343':
        a5 = synth.atoms_jittered_grid(7)
        c.rho = synth.synth_density(shape, c.lattice, a5)
    else:
        a5 = synth.ATOMS8
        c.rho = synth.synth_density(shape, c.lattice, a5) - synth.BACKGROUND
    c.atoms = np.ascontiguousarray(a5[:, :3] @ c.lattice)
    if name == 'thin':
        c.atoms = c.atoms.copy()
        c.atoms[2] += c.lattice[0] - 2 * c.lattice[2]      # an atom outside the cell: taken as given
    if name == 'negative':
        # a fifth of the voxels at -1.5 times their value: some shells sum below zero, clamp to zero and stay zero (19 after
        # the first iteration, 75 of 512 after the seventh)
        c.rho = np.ascontiguousarray(c.rho * (1.0 - 2.5 * (synth.hash_noise(shape, 11) < 0.2)))
    c.r_cut = np.full(c.atoms.shape[0], float(r_cut))
    c.bound = float(np.abs(c.rho).max())
    for a in (c.atoms, c.rho, c.r_cut):
        a.flags.writeable = False
    return c


@functools.lru_cache(maxsize=None)
def geo(name):
    c = case(name)
    return geometry(c.shape, c.lattice, c.atoms, c.r_cut, c.K, prefilter=name in LONG)


@functools.lru_cache(maxsize=None)
def reference(name, iters=7):
    """(e, qsum rows, the tables after each iteration) of one input, computed once and never written"""
    c, g = case(name), geo(name)
    e = exponent(c.bound, g.count.max())
    rows, tabs = run(g, c.rho, e, iters)
    return e, rows, tabs


# ---- the restatement itself -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('lname', ['cubic', 'tric'])
def test_restatement_against_a_scalar_triple_loop(lname):
    shape, lat, K = (5, 7, 11), LATTICES[lname], 6
    atoms = synth.ATOMS8[:, :3] @ lat
    r_cut = np.array([2.5, 2.0, 3.0, 1.5, 2.5, 2.2, 1.0, 2.8])
    rho = synth.synth_density(shape, lat, synth.ATOMS8) - synth.BACKGROUND
    g = geometry(shape, lat, atoms, r_cut, K)
    e = exponent(np.abs(rho).max(), g.count.max())
    images = image_list(lat, atoms, np.arange(8), r_cut).tolist()
    A = np.ones((8, K))
    for it in range(3):
        nxt, bins, qsum, _ = iterate(g, rho, A, e)
        nxt_s, bins_s, count_s = iterate_scalar(shape, lat, atoms, r_cut, K, rho, A, e, images)
        assert np.array_equal(g.count, count_s) and np.array_equal(bins, bins_s), (lname, it)
        assert np.array_equal(nxt.view(np.uint64), nxt_s.view(np.uint64)), (lname, it)
        assert np.array_equal(qsum, bins.sum(axis=1))
        A = nxt
    assert (g.count > 0).any(axis=1).all() and (A > 0).any()


@pytest.mark.parametrize('name', ['cubic_r2_k16', 'tric_r3_k16', 'thin', 'three'])
def test_counts_against_a_brute_force_over_a_wider_image_range(name):
    """every (voxel, image) pair over a range three shifts wider at either end, one dense d2 matrix: the same counts"""
    c, g = case(name), geo(name)
    lat = np.asarray(c.lattice, dtype=np.float64).reshape(9)
    pc = _positions(c.shape, lat)
    wide = image_list(c.lattice, c.atoms, np.arange(c.atoms.shape[0]), c.r_cut, widen=3)
    assert wide.shape[0] > 3 * image_list(c.lattice, c.atoms, np.arange(c.atoms.shape[0]), c.r_cut).shape[0]
    count = np.zeros_like(g.count)
    for a, x, y, z in wide:
        q = [c.atoms[a, j] + ((lat[j] * np.float64(x) + lat[3 + j] * np.float64(y)) + lat[6 + j] * np.float64(z)) for j in range(3)]
        e = [pc[j] - q[j] for j in range(3)]
        d2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
        rc2 = c.r_cut[a] * c.r_cut[a]
        k = np.minimum((d2[d2 < rc2] * (np.float64(c.K) / rc2)).astype(np.int64), c.K - 1)
        count[a] += np.bincount(k, minlength=c.K)
    assert np.array_equal(count, g.count) and count.sum() > 0
    g2 = geometry(c.shape, c.lattice, c.atoms, c.r_cut, c.K, widen=2)
    assert np.array_equal(g2.count, g.count)


def test_the_prefilter_changes_no_count_and_no_bit():
    c = case('tric_r2_k64')
    g, g2 = geo('tric_r2_k64'), geometry(c.shape, c.lattice, c.atoms, c.r_cut, c.K, prefilter=True)
    assert np.array_equal(g.count, g2.count)
    e = exponent(c.bound, g.count.max())
    a, b = run(g, c.rho, e, 2), run(g2, c.rho, e, 2)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1][-1].view(np.uint64), b[1][-1].view(np.uint64))


def test_the_exponent_from_frexp_against_exact_integers():
    """ceil_log2 by frexp equals the least c with x <= 2^c in exact rational arithmetic, at powers of two and their neighbours"""
    for p in list(range(-1074, -1060)) + list(range(-70, 70)) + list(range(1010, 1024)):
        x = math.ldexp(1.0, p)
        for v in (x, np.nextafter(x, 0.0), np.nextafter(x, np.inf)):
            v = float(v)
            if not (v > 0 and math.isfinite(v)):
                continue
            c = ceil_log2_frexp(v)
            assert Fraction(v) <= Fraction(2) ** c and Fraction(v) > Fraction(2) ** (c - 1), (p, v)
    for cmax in [0, 1, 2, 3, 4, 7, 8, 9, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 40 - 1, 2 ** 40]:
        c = int(cmax).bit_length()
        assert cmax + 1 <= 2 ** c and (c == 0 or cmax + 1 > 2 ** (c - 1))
    # no bin can reach 2^62: cmax pairs of at most rint(rho_bound 2^e) each
    for bound in (1e-300, 0.7, 1.0, 1.5, 7.5, 1e6, 1e300):
        for cmax in (0, 1, 5, 8, 13824, 2 ** 33):
            e = exponent(bound, cmax)
            assert max(cmax, 1) * (math.floor(Fraction(bound) * Fraction(2) ** e) + 1) < 2 ** 62
    assert exponent(1.0, 0) == 61 and exponent(2.0, 1) == 59 and exponent(0.5, 3) == 60 and exponent(3.0, 4) == 56


def test_the_pair_A_zero_gives_A_exactly_through_the_term_of_section_19():
    """term = f[k] + t*(f[k+1] - f[k]) with the pair (A, +0.0): A + t*0.0 == A bit for bit, for every t the last shell's clamp allows"""
    A = np.array([0.0, 5e-324, 2.2250738585072014e-308, 1e-17, 0.1, 1.0, 1.5, 7.5, 1e300, 1.7976931348623157e308])
    t = np.array([0.0, 5e-324, 1e-9, 0.5, np.nextafter(1.0, 0.0), 1.0, 2.5, 1e6])
    got = A[:, None] + t[None, :] * np.float64(0.0)
    assert np.array_equal(got.view(np.uint64), np.broadcast_to(A[:, None], got.shape).view(np.uint64))
    # and through the restated total: with every table constant the field is a count of images times that constant
    c, g = case('three'), geo('three')
    P = total(g, np.full((g.n, g.K), 0.25))
    reach = np.zeros(g.N, np.int64)
    for _, vox, _ in g.images:
        reach[vox] += 1
    assert np.array_equal(P, 0.25 * reach)


def isa_win():
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_isa.h')).read()
    return int(re.search(r'#define ISA_WIN (\d+)', src).group(1))


def wave_spans(shape, g):
    """per image of the list and per wave of csrc/k_isa.h (wave w of an 8^3 tile takes its x-planes w and w + 4) that the image
    reaches: the largest shell minus the smallest among the wave's voxels -> all of them, one array"""
    nt = [-(-s // 8) for s in shape]
    out = []
    for _, vox, k in g.images:
        x, y, z = np.unravel_index(vox, shape)
        wid = (((x // 8) * nt[1] + y // 8) * nt[2] + z // 8) * 4 + x % 4
        lo, hi = np.full(4 * nt[0] * nt[1] * nt[2], g.K), np.full(4 * nt[0] * nt[1] * nt[2], -1)
        np.minimum.at(lo, wid, k)
        np.maximum.at(hi, wid, k)
        out.append((hi - lo)[hi >= 0])
    return np.concatenate(out)


def test_the_wide_case_leaves_the_window_and_the_others_stay_inside():
    """the default route keeps shells kmin .. kmin + ISA_WIN - 1 of an image in a wave's LDS window and sends the others out
    directly; 'wide_k2048' is the input whose waves do both, every other input's waves stay inside (K <= 64)"""
    W = isa_win()
    spans = wave_spans(case('wide_k2048').shape, geo('wide_k2048'))
    print(f'wide_k2048: {spans.size} (image, wave) runs, {int((spans >= W).sum())} reach beyond a window of {W}, the widest spans {int(spans.max())} shells')
    assert (spans >= W).sum() > spans.size // 10 and (spans < W).sum() > spans.size // 10 and spans.max() >= 2 * W
    for name in CASES:
        if name != 'wide_k2048':
            assert CASES[name][4] <= W and wave_spans(case(name).shape, geo(name)).max() < W, name


# ---- ML-EM ----------------------------------------------------------------------------------------------------------------------
EM_CASES = ['cubic_r3_k64', 'tric_r3_k64']


@pytest.mark.parametrize('name', EM_CASES)
def test_every_iteration_keeps_the_shell_sums(name):
    """A'[a][k] = fl(fl(bin) / fl(count)) 2^-e: one rounding of the int64 -> float64 conversion (bins may exceed 2^53) and one of the
    division, so in exact arithmetic |A' count 2^e - bin| <= (2 u + u^2) bin per shell, and summed over the shells."""
    c, g = case(name), geo(name)
    e = exponent(c.bound, g.count.max())
    A = np.ones((g.n, g.K))
    for it in range(4):
        A, bins, _, _ = iterate(g, c.rho, A, e)
        lhs = sum(Fraction(float(A[a, k])) * int(g.count[a, k]) * Fraction(2) ** e for a in range(g.n) for k in range(g.K))
        rhs = int(bins.sum())
        lim = (2 * Fraction(U) + Fraction(U) ** 2) * int(np.abs(bins).sum())
        assert (bins >= 0).all() and abs(lhs - rhs) <= lim, (name, it, float(abs(lhs - rhs)), float(lim))


@pytest.mark.parametrize('name', EM_CASES)
def test_the_fixed_point_charges_sum_to_the_density(name):
    """BOUND, stated before running.  At a voxel with P > 0 and m pairs with term > 0 the shares are q_i = rint(rho 2^e w_i),
    w_i = fl(term_i / P).  P is the running sum of the m terms: relative error at most (m - 1) u; each w_i one more u, the product
    rho w_i another: sum_i fl(rho w_i) = rho (1 + theta), |theta| <= (m + 2) u (to first order; asserted with a factor 1 + 2^-40).
    Each rint moves a share by at most half a quantum, rint(rho 2^e) itself by half: at most one quantum per pair in all (m >= 1).
    So  |sum_a qsum[a] - sum_{v: P > 0} rint(rho 2^e)| <= sum_v [ m_v + |rho_v| 2^e (m_v + 2) u ]."""
    c, g = case(name), geo(name)
    rho = c.rho.reshape(-1)
    e = exponent(c.bound, g.count.max())
    A = np.ones((g.n, g.K))
    for it in range(3):
        old = A
        A, bins, qsum, P = iterate(g, rho, A, e)
        m = np.zeros(g.N, np.int64)
        for a, vox, k in g.images:
            m[vox] += old[a][k] > 0
        have = P > 0
        assert (rho[have] >= 0).all() and (m[have] >= 1).all()
        want = int(np.rint(np.ldexp(rho[have], e)).astype(np.int64).sum())
        lim = int(m[have].sum()) + float((np.ldexp(np.abs(rho[have]), e) * (m[have] + 2) * U).sum()) * (1 + 2.0 ** -40)
        got = int(qsum.sum())
        print(f'{name} iteration {it}: sum qsum - sum rint(rho 2^e) = {got - want}, bound {lim:.3e}')
        assert abs(got - want) <= lim


@pytest.mark.parametrize('name', EM_CASES)
def test_the_i_divergence_does_not_increase(name):
    """On a uniform grid with piecewise-constant shells the iteration is ML-EM for the model P = sum of the shells' indicator
    functions times A[a][k]: A' = A * (sum over the shell's pairs of rho / P) / count.  The I-divergence sum_v [rho ln(rho / P)
    - rho + P] over the covered voxels therefore never increases.  Allowed: the float64 sum bound of section 13, (N + 2) u times the
    sum of the magnitudes |rho ln(rho / P)| + |rho| + |P|, for each of the two sums compared."""
    c, g = case(name), geo(name)
    rho = c.rho.reshape(-1)
    e = exponent(c.bound, g.count.max())

    def divergence(P):
        have = P > 0
        assert have.all() and (rho >= 0).all()
        pos = rho > 0
        t = np.zeros(g.N)
        t[pos] = rho[pos] * np.log(rho[pos] / P[pos])
        return math.fsum(t) - math.fsum(rho) + math.fsum(P), (g.N + 2) * U * float((np.abs(t) + np.abs(rho) + np.abs(P)).sum())

    A = np.ones((g.n, g.K))
    last = None
    for it in range(12):
        d = divergence(total(g, A))
        if last is not None:
            print(f'{name} iteration {it}: I-divergence {d[0]!r} after {last[0]!r}')
            assert d[0] <= last[0] + d[1] + last[1], (name, it)
        last = d
        A = iterate(g, rho, A, e)[0]
    assert last[0] < 0.01 * divergence(total(g, np.ones((g.n, g.K))))[0], 'and it falls a long way'


# ---- the one tolerance that cannot be derived ---------------------------------------------------------------------------------
def restated_charges(g, rho, A, vv):
    """charge per atom on the tables A: sum_v rho p_a / P, by fsum"""
    P = total(g, A)
    p = np.zeros((g.n, g.N))
    for a, vox, k in g.images:
        p[a][vox] = p[a][vox] + A[a][k]
    have = P > 0
    w = np.zeros_like(p)
    w[:, have] = p[:, have] / P[have]
    return np.array([math.fsum(rho * x) for x in w]) * vv, np.array([math.fsum(x) for x in w]) * vv, w


@functools.lru_cache(maxsize=None)
def converged(name, tol=1e-6, max_iter=2000):
    c, g = case(name), geo(name)
    vv = abs(np.linalg.det(c.lattice)) / g.N
    e = exponent(c.bound, g.count.max())
    A, last, it = np.ones((g.n, g.K)), None, 0
    while it < max_iter:
        A, _, qsum, _ = iterate(g, c.rho, A, e)
        it += 1
        row = qsum.astype(np.float64) * (math.ldexp(1.0, -e) * vv)
        if last is not None and np.max(np.abs(row - last)) < tol:
            break
        last = row
    return A, it, vv


MEASURED_ISA_DISTANCE = 1.18e-3   # measured on the CPU (the numpy restatement), see the test below


def test_isa_charges_of_overlapping_synth_atoms_against_their_own_integrals():
    """synth_density(24^3) - BACKGROUND in the cubic cell is the sum of eight overlapping atoms A g(r^2), each with the known integral
    A pi^(3/2) R^3 Gamma(1025) / Gamma(1026.5), R^2 = 2048 s^2.  ISA (the numpy restatement run to tol = 1e-6, r_cut = 3, K = 64)
    shares the density among spherical atoms; how far its charges lie from the atoms' own integrals follows from no bound -- it is
    what the method does with overlapping tails on a 0.25 A grid with 64 shells.
    MEASURED ON THE CPU (numpy restatement, 286 iterations): max_a |q_a - integral_a| = 1.18e-3 of charges between 1.17 and 13.26
    (atom 7; 0.07 % of the smallest charge, atom 6, which is off by 8.2e-4); asserted at TWICE the measured value, a margin for
    nothing but a change of K default rounding."""
    name = 'cubic_r3_k64'
    c, g = case(name), geo(name)
    A, it, vv = converged(name)
    charge, _, _ = restated_charges(g, c.rho.reshape(-1), A, vv)
    exact = np.array([amp * math.pi ** 1.5 * (2048 * sg * sg) ** 1.5 * math.exp(math.lgamma(1025) - math.lgamma(1026.5))
                      for _, _, _, sg, amp in synth.ATOMS8])
    dist = np.abs(charge - exact)
    print(f'{name}: {it} iterations; ISA {charge.round(5).tolist()}; integrals {exact.round(5).tolist()}; max distance {dist.max():.4e}')
    assert it < 2000
    assert dist.max() <= 2 * MEASURED_ISA_DISTANCE


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_isa_names():
    text = open(os.path.join(ROOT, 'include', 'bader_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = [e.strip() for body in re.findall(r'enum\s*\{([^}]*)\}', hdr) for e in body.split(',') if e.strip().startswith('XB_ISA_')]
    declared = {name: int(value) for name, value in (re.fullmatch(r'(\w+)\s*=\s*(\d+)', e).groups() for e in names)}
    mirrored = {name: getattr(_lib, name) for name in dir(_lib) if name.startswith('XB_ISA_')}
    assert declared == mirrored == {'XB_ISA_DIRECT': 2, 'XB_ISA_ITERS_MAX': 64}
    assert _lib.XB_ISA_DIRECT & _lib.XB_HIRSHFELD_FULL_SEARCH == 0
    want = {
        'xb_isa_setup': ['xb_ctx *c', 'const double lattice[9]', 'const double *atoms_cart', 'int64_t n', 'const double *r_cut',
                         'int64_t shells', 'const double *initial', 'double rho_bound', 'int64_t out_info[4]'],
        'xb_isa_iterate': ['xb_ctx *c', 'int64_t iters', 'int flags', 'int64_t *qsum_out', 'int64_t stats[4]'],
        'xb_isa_tables': ['xb_ctx *c', 'double *A_out', 'int64_t *count_out'],
        'xb_isa_load': ['xb_ctx *c', 'const double *tables'],
        'xb_isa_rho_bound': ['xb_ctx *c', 'double *out'],
    }
    for name, args in want.items():
        m = re.search(r'\bint\s+%s\s*\(([^)]*)\)\s*;' % name, hdr)
        assert m, f'include/bader_hip.h does not declare {name}'
        assert [re.sub(r'\s+', ' ', a).strip() for a in m.group(1).split(',')] == args, name
        assert _lib.SYMBOLS[name][0] is C.c_int and len(_lib.SYMBOLS[name][1]) == len(args)
    for method in ('isa_setup', 'isa_iterate', 'isa_tables', 'isa_load', 'density_absmax'):
        assert callable(getattr(_lib.Context, method))
    design = open(os.path.join(ROOT, 'DESIGN.md')).read()
    for line in ('q = llrint(ldexp(c, e))', 'e = 61 - ceil_log2(rho_bound) - ceil_log2(cmax + 1)'):
        assert line in text and line in design, line
    assert '## 23.' in design
    src = open(os.path.join(ROOT, 'pybader_amd', 'csrc', 'k_isa.h')).read()
    assert '#define ISA_WIN 256' in src
    assert _lib.XB_TIMER_COUNT == 11, 'no timer slot came with it'


def test_the_library_exports_the_calls(lib):
    for name in ('xb_isa_setup', 'xb_isa_iterate', 'xb_isa_tables', 'xb_isa_load', 'xb_isa_rho_bound'):
        assert getattr(lib, name) is not None
    # a null context is an argument error in all four, found before anything else
    assert lib.xb_isa_setup(None, None, None, 1, None, 1, None, 1.0, None) == _lib.XB_E_ARG
    assert lib.xb_isa_iterate(None, 1, 0, None, None) == _lib.XB_E_ARG
    assert lib.xb_isa_tables(None, None, None) == _lib.XB_E_ARG
    assert lib.xb_isa_load(None, None) == _lib.XB_E_ARG
    assert lib.xb_isa_rho_bound(None, None) == _lib.XB_E_ARG


def test_default_shells():
    assert isa.default_shells(synth.CUBIC6, (24, 24, 24), [3.0]) == 36           # (3 / 0.5)^2
    assert isa.default_shells(synth.CUBIC6, (512, 512, 512), [3.0, 2.0]) == 4096  # (2 / 0.0234)^2 = 7281, clamped
    assert isa.default_shells(synth.CUBIC6, (8, 8, 8), [1.0]) == 8                # (1 / 1.5)^2 = 0, clamped
    assert isa.default_shells(synth.CUBIC6, (24, 48, 24), [3.0]) == 36            # the LONGEST voxel edge


def test_bader_has_the_flag_and_it_is_off():
    from pybader_amd.interface import Bader
    assert Bader.isa_flag is False and callable(Bader.isa_analysis)
    assert Bader.isa_r_cut == 3.0 and Bader.isa_shells is None and Bader.isa_tol == 1e-6


def test_isa_charges_need_the_gpu(lib):
    """without a GPU the call fails loudly (no fallback); with one it answers"""
    c = case('three')
    if lib.xb_device_count() > 0:
        r = isa.isa_charges(c.rho, c.lattice, c.atoms, 1.0, r_cut=3.0, shells=16, max_iter=3)
        assert r.charge.shape == (8,) and r.iterations == 3
        return
    with pytest.raises(_lib.BaderHipError):
        isa.isa_charges(c.rho, c.lattice, c.atoms, 1.0, r_cut=3.0, shells=16, max_iter=3)
