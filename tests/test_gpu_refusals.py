"""The refusals of the analyses' entry points, as a whole: every call below must be refused before anything is launched, and its
code and its xb_last_error text are compared with tests/golden/refusals.json (pointers in the text replaced by a fixed token).

States: a null context, a context without a grid, a 6 x 5 x 4 grid (the smallest that is thin on no axis) held as the slab [0, 3),
the whole grid without a density, with a density and without labels, and with both.  On the last one: device arrays misaligned by
one byte, device arrays that overlap the resident density or labels (or each other), and each call's own argument refusals taken
together -- a null argument against unknown flag bits against a bad count -- so that the file also pins which refusal wins.

`python tests/test_gpu_refusals.py --record [PATH]` writes the file from the library as it is built."""
import ctypes as C
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'refusals.json')
SHAPE, SLAB = (6, 5, 4), (0, 3)
N = SHAPE[0] * SHAPE[1] * SHAPE[2]
XB_F64, BAD_FLAGS = 64, 0x40

pytestmark = pytest.mark.gpu


class Env:
    """a context of its own and the arguments every call is made with; nothing here is ever written: every call is refused"""

    def __init__(self):
        from pybader_amd import _lib, device
        self.L, self.ctx = _lib, _lib.Context(0)
        self.lib, self.h = self.ctx.lib, self.ctx.h
        self.lat = np.diag([3., 2.5, 2.]).ravel().copy()
        self.alpha = np.zeros(27)
        self.pts = np.ones((2, 3))
        self.dirs = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1]], np.int32)
        self.idx = np.array([0, N // 2], np.int64)
        self.species = np.zeros(2, np.int32)
        self.tables = np.array([1., .5, 0.])
        self.r_cut = np.ones(1)
        self.edges = np.array([0., 1., 2.])
        self.stride = np.array([SHAPE[1] * SHAPE[2], SHAPE[2], 1], np.int64)
        self.f8, self.i8, self.i4 = np.zeros(4 * N), np.zeros(4 * N, np.int64), np.zeros(4 * N, np.int32)
        self.dev = [device.DeviceArray(self.ctx, (N + 8,), np.float64) for _ in range(2)]

    def close(self):
        self.dev = None
        self.ctx.close()


def d(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def q(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64))


def v(a):
    return None if a is None else (C.c_void_p(a) if isinstance(a, int) else a.ctypes.data_as(C.c_void_p))


# every call: (e, h, null, flags, n, **device pointers) -> code.  `null` takes one required pointer away, `flags` go in as they
# are, `n` is the call's count of labels / atoms / voxels (None: a valid one)
def weight_sum(e, h, null=False, flags=0, n=None):
    return e.lib.xb_weight_sum(h, None if null else d(e.alpha), 1., None, q(e.i8))


def weight_sum_device(e, h, null=False, flags=0, n=None, ptr=None, dtype=XB_F64):
    return e.lib.xb_weight_sum_device(h, d(e.alpha), 1., v(e.dev[0].ptr if ptr is None else ptr), dtype, None if null else q(e.stride), None, q(e.i8))


def weight_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_weight_fetch(h, v(e.i8), v(e.f8), v(e.f8), N)


def weight_stats(e, h, null=False, flags=0, n=None):
    return e.lib.xb_weight_stats(h, None if null else q(e.i8))


def moment_sum(e, h, null=False, flags=0, n=None):
    return e.lib.xb_moment_sum(h, None if null else d(e.lat), d(e.pts), 2 if n is None else n, 1., d(e.f8), d(e.f8))


def adjacency(e, h, null=False, flags=0, n=None, n_dirs=3):
    return e.lib.xb_adjacency(h, None if null else v(e.dirs), n_dirs, 2 if n is None else n, q(e.i8))


def adjacency_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_adjacency_fetch(h, None if null else v(e.i4), v(e.i4), v(e.i8), v(e.f8), v(e.i8), N)


def merge_basins(e, h, null=False, flags=0, n=None, n_dirs=3, rounds=64, tol=1.):
    out = (C.c_int64(), C.c_int64(), C.c_int())
    return e.lib.xb_merge_basins(h, v(e.dirs), n_dirs, 2 if n is None else n, None if null else v(e.idx), tol, rounds, C.byref(out[0]), C.byref(out[1]),
                                 C.byref(out[2]))


def merge_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_merge_fetch(h, None if null else v(e.i4), v(e.i4), v(e.f8), N)


def voronoi_assign(e, h, null=False, flags=0, n=None):
    return e.lib.xb_voronoi_assign(h, None if null else d(e.lat), d(e.pts), 2 if n is None else n, 0., flags, q(e.i8))


def critical_points(e, h, null=False, flags=0, n=None):
    return e.lib.xb_critical_points(h, float('nan'), flags, None if null else q(e.i8), q(e.i8))


def critical_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_critical_fetch(h, None if null else v(e.i8), v(e.i4), v(e.i4), v(e.i4), N)


def critical_bonds(e, h, null=False, flags=0, n=None):
    return e.lib.xb_critical_bonds(h, 2 if n is None else n, None if null else q(e.i8), q(e.i8))


def critical_bonds_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_critical_bonds_fetch(h, None if null else v(e.i4), v(e.i4), v(e.i8), v(e.f8), v(e.i8), N)


def laplacian_field(e, h, null=False, flags=0, n=None, host=True, dev=None):
    return e.lib.xb_laplacian_field(h, None if null else d(e.lat), flags, v(e.f8) if host else None, v(dev))


def laplacian_sum(e, h, null=False, flags=0, n=None):
    return e.lib.xb_laplacian_sum(h, None if null else d(e.lat), 2 if n is None else n, 1., flags, d(e.f8), d(e.f8), d(e.f8))


def stencil_points(e, h, null=False, flags=0, n=None):
    return e.lib.xb_stencil_points(h, None if null else d(e.lat), v(e.i8), 2 if n is None else n, v(e.f8))


def nci_field(e, h, null=False, flags=0, n=None, host=True, s_dev=None, x_dev=None):
    return e.lib.xb_nci_field(h, None if null else d(e.lat), flags, v(e.f8) if host else None, v(e.f8) if host else None, v(s_dev), v(x_dev))


def nci_sum(e, h, null=False, flags=0, n=None, s_cut=.5):
    return e.lib.xb_nci_sum(h, None if null else d(e.lat), 2 if n is None else n, 1., s_cut, .1, .01, flags, q(e.i8), d(e.f8), d(e.f8))


def nci_hist(e, h, null=False, flags=0, n=None):
    return e.lib.xb_nci_hist(h, None if null else d(e.lat), d(e.edges), 2 if n is None else n, d(e.edges), 2, flags, q(e.i8))


def hirshfeld_setup(e, h, null=False, flags=0, n=None, knots=2):
    return e.lib.xb_hirshfeld_setup(h, d(e.lat), d(e.pts), v(e.species), 2 if n is None else n, None if null else d(e.tables), d(e.r_cut), 1, knots)


def hirshfeld_sum(e, h, null=False, flags=0, n=None):
    return e.lib.xb_hirshfeld_sum(h, 1., flags, None if null else d(e.f8), d(e.f8), d(e.f8), q(e.i8))


def hirshfeld_field(e, h, null=False, flags=0, n=None, mode=1, host=True, dev=None):
    return e.lib.xb_hirshfeld_field(h, mode, flags, v(e.f8) if host else None, v(dev))


def isosurface(e, h, null=False, flags=0, n=None, field=None, colour=None, level=.5):
    return e.lib.xb_isosurface(h, v(field), v(colour), None if null else d(e.lat), level, 2 if n is None else n, flags, q(e.i8))


def isosurface_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_isosurface_fetch(h, 0, None if null else v(e.f8), None, v(e.i8), v(e.i4), v(e.i8), N, N, d(e.f8), d(e.f8), N)


def isosurface_nci_mask(e, h, null=False, flags=0, n=None, dev=-1, rho_cut=.1):
    return e.lib.xb_isosurface_nci_mask(h, v(None if null else (e.dev[0].ptr if dev == -1 else dev)), rho_cut)


def regions_label(e, h, null=False, flags=0, n=None, mode=0, field=None, nci_lattice=True):
    return e.lib.xb_regions_label(h, mode, v(field), .5, d(e.lat) if nci_lattice else None, .5, .1, flags, None if null else q(e.i8))


def regions_sums(e, h, null=False, flags=0, n=None):
    return e.lib.xb_regions_sums(h, 1., float('nan'), None if null else q(e.i8), q(e.i8), q(e.i8), d(e.f8), d(e.f8), None, None, None, N)


def regions_shares(e, h, null=False, flags=0, n=None):
    return e.lib.xb_regions_shares(h, 2 if n is None else n, flags, None if null else q(e.i8))


def regions_shares_fetch(e, h, null=False, flags=0, n=None):
    return e.lib.xb_regions_shares_fetch(h, None if null else v(e.i4), v(e.i4), q(e.i8), N)


def regions_fetch_map(e, h, null=False, flags=0, n=None):
    return e.lib.xb_regions_fetch_map(h, 0, None if null else v(e.i4))


def regions_times(e, h, null=False, flags=0, n=None):
    return e.lib.xb_regions_times(h, None if null else d(e.f8))


def import_labels(e, h, null=False, flags=0, n=None, ptr=None, dtype=4):
    return e.lib.xb_import_labels(h, v(e.dev[0].ptr if ptr is None else ptr), dtype, None)


def export_labels(e, h, null=False, flags=0, n=None, ptr=None, dtype=4):
    return e.lib.xb_export_labels(h, v(e.dev[0].ptr if ptr is None else ptr), dtype, None)


def release(name):
    def call(e, h, null=False, flags=0, n=None):
        return getattr(e.lib, f'xb_{name}_release')(h)
    call.__name__ = f'{name}_release'
    return call


RELEASES = [release(a) for a in ('weight', 'adjacency', 'merge', 'critical', 'hirshfeld', 'isosurface', 'regions')]
FETCHES = [weight_fetch, adjacency_fetch, merge_fetch, critical_fetch, critical_bonds_fetch, isosurface_fetch, regions_sums, regions_shares,
           regions_shares_fetch, regions_fetch_map, regions_times]
CALLS = [weight_sum, weight_sum_device, moment_sum, adjacency, merge_basins, voronoi_assign, critical_points, critical_bonds, laplacian_field,
         laplacian_sum, stencil_points, nci_field, nci_sum, nci_hist, hirshfeld_setup, hirshfeld_sum, hirshfeld_field, isosurface,
         isosurface_nci_mask, regions_label]
# (the fetches of a context that holds no result are refused in every state; import_labels / export_labels take a null context as "no grid")
NO_GRID = CALLS + FETCHES + [import_labels, export_labels]
NULL_CTX = NO_GRID + RELEASES + [weight_stats]
NOT_ON_A_SLAB = {moment_sum}                                  # xb_moment_sum sums over the owned planes of a slab
NO_DENSITY_NEEDED = {weight_sum, weight_sum_device, hirshfeld_setup}   # (the weight method takes what the card holds)
READS_LABELS = [moment_sum, adjacency, merge_basins, critical_bonds, laplacian_sum, nci_sum, isosurface]
# the knobs of a call that can collide: every non-empty subset of them is a case
KNOBS = {
    weight_sum: ['null'], weight_sum_device: ['null', 'dtype'], weight_stats: ['null'], moment_sum: ['null', 'n'],
    adjacency: ['null', 'n', 'n_dirs'], merge_basins: ['null', 'n', 'n_dirs', 'rounds', 'tol'], voronoi_assign: ['null', 'n', 'flags'],
    critical_points: ['null', 'flags'], critical_bonds: ['null', 'n'], laplacian_field: ['null', 'flags', 'both'],
    laplacian_sum: ['null', 'flags', 'n'], stencil_points: ['null', 'n'], nci_field: ['null', 'flags', 'both'], nci_sum: ['null', 'flags', 'n', 's_cut'],
    nci_hist: ['null', 'flags', 'n'], hirshfeld_setup: ['null', 'n', 'knots'], hirshfeld_sum: ['null', 'flags'], hirshfeld_field: ['mode', 'flags', 'both'],
    isosurface: ['null', 'flags', 'n', 'level'], isosurface_nci_mask: ['null', 'rho_cut'], regions_label: ['null', 'flags', 'mode'],
}
KNOB_VALUES = {'null': {'null': True}, 'flags': {'flags': BAD_FLAGS}, 'n': {'n': -1}, 'n_dirs': {'n_dirs': 0}, 'rounds': {'rounds': 0},
               'tol': {'tol': float('nan')}, 'dtype': {'dtype': 16}, 's_cut': {'s_cut': -1.}, 'knots': {'knots': 0}, 'mode': {'mode': 7},
               'level': {'level': float('inf')}, 'rho_cut': {'rho_cut': float('nan')}}


def knob_cases(e):
    for call, knobs in KNOBS.items():
        for k in range(1, len(knobs) + 1):
            for subset in itertools.combinations(knobs, k):
                kw = {}
                for knob in subset:
                    # both outputs at once: a host array and a (sound) device array
                    kw.update({'dev': e.dev[0].ptr} if knob == 'both' and call is not nci_field else
                              {'s_dev': e.dev[0].ptr, 'x_dev': e.dev[1].ptr} if knob == 'both' else KNOB_VALUES[knob])
                yield f'{call.__name__}[{"+".join(subset)}]', call, kw


def device_cases(e, rho, lab):
    a, b = e.dev[0].ptr, e.dev[1].ptr
    yield 'laplacian_field[misaligned]', laplacian_field, dict(host=False, dev=a + 1)
    yield 'laplacian_field[density]', laplacian_field, dict(host=False, dev=rho)
    yield 'laplacian_field[density+8]', laplacian_field, dict(host=False, dev=rho + 8)
    yield 'nci_field[s misaligned]', nci_field, dict(host=False, s_dev=a + 1, x_dev=b)
    yield 'nci_field[x misaligned]', nci_field, dict(host=False, s_dev=a, x_dev=b + 1)
    yield 'nci_field[both misaligned]', nci_field, dict(host=False, s_dev=a + 1, x_dev=b + 1)
    yield 'nci_field[x is the density]', nci_field, dict(host=False, s_dev=a, x_dev=rho)
    yield 'nci_field[s misaligned, x is the density]', nci_field, dict(host=False, s_dev=a + 1, x_dev=rho)
    yield 'nci_field[s is x]', nci_field, dict(host=False, s_dev=a, x_dev=a)
    yield 'nci_field[s overlaps x]', nci_field, dict(host=False, s_dev=a, x_dev=a + 8)
    yield 'nci_field[one device output]', nci_field, dict(host=False, s_dev=a)
    yield 'hirshfeld_field[misaligned]', hirshfeld_field, dict(host=False, dev=a + 1)
    yield 'hirshfeld_field[density]', hirshfeld_field, dict(host=False, dev=rho)
    yield 'hirshfeld_field[no output]', hirshfeld_field, dict(host=False)
    yield 'isosurface[field misaligned]', isosurface, dict(field=a + 1)
    yield 'isosurface[colour misaligned]', isosurface, dict(colour=a + 1)
    yield 'isosurface[field misaligned, no labels count]', isosurface, dict(field=a + 1, n=-1)
    yield 'isosurface[field overlaps colour]', isosurface, dict(field=a, colour=a + 8)
    yield 'isosurface_nci_mask[misaligned]', isosurface_nci_mask, dict(dev=a + 1)
    yield 'isosurface_nci_mask[density]', isosurface_nci_mask, dict(dev=rho)
    yield 'regions_label[field misaligned]', regions_label, dict(field=a + 1)
    yield 'regions_label[field misaligned, below]', regions_label, dict(field=a + 1, mode=1)
    yield 'regions_label[nci with a field]', regions_label, dict(field=a, mode=2)
    yield 'regions_label[nci without a lattice]', regions_label, dict(mode=2, nci_lattice=False)
    yield 'regions_label[gather without nci]', regions_label, dict(flags=4)
    yield 'weight_sum_device[misaligned]', weight_sum_device, dict(ptr=a + 1)
    yield 'weight_sum_device[misaligned, null stride]', weight_sum_device, dict(ptr=a + 1, null=True)
    yield 'import_labels[misaligned]', import_labels, dict(ptr=a + 1)
    yield 'import_labels[labels]', import_labels, dict(ptr=lab)
    yield 'import_labels[bad dtype, misaligned]', import_labels, dict(ptr=a + 1, dtype=3)
    yield 'export_labels[misaligned]', export_labels, dict(ptr=a + 2)
    yield 'export_labels[labels]', export_labels, dict(ptr=lab)


def collect():
    """case id -> [code, text]"""
    e = Env()
    got = {}
    token = re.compile(r'0x[0-9a-f]{6,}')

    def run(state, name, call, h, **kw):
        rc = call(e, h, **kw)
        assert f'{state}/{name}' not in got
        got[f'{state}/{name}'] = [int(rc), token.sub('<ptr>', e.lib.xb_last_error().decode())]

    try:
        zeros = (np.zeros(27), np.zeros(9))
        for call in NULL_CTX:
            run('null context', call.__name__, call, None)
        for call in NO_GRID:
            run('no grid', call.__name__, call, e.h)
        rho = np.arange(N, dtype=np.float64).reshape(SHAPE)
        e.ctx.set_grid(SHAPE, *zeros, x_range=SLAB)
        e.ctx.upload_density(rho)
        e.ctx.upload_labels(np.zeros(SHAPE, np.int32))
        for call in CALLS:
            if call not in NOT_ON_A_SLAB:
                run('slab', call.__name__, call, e.h)
        e.ctx.set_grid((3, 3, 3), *zeros)         # (another voxel count: whatever the slab held goes)
        e.ctx.set_grid(SHAPE, *zeros)
        for call in CALLS + FETCHES:
            if call not in NO_DENSITY_NEEDED:
                run('no density', call.__name__, call, e.h)
        e.ctx.upload_density(rho)
        for call in READS_LABELS:
            run('no labels', call.__name__, call, e.h)
        e.ctx.upload_labels(np.zeros(SHAPE, np.int32))
        run('ready', 'hirshfeld_field[no setup]', hirshfeld_field, e.h)
        assert hirshfeld_setup(e, e.h) == 0, e.lib.xb_last_error()     # (the one call here that is not refused: the field's checks need a setup)
        p_rho, p_lab = int(e.lib.xb_density_ptr(e.h)), int(e.lib.xb_labels_ptr(e.h))
        for name, call, kw in itertools.chain(knob_cases(e), device_cases(e, p_rho, p_lab)):
            run('ready', name, call, e.h, **kw)
        for call in FETCHES:
            run('ready', call.__name__, call, e.h)
    finally:
        e.close()
    return got


def test_every_refusal_keeps_its_code_and_its_text():
    want = json.load(open(GOLDEN))
    got = collect()
    assert sorted(got) == sorted(want)
    assert all(rc in (-1, -3, -4) and text for rc, text in got.values()), {k: x for k, x in got.items() if x[0] not in (-1, -3, -4) or not x[1]}
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, f'{len(wrong)} of {len(want)} refusals changed: {list(wrong.items())[:4]}'


if __name__ == '__main__':
    if len(sys.argv) < 2 or sys.argv[1] != '--record':
        sys.exit('usage: test_gpu_refusals.py --record [PATH]')
    path = sys.argv[2] if len(sys.argv) > 2 else GOLDEN
    cases = collect()
    bad = {k: x for k, x in cases.items() if x[0] not in (-1, -3, -4)}
    if bad:
        sys.exit(f'not refused: {bad}')
    with open(path, 'w') as f:
        json.dump(cases, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'{len(cases)} refusals written to {path}')
