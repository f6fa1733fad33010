"""CPU tests of the cube reader (io_cube.read): the header parser against the fixtures captured from the reference's
reader (tests/golden/make_golden_cube.py), the layouts the reference cannot read (an orbital id list, a fifth number on
line 3), and the orbital selection with a numpy restatement of xb_parse_cube_text standing in for the device."""
import os

import numpy as np
import pytest

from pybader_amd import io_cube

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CASES = ['cube_10x9x13_ff0', 'cube_10x9x13_ff1', 'cube_10x9x13_ff2', 'cube_8x7x12_ff0', 'cube_8x7x12_ff1',
         'cube_8x7x12_ff2', 'hand_12x10x18_signed', 'hand_7x9x11_crlf']
SCALE = io_cube.ang_to_bohr ** 3


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'cube_read.npz'))


def lines_of(raw):
    return raw.splitlines(keepends=True)


class NumpyCubeContext:
    """stands in for _lib.Context in io_cube.read: xb_parse_cube_text restated with numpy's string -> float64"""
    shape = None

    def __init__(self):
        self.calls = []

    def set_grid(self, shape, dist_mat, T_grad):
        self.shape = tuple(shape)

    def parse_cube_text(self, text, scale, nval=1, pick=0, accumulate=False):
        n = int(np.prod(self.shape))
        vals = np.array(bytes(text).split()[:n * nval], dtype=np.float64)
        if vals.size < n * nval:
            raise ValueError('short')
        x = vals[pick::nval].reshape(self.shape)
        self.rho = (self.rho + x) * scale if accumulate else x * scale
        self.calls.append((nval, pick, bool(accumulate), scale))
        return vals.size, 0

    def download_density(self):
        return self.rho.copy()


@pytest.mark.parametrize('case', CASES)
def test_header_equals_reference(golden, case):
    raw = golden[case + '_bytes'].tobytes()
    head = io_cube.read_header(raw)
    charge = golden[case + '_charge']
    assert np.array_equal(head.lattice, golden[case + '_lattice'])      # bit for bit
    assert np.array_equal(head.atoms, golden[case + '_atoms'])
    assert head.elements.dtype == np.int64 and np.array_equal(head.elements, golden[case + '_elements'])
    assert head.shape == charge.shape and head.nval == 1 and head.atom_count == head.elements.size
    # the density block starts on the line after the last atom
    assert head.data_offset == sum(len(t) for t in lines_of(raw)[:6 + head.atom_count])
    vals = np.array(raw[head.data_offset:].split(), dtype=np.float64)
    assert vals.size == charge.size
    assert np.array_equal((vals.reshape(charge.shape) * SCALE).view(np.int64), charge.view(np.int64))


@pytest.mark.parametrize('case', ['cube_10x9x13_ff0', 'hand_7x9x11_crlf'])
def test_reader_with_numpy_parser_equals_reference(golden, case, tmp_path, monkeypatch):
    from pybader_amd import utils
    monkeypatch.setattr(utils, 'remember_density', lambda ctx, d: None)
    path = tmp_path / 'f.cube'
    path.write_bytes(golden[case + '_bytes'].tobytes())
    density, lattice, atoms, info = io_cube.read(str(path), ctx=NumpyCubeContext())
    assert np.array_equal(density['charge'], golden[case + '_charge'])
    assert np.array_equal(lattice, golden[case + '_lattice']) and np.array_equal(atoms, golden[case + '_atoms'])
    assert info['filename'] == str(path) and info['prefix'] == str(tmp_path) + os.sep
    assert info['file_type'] == 'cube' and info['write_function'] is io_cube.write
    assert np.array_equal(info['voxel_offset'], [.5, .5, .5]) and info['elements'].dtype == np.int64


def with_orbitals(raw, nval, ids=None, per_line=None, seed=5):
    """the fixture's header turned into an orbital cube: a negative atom count and the id list (`per_line` ids on a
    line, the count first) or, without ids, nval as the fifth number of line 3; every voxel gets nval seeded values.
    Returns (file bytes, values [x][y][z][nval] as written)."""
    lines = lines_of(raw)
    head = io_cube.read_header(raw)
    natoms = head.atom_count
    l3 = lines[2].decode().split()
    if ids is None:
        lines[2] = (' '.join(l3[:4] + [str(nval)]) + '\n').encode()
        extra = []
    else:
        lines[2] = (' '.join([str(-natoms)] + l3[1:4]) + '\n').encode()
        toks = [str(len(ids))] + [str(i) for i in ids]
        per_line = per_line or len(toks)
        extra = [(' '.join(toks[k:k + per_line]) + '\n').encode() for k in range(0, len(toks), per_line)]
    rng = np.random.default_rng(seed)
    vals = rng.lognormal(-2.0, 2.0, head.shape + (nval,)) * rng.choice([-1.0, 1.0], head.shape + (nval,))
    flat = vals.reshape(-1)
    body = b''.join(b''.join(b'%13.5E' % v for v in flat[k:k + 6]) + b'\n' for k in range(0, flat.size, 6))
    return b''.join(lines[:6 + natoms] + extra) + body, np.array(['%13.5E' % v for v in flat], np.float64).reshape(vals.shape)


@pytest.mark.parametrize('per_line', [None, 2, 3])
def test_orbital_id_list(golden, per_line):
    """a negative atom count: the id list after the atoms, on one line or wrapped (the reference swallows the first
    data line after it)"""
    base = golden['cube_8x7x12_ff0_bytes'].tobytes()
    ids = [31, 32, 40, 7, 33]
    raw, _ = with_orbitals(base, len(ids), ids=ids, per_line=per_line)
    head = io_cube.read_header(raw)
    ref = io_cube.read_header(base)
    assert head.nval == 5 and list(head.ids) == ids and head.atom_count == -ref.atom_count
    assert np.array_equal(head.lattice, ref.lattice) and np.array_equal(head.atoms, ref.atoms)
    assert np.array_equal(head.elements, ref.elements)
    n_id_lines = 1 if per_line is None else -(-(len(ids) + 1) // per_line)
    assert head.data_offset == sum(len(t) for t in lines_of(raw)[:6 + ref.atom_count + n_id_lines])


def test_fifth_number_on_line_3(golden):
    """Gaussian: nval as the fifth number of line 3 (the reference reads a sixth one and raises IndexError)"""
    base = golden['cube_10x9x13_ff1_bytes'].tobytes()
    raw, _ = with_orbitals(base, 3)
    head = io_cube.read_header(raw)
    ref = io_cube.read_header(base)
    assert head.nval == 3 and list(head.ids) == [1, 2, 3] and head.atom_count == ref.atom_count
    assert np.array_equal(head.lattice, ref.lattice) and np.array_equal(head.atoms, ref.atoms)
    assert head.data_offset == ref.data_offset + len(lines_of(raw)[2]) - len(lines_of(base)[2])


def test_orbital_selection(golden, tmp_path, monkeypatch):
    """every `orbitals` case, with the numpy stand-in for the device: the calls io_cube.read issues and their result"""
    from pybader_amd import utils
    monkeypatch.setattr(utils, 'remember_density', lambda ctx, d: None)
    base = golden['cube_8x7x12_ff0_bytes'].tobytes()
    ids = [31, 32, 40, 7]
    raw, vals = with_orbitals(base, len(ids), ids=ids, per_line=3)
    path = tmp_path / 'orb.cube'
    path.write_bytes(raw)

    def read(orbitals):
        ctx = NumpyCubeContext()
        return io_cube.read(str(path), orbitals=orbitals, ctx=ctx)[0]['charge'], ctx.calls

    got, calls = read(0)                                   # negative atom count: the sum of every value
    want = (((vals[..., 0] + vals[..., 1]) + vals[..., 2]) + vals[..., 3]) * SCALE
    assert np.array_equal(got, want)
    assert calls == [(4, 0, False, 1.0), (4, 1, True, 1.0), (4, 2, True, 1.0), (4, 3, True, SCALE)]
    got, calls = read(40)
    assert np.array_equal(got, vals[..., 2] * SCALE) and calls == [(4, 2, False, SCALE)]
    got, _ = read([7, 31])                                 # in the order listed
    assert np.array_equal(got, (vals[..., 3] + vals[..., 0]) * SCALE)
    got, _ = read(-1)
    assert got.shape == (4,) + vals.shape[:3]
    assert np.array_equal(got, np.moveaxis(vals, -1, 0) * SCALE)
    for bad in (5, [31, 99], []):
        with pytest.raises(ValueError):
            read(bad)
    # positive atom count, nval on line 3: 0 takes the first value, ids are 1..nval
    raw, vals = with_orbitals(base, 3)
    path.write_bytes(raw)
    got, calls = read(0)
    assert np.array_equal(got, vals[..., 0] * SCALE) and calls == [(3, 0, False, SCALE)]
    got, _ = read(3)
    assert np.array_equal(got, vals[..., 2] * SCALE)
