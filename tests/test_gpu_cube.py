"""GPU tests of the cube reader: io_cube.read against the fixtures captured from the reference's reader (bit for bit,
density left resident), xb_parse_cube_text against numpy's string -> float64 on seeded text of every number shape
(nval 1 and 3, accumulate chains, errors), Bader end to end on a cube file (also with a second cube as the spin
density) and write_volume after a cube read."""
import os

import numpy as np
import pytest

from pybader_amd import _lib, io_cube
from pybader_amd.interface import Bader
from test_gpu_chgcar import seeded_text

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CASES = ['cube_10x9x13_ff0', 'cube_10x9x13_ff1', 'cube_10x9x13_ff2', 'cube_8x7x12_ff0', 'cube_8x7x12_ff1',
         'cube_8x7x12_ff2', 'hand_12x10x18_signed', 'hand_7x9x11_crlf']
SCALE = io_cube.ang_to_bohr ** 3


@pytest.fixture(scope='module')
def golden():
    return np.load(os.path.join(GOLDEN, 'cube_read.npz'))


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def write_case(golden, case, path):
    path.write_bytes(golden[case + '_bytes'].tobytes())
    return str(path)


@pytest.mark.parametrize('case', CASES)
def test_reader_equals_reference(ctx, golden, case, tmp_path):
    fn = write_case(golden, case, tmp_path / 'f.cube')
    density, lattice, atoms, info = io_cube.read(fn, ctx=ctx)
    want = golden[case + '_charge']
    assert np.array_equal(bits(density['charge']), bits(want))        # bit for bit, signed zeros included
    assert np.array_equal(lattice, golden[case + '_lattice'])
    assert np.allclose(atoms, golden[case + '_atoms'], rtol=0, atol=1e-12)
    assert np.array_equal(info['elements'], golden[case + '_elements'])
    assert info['write_function'] is io_cube.write and info['file_type'] == 'cube'
    # the density is the resident one: the hot path starts without an upload
    assert np.array_equal(bits(ctx.download_density()), bits(want))


def numpy_values(text, n):
    return np.array(text.split()[:n], dtype=np.float64)


@pytest.mark.parametrize('shape,seed', [((7, 5, 3), 1), ((16, 8, 24), 2), ((40, 48, 56), 3)])
def test_parser_equals_numpy_on_seeded_text(ctx, shape, seed):
    """fast path, 18-digit mantissas and huge exponents (host fallback), zeros, ragged lines, tabs"""
    n = int(np.prod(shape))
    text = seeded_text(shape, seed)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    n_tokens, n_host = ctx.parse_cube_text(text, SCALE)
    want = numpy_values(text, n).reshape(shape) * SCALE                 # C order
    assert n_tokens >= n and n_host > 0
    assert np.array_equal(bits(ctx.download_density()), bits(want))


def test_negative_zero_in_store_mode(ctx):
    toks = ['-0.00000E+00', '0.0', '-0.0', '1.5', '-2.5E-03', '-0', '+0.0', '-.0E5']
    text = ' '.join(toks * 8).encode()
    ctx.set_grid((4, 4, 4), np.zeros(27), np.zeros(9))
    ctx.parse_cube_text(text, SCALE)
    want = numpy_values(text, 64).reshape(4, 4, 4) * SCALE
    assert np.array_equal(bits(ctx.download_density()), bits(want))
    assert np.signbit(ctx.download_density().reshape(-1)[0])


def test_orbitals_pick_and_accumulate(ctx):
    """nval = 3: every pick on its own, and a chain ((a + b) + c) * s against numpy left to right"""
    shape = (12, 10, 14)
    n = int(np.prod(shape))
    text = seeded_text((3,) + shape, 4)                                 # 3 n numbers
    vals = numpy_values(text, 3 * n)
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    for pick in range(3):
        _, n_host = ctx.parse_cube_text(text, SCALE, 3, pick)
        assert n_host > 0 or pick == 0                                  # seeded_text's host-only shapes: k % 9 in (4, 5)
        assert np.array_equal(bits(ctx.download_density()), bits(vals[pick::3].reshape(shape) * SCALE))
    order = [2, 0, 1]
    for k, pick in enumerate(order):
        ctx.parse_cube_text(text, SCALE if k == len(order) - 1 else 1.0, 3, pick, accumulate=k > 0)
    v = [vals[p::3].reshape(shape) for p in order]
    assert np.array_equal(bits(ctx.download_density()), bits(((v[0] + v[1]) + v[2]) * SCALE))


def test_parser_errors(ctx):
    ctx.set_grid((4, 4, 4), np.zeros(27), np.zeros(9))
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.parse_cube_text(b' 1.0 2.0 3.0\n', 1.0)                    # fewer numbers than voxels
    assert e.value.code == _lib.XB_E_SHORT
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.parse_cube_text(b' '.join([b'1.0'] * 191), 1.0, 3, 1)     # 191 < 64 * 3
    assert e.value.code == _lib.XB_E_SHORT
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.parse_cube_text(b' '.join([b'1.0'] * 63 + [b'1.0x']), 1.0)  # a malformed number
    assert e.value.code == _lib.XB_E_ARG
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.parse_cube_text(b'1.0 ' * 64, 1.0, 2, 2)                    # pick outside [0, nval)
    assert e.value.code == _lib.XB_E_ARG
    with pytest.raises(_lib.BaderHipError) as e:
        ctx.parse_cube_text(b'1.0 ' * 64, 1.0, 1 << 25, 0)              # 64 * 2^25 numbers: beyond int offsets
    assert e.value.code == _lib.XB_E_LIMIT
    ctx.parse_cube_text(b'2.0 ' * 64, 0.5)                              # the context is still usable
    assert np.array_equal(ctx.download_density(), np.ones((4, 4, 4)))


def host_bader(charge, lattice, atoms, spin=None):
    density = {'charge': np.array(charge)}
    if spin is not None:
        density['spin'] = np.array(spin)
    b = Bader(density, lattice, atoms, {'voxel_offset': np.array([.5, .5, .5])}, spin_flag=spin is not None)
    b()
    return b


def assert_same_run(got, want, spin=False):
    """same maps and volumes; the sums agree to a few ulps: xb_charge_sum adds with device atomics, so two runs on one
    density may add in another order"""
    assert np.array_equal(got.bader_volumes, want.bader_volumes)
    assert np.array_equal(got.atoms_volumes, want.atoms_volumes)
    assert np.array_equal(got.atoms_volume, want.atoms_volume) and np.array_equal(got.bader_volume, want.bader_volume)
    pairs = [(got.atoms_charge, want.atoms_charge), (got.bader_charge, want.bader_charge)]
    if spin:
        pairs += [(got.atoms_spin, want.atoms_spin), (got.bader_spin, want.bader_spin)]
    for a, b in pairs:
        assert np.allclose(a, b, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize('case', ['cube_10x9x13_ff0', 'hand_7x9x11_crlf'])
def test_bader_end_to_end(golden, case, tmp_path):
    fn = write_case(golden, case, tmp_path / 'f.cube')
    b = Bader(*io_cube.read(fn))
    b()
    want = host_bader(golden[case + '_charge'], golden[case + '_lattice'], golden[case + '_atoms'])
    assert_same_run(b, want)


def test_spin_from_a_second_cube(golden, tmp_path):
    """examples/cube_charges.py --spin: the charge cube read first, then a second cube as the spin density -- the
    partition must run on the charge, not on the density the second read left on the card"""
    case = 'cube_10x9x13_ff0'
    raw = golden[case + '_bytes'].tobytes()
    head = io_cube.read_header(raw)
    rng = np.random.default_rng(9)
    spin_vals = (rng.random(head.shape) - 0.5) * golden[case + '_charge'] / SCALE
    toks = ['%13.5E' % v for v in spin_vals.reshape(-1)]
    body = ''.join(''.join(toks[k:k + 6]) + '\n' for k in range(0, len(toks), 6)).encode()
    (tmp_path / 'spin.cube').write_bytes(raw[:head.data_offset] + body)
    fn = write_case(golden, case, tmp_path / 'charge.cube')
    density, lattice, atoms, info = io_cube.read(fn)
    density['spin'] = io_cube.read(str(tmp_path / 'spin.cube'))[0]['charge']
    b = Bader(density, lattice, atoms, info, spin_flag=True)
    b()
    spin_host = np.array(toks, dtype=np.float64).reshape(head.shape) * SCALE
    assert np.array_equal(bits(density['spin']), bits(spin_host))
    want = host_bader(golden[case + '_charge'], golden[case + '_lattice'], golden[case + '_atoms'], spin=spin_host)
    assert_same_run(b, want, spin=True)


def test_write_volume_after_cube_read(golden, tmp_path):
    case = 'hand_12x10x18_signed'
    os.makedirs(tmp_path / 'in')
    fn = write_case(golden, case, tmp_path / 'in' / 'f.cube')
    b = Bader(*io_cube.read(fn))
    b()
    b.export_mode = ('atoms', [0])
    b.write_volume(0)
    masked = np.where(b.atoms_volumes == 0, b.charge, 0.0)
    info = dict(b.info, fortran_format=0, comment='Bader atoms: 0\n')
    io_cube.write('Bader-atoms-0', b.atoms, b.lattice, {'charge': masked}, info, prefix=str(tmp_path) + '/')
    got = (tmp_path / 'in' / 'Bader-atoms-0.cube').read_bytes()
    assert got == (tmp_path / 'Bader-atoms-0.cube').read_bytes()
    assert got[:len(b'Cube File')] == b'Cube File'


def test_example_with_spin(golden, tmp_path):
    """examples/cube_charges.py --spin on fixture files: charge conserved, spin summed per atom"""
    import importlib.util
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('cube_charges', os.path.join(root, 'examples', 'cube_charges.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    charge = write_case(golden, 'cube_10x9x13_ff0', tmp_path / 'charge.cube')
    spin = write_case(golden, 'cube_10x9x13_ff2', tmp_path / 'spin.cube')
    argv, sys.argv = sys.argv, ['cube_charges.py', charge, '--spin', spin]
    try:
        b = mod.main()
    finally:
        sys.argv = argv
    assert np.array_equal(b.charge, golden['cube_10x9x13_ff0_charge'])
    assert np.array_equal(b.spin, golden['cube_10x9x13_ff2_charge'])
    for k in range(b.atoms_charge.shape[0]):
        m = b.atoms_volumes == k
        assert abs(b.atoms_spin[k] - b.spin[m].sum() * b.voxel_volume) <= 1e-9 * max(1.0, abs(b.atoms_spin[k]))
    total = b.atoms_charge.sum() + b.vacuum_charge
    assert abs(total - b.charge.sum() * b.voxel_volume) < 1e-9 * abs(total)
