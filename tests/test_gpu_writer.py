"""GPU tests of the density text writers (io_vasp.write, io_cube.write, Context.format_density_text): whole files
against the bytes the reference's writers produced (tests/golden/writer_files.npz), the read -> write round trip of
the CHGCAR fixtures, the adversarial formatting vectors through the C ABI, the fast path's share, the deliberate
divergences, the per-atom export without pybader, and a streamed 512^3 block."""
import os
import resource
import sys

import numpy as np
import pytest

from pybader_amd import _lib, io_cube, io_vasp, synth, textfmt

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), 'golden')
CHGCAR_CASES = [('chgcar_spin_12x11x14', True), ('chgcar_9x7x13', False)]
CUBE_CASES = ['cube_10x9x13', 'cube_8x7x12']


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


@pytest.fixture
def reference_powers(monkeypatch):
    """the Fortran style divides by numpy's np.power(10.0, k), which differs between numpy builds: use the powers of the
    numpy that ran the reference (stored with the fixtures), as the reference's output depends on them"""
    p10 = np.load(os.path.join(GOLDEN, 'writer_vectors.npz'))['pow10']
    monkeypatch.setattr(textfmt, 'pow10_table', lambda: p10.copy())
    return p10


def files():
    return np.load(os.path.join(GOLDEN, 'writer_files.npz'))


@pytest.mark.parametrize('ff', [0, 1, 2])
@pytest.mark.parametrize('name,spin', CHGCAR_CASES)
def test_chgcar_file_equals_reference(ctx, reference_powers, tmp_path, name, spin, ff):
    g = files()
    density = {'charge': g[name + '_charge']}
    if spin:
        density['spin'] = g[name + '_spin']
    keep = {k: v.copy() for k, v in density.items()}
    atoms, lattice = g[name + '_atoms'], g[name + '_lattice']
    atoms0, lattice0 = atoms.copy(), lattice.copy()
    info = {'element_nums': np.array([5, 3]), 'elements': ['Si', 'O'], 'charge_flag': True, 'spin_flag': spin,
            'fortran_format': ff, 'buffer_size': 64, 'comment': f'golden writer {name}\n'}
    io_vasp.write('t', atoms, lattice, density, info, prefix=str(tmp_path) + '/', ctx=ctx)
    got = (tmp_path / 't-CHGCAR').read_bytes()
    assert got == g[f'{name}_ff{ff}_bytes'].tobytes()
    for k in density:                                  # the caller's arrays are left alone
        assert np.array_equal(density[k], keep[k])
    assert np.array_equal(atoms, atoms0) and np.array_equal(lattice, lattice0)


@pytest.mark.parametrize('ff', [0, 1, 2])
@pytest.mark.parametrize('name', CUBE_CASES)
def test_cube_file_equals_reference(ctx, reference_powers, tmp_path, name, ff):
    g = files()
    rho, atoms, lattice = g[name + '_charge'], g[name + '_atoms'], g[name + '_lattice']
    keep = (rho.copy(), atoms.copy(), lattice.copy())
    info = {'elements': g[name + '_elements'], 'fortran_format': ff, 'comment': f'golden cube {name}\n'}
    for k in range(2):                                 # a second export from the same arrays: the same bytes
        io_cube.write('t', atoms, lattice, {'charge': rho}, info, prefix=str(tmp_path) + f'/{k}', ctx=ctx)
        assert (tmp_path / f'{k}t.cube').read_bytes() == g[f'{name}_ff{ff}_bytes'].tobytes()
    assert all(np.array_equal(a, b) for a, b in zip((rho, atoms, lattice), keep))


@pytest.mark.parametrize('name,ff', [('chgcar_py_12x11x14', 0), ('chgcar_f90_16x16x16', 2)])
def test_read_write_round_trip(ctx, reference_powers, tmp_path, name, ff):
    g = np.load(os.path.join(GOLDEN, name + '.npz'))
    src = tmp_path / 'CHGCAR'
    src.write_bytes(g['file_bytes'].tobytes())
    density, lattice, atoms, info = io_vasp.read(str(src), spin_flag=True, ctx=ctx)
    assert info['write_function'] is io_vasp.write
    info.update(comment='golden\n', elements=['H'], fortran_format=ff)
    info['write_function']('out', atoms, lattice, density, info, prefix=str(tmp_path) + '/', ctx=ctx)
    assert (tmp_path / 'out-CHGCAR').read_bytes() == g['file_bytes'].tobytes()


def formatted(ctx, vals, style, prec):
    """one value per line through the ABI (cube layout, records of one value)"""
    parts, n_host = [], 0
    for chunk, n in ctx.format_density_text(np.asarray(vals).reshape(-1, 1, 1), 1.0, style, prec, 'cube'):
        parts.append(bytes(chunk))
        n_host = n
    lines = b''.join(parts).decode().split('\n')
    assert lines[-1] == ''
    return lines[:-1], n_host


def vectors(prec):
    g = np.load(os.path.join(GOLDEN, 'writer_vectors.npz'))
    logn = synth.lognormal_bits(int(g['n_lognormal']), int(g['seed_lognormal']))
    assert synth.sha256(logn) == str(g['lognormal_sha256'])
    text = (g['F5'] if prec == 5 else np.load(os.path.join(GOLDEN, 'writer_vectors_f11.npz'))['F11']).tobytes()
    return np.concatenate([g['values'], logn]), text.decode().split('\n')[:-1]


@pytest.mark.parametrize('prec', [11, 5])
def test_adversarial_vectors(ctx, reference_powers, prec):
    vals, want_f = vectors(prec)
    for style, align in (('E', ''), ('E_space', ' ')):
        got, n_host = formatted(ctx, vals, style, prec)
        want = [' ' + format(float(v), f'{align}.{prec}E') for v in vals]
        bad = [i for i in range(vals.size) if got[i] != want[i]]
        assert not bad, [(repr(vals[i]), got[i], want[i]) for i in bad[:5]]
        assert n_host > 0
    got, n_host = formatted(ctx, vals, 'F', prec)
    bad = [i for i in range(vals.size) if got[i] != want_f[i]]
    assert not bad, [(repr(vals[i]), got[i], want_f[i]) for i in bad[:5]]
    assert n_host > 0


def test_fast_path_share(ctx):
    from pybader_amd.interface import distance_matrix, gradient_transform
    lat = synth.TRICLINIC
    shape = (128, 128, 128)
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)
    rho = ctx.download_density()
    resident = rho.copy()
    vol = float(np.dot(lat[0], np.cross(lat[1], lat[2])))
    for style in ('E', 'F'):
        n_host, nbytes = 0, 0
        for chunk, n in ctx.format_density_text(rho, vol, style, 11, 'chgcar'):
            n_host, nbytes = n, nbytes + len(chunk)
        assert n_host <= 0.001 * rho.size, (style, n_host)
        assert nbytes == 128 ** 3 // 5 * (5 * 18 + 1) + (128 ** 3 % 5) * 18 + 1   # 18 bytes a value in both
    assert np.array_equal(ctx.download_density(), resident)        # the resident density is left alone


@pytest.mark.parametrize('shape', [(10, 10, 10), (4, 4, 4)])
def test_grids_the_reference_cannot_write(ctx, tmp_path, shape):
    """N % 5 == 0 and fewer than buffer_size lines: the reference raises, ours writes the file by the same rule"""
    lat = synth.CUBIC6
    rho = synth.synth_density(shape, lat)
    info = {'element_nums': np.array([8]), 'elements': ['C'], 'charge_flag': True, 'spin_flag': False,
            'fortran_format': 0, 'buffer_size': 64, 'comment': 'divergence\n'}
    io_vasp.write('t', synth.atoms_cartesian(synth.ATOMS8, lat), lat, {'charge': rho}, info,
                  prefix=str(tmp_path) + '/', ctx=ctx)
    text = (tmp_path / 't-CHGCAR').read_bytes()
    n = rho.size
    assert text.count(b'\n') == 8 + 8 + 1 + 1 + (n + 4) // 5   # header, atoms, blank, grid line, data
    density, _, _, _ = io_vasp.read(str(tmp_path / 't-CHGCAR'), ctx=ctx)
    assert np.allclose(density['charge'], rho, rtol=1e-11, atol=0)


def test_export_atoms_without_pybader(ctx, tmp_path, monkeypatch):
    for mod in [m for m in sys.modules if m == 'pybader' or m.startswith('pybader.')]:
        monkeypatch.delitem(sys.modules, mod)
    monkeypatch.setitem(sys.modules, 'pybader', None)   # `import pybader` fails from here on
    from pybader_amd import thread_handlers
    from pybader_amd.interface import Bader
    thread_handlers.VERBOSE = False
    g = np.load(os.path.join(GOLDEN, 'chgcar_py_12x11x14.npz'))
    src = tmp_path / 'CHGCAR'
    src.write_bytes(g['file_bytes'].tobytes())
    density, lattice, atoms, info = io_vasp.read(str(src), ctx=ctx)
    info['elements'] = ['H']
    b = Bader(density, lattice, atoms, info, export_mode=('atoms', [-2]))
    b()
    outs = sorted(p for p in os.listdir(tmp_path) if p.startswith('Bader-atoms-'))
    assert len(outs) == atoms.shape[0]
    total = np.zeros_like(density['charge'])
    for k in range(atoms.shape[0]):
        got, _, _, _ = io_vasp.read(str(tmp_path / f'Bader-atoms-{k}-CHGCAR'), ctx=ctx)
        mine = got['charge']
        want = np.where(b.atoms_volumes == k, density['charge'], 0.0)
        assert np.allclose(mine, want, rtol=1e-12, atol=0)
        total += mine
    assert np.allclose(total, density['charge'], rtol=1e-12, atol=0)


def test_streamed_512(ctx, tmp_path):
    """a 2.4 GB text block written in chunks: every 997th line and every host-formatted value against Python's format,
    host memory bounded far below the size of the text"""
    from pybader_amd.interface import distance_matrix, gradient_transform
    lat = synth.CUBIC6
    shape = (512, 512, 512)
    vl = lat / np.array(shape, dtype=np.float64)[:, None]
    ctx.set_grid(shape, distance_matrix(vl), gradient_transform(vl))
    ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)          # bit-identical to synth.synth_density
    rho = ctx.download_density()
    vol = float(np.dot(lat[0], np.cross(lat[1], lat[2])))
    rss0 = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024
    path = tmp_path / 'block'
    with open(path, 'wb') as f:
        n_host = textfmt.write_block(f, ctx, rho, vol, 'E', 11, 'chgcar')
    grow = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024 - rss0
    size = path.stat().st_size
    assert size > 2_000_000_000
    assert grow < size // 4, f'peak host memory grew by {grow} bytes for {size} bytes of text'
    idx, hv = ctx.format_host
    assert idx.size == n_host
    flat = (np.swapaxes(rho, 0, 2).ravel()) * vol
    with open(path, 'rb') as f:
        for i, line in enumerate(f):
            if i % 997 == 0:
                want = ''.join(' ' + format(float(v), '.11E') for v in flat[5 * i:5 * i + 5]) + '\n'
                assert line.decode() == want, i
    assert i == (flat.size + 4) // 5 - 1
    for j, v in zip(idx, hv):
        assert v == flat[j]
    path.unlink()
