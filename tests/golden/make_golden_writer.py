#!/opt/conda/bin/python3.9
"""Golden fixtures for the density text writers (io_vasp.write, io_cube.write), made by IMPORTING THE REFERENCE:

    /opt/conda/bin/python3.9 -W ignore tests/golden/make_golden_writer.py

Drives the reference's own `pybader.io.vasp.write`, `pybader.io.cube.write` and `pybader.utils.fortran_format` and
stores data only: the inputs handed to them and the bytes / strings they produced.
  writer_files.npz    whole files: CHGCAR (with and without spin) and cube (nz % 6 != 0 and == 0) in fortran_format
                      0, 1 and 2, on grids the reference can write
  writer_vectors.npz  adversarial values (ties, carries, neighbours of 10^k, 3-digit exponents, subnormals, +-0, nan,
                      +-inf, 1e+-300, the '<U{prec}' truncation case) followed by 20 k synth.lognormal_bits values (not
                      stored: the tests regenerate them, their sha256 is stored) and the reference's fortran_format
                      text of each at precision 5 ('\\n' separated bytes); writer_vectors_f11.npz the same at precision 11
Nothing of the reference is copied.  Runs only in the build container (needs /root/reference)."""
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402,F401  (sets up the environment + numba shim the reference needs)
from pybader.io import cube, vasp  # noqa: E402
from pybader.utils import fortran_format, nostdout  # noqa: E402

from pybader_amd import synth  # noqa: E402

FORMATS = (0, 1, 2)
LOGNORMAL = (20000, 17)   # synth.lognormal_bits(n, seed) values appended to the adversarial ones


def chgcar_case(out, name, shape, lattice, spin, ff):
    rho = synth.synth_density(shape, lattice, synth.ATOMS8, synth.BACKGROUND)
    density = {'charge': rho}
    if spin:
        rng = np.random.default_rng(3)
        density['spin'] = (rng.random(shape) - 0.5) * rho
    atoms = synth.atoms_cartesian(synth.ATOMS8, lattice)
    info = {'element_nums': np.array([5, 3]), 'elements': ['Si', 'O'], 'charge_flag': True, 'spin_flag': spin,
            'fortran_format': ff, 'buffer_size': 64, 'comment': f'golden writer {name}\n'}
    d = tempfile.mkdtemp()
    with nostdout():
        vasp.write('t', atoms.copy(), lattice.copy(), {k: v.copy() for k, v in density.items()}, info,
                   prefix=os.path.join(d, ''))
    key = f'{name}_ff{ff}'
    out[key + '_bytes'] = np.frombuffer(open(os.path.join(d, 't-CHGCAR'), 'rb').read(), dtype=np.uint8)
    if ff == 0:                                   # inputs once per case
        out[name + '_charge'] = rho
        if spin:
            out[name + '_spin'] = density['spin']
        out[name + '_atoms'] = atoms
        out[name + '_lattice'] = lattice
    print(key, out[key + '_bytes'].size, 'bytes')


def cube_case(out, name, shape, lattice, ff):
    rho = synth.synth_density(shape, lattice, synth.ATOMS8, synth.BACKGROUND) * 0.1481847
    atoms = synth.atoms_cartesian(synth.ATOMS8, lattice)
    info = {'elements': np.array([14, 14, 8, 8, 8, 1, 1, 6]), 'fortran_format': ff, 'comment': f'golden cube {name}\n'}
    d = tempfile.mkdtemp()
    with nostdout():
        cube.write('t', atoms.copy(), lattice.copy(), {'charge': rho.copy()}, info, prefix=os.path.join(d, ''))
    key = f'{name}_ff{ff}'
    out[key + '_bytes'] = np.frombuffer(open(os.path.join(d, 't.cube'), 'rb').read(), dtype=np.uint8)
    if ff == 0:
        out[name + '_charge'] = rho
        out[name + '_atoms'] = atoms
        out[name + '_lattice'] = lattice
        out[name + '_elements'] = info['elements']
    print(key, out[key + '_bytes'].size, 'bytes')


def adversarial():
    rng = np.random.default_rng(2024)
    v = [0.0, -0.0, np.nan, -np.nan, np.inf, -np.inf, 1e300, -1e300, 1e-300, -1e-300, 1e100, 1e-100, 3.7e123, -4.2e-150,
         5e-324, -5e-324, 2.2250738585072014e-308, 2.225073858507201e-308, 1.5e-310,
         1234567890.125, 9.9999999999995e5, 0.999999999999, 0.99999999999949, 9.99999, 9.999995, 0.1, 1.0, -1.0, 0.5]
    for k in range(-40, 41):                      # 10^k and its neighbours, both signs
        p = float('1e%d' % k)
        for x in (p, np.nextafter(p, 0.0), np.nextafter(p, np.inf)):
            v += [x, -x]
    for prec in (11, 5):                          # exact ties: integers of prec + 2 digits ending in 5, and x.5
        d = rng.integers(10 ** prec, 10 ** (prec + 1), 200, dtype=np.int64)
        v += [float(int(x) * 10 + 5) for x in d]
        v += [float(int(x)) + 0.5 for x in rng.integers(10 ** prec, 10 ** (prec + 1) // 2, 100, dtype=np.int64)]
        nines = 10 ** (prec + 1) - 1              # carries into the next exponent: 9.99...9|5 and above
        for e in (-12, -3, 0, 3, 12):
            v += [float('%d5e%d' % (nines, e - prec - 1)), float('%d6e%d' % (nines, e - prec - 1))]
    return np.array(v, dtype=np.float64)


if __name__ == '__main__':
    files = {}
    for ff in FORMATS:
        chgcar_case(files, 'chgcar_spin_12x11x14', (12, 11, 14), synth.TRICLINIC, True, ff)
        chgcar_case(files, 'chgcar_9x7x13', (9, 7, 13), synth.CUBIC6, False, ff)
        cube_case(files, 'cube_10x9x13', (10, 9, 13), synth.TRICLINIC, ff)
        cube_case(files, 'cube_8x7x12', (8, 7, 12), synth.CUBIC6, ff)
    np.savez_compressed(os.path.join(HERE, 'writer_files.npz'), **files)
    vals = adversarial()
    logn = synth.lognormal_bits(*LOGNORMAL)
    vec = {'values': vals, 'n_lognormal': LOGNORMAL[0], 'seed_lognormal': LOGNORMAL[1],
           'lognormal_sha256': synth.sha256(logn),
           'pow10': np.power(10.0, np.arange(-300, 301, dtype=np.int64))}   # this numpy's powers (the F style's digits)
    vals = np.concatenate([vals, logn])
    with np.errstate(all='ignore'):
        text = {prec: np.frombuffer(fortran_format(vals.reshape(-1, 1), prec).encode(), dtype=np.uint8) for prec in (11, 5)}
    np.savez_compressed(os.path.join(HERE, 'writer_vectors.npz'), F5=text[5], **vec)
    np.savez_compressed(os.path.join(HERE, 'writer_vectors_f11.npz'), F11=text[11])
    for f in ('writer_files.npz', 'writer_vectors.npz', 'writer_vectors_f11.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)), 'bytes')
