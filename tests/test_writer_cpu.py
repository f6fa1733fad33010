"""The digit core of the density text writer (pybader_amd/csrc/fmt_core.h) compiled for the host with g++ and checked
against Python's own format / the reference's fortran_format text (tests/golden/writer_vectors*.npz) before any GPU
runs it; the host fallback (textfmt.host_strings) against the same fixtures; and the writer's loud failure without a
GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from pybader_amd import _lib, io_cube, io_vasp, synth, textfmt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
CORE = os.path.join(ROOT, 'pybader_amd', 'csrc', 'fmt_core.h')

SHIM = r'''
#include "fmt_core.h"
extern "C" long long fmt_many(const double *v, long long n, int style, int prec, const double *p10, int lo, int np_,
                              char *out, long long *off) {
    long long pos = 0, n_host = 0;
    for (long long i = 0; i < n; i++) {
        off[i] = pos;
        int k = fmt_value(v[i], style, prec, p10, lo, np_, out + pos);
        if (k < 0) { n_host++; k = 0; }
        pos += k;
    }
    off[n] = pos;
    return n_host;
}
'''


@pytest.fixture(scope='module')
def core(tmp_path_factory):
    gxx = shutil.which('g++') or shutil.which('c++')
    if gxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('fmt_core')
    src = d / 'shim.cpp'
    src.write_text(SHIM)
    so = d / 'fmt_core.so'
    subprocess.check_call([gxx, '-O2', '-std=c++17', '-ffp-contract=off', '-fno-fast-math', '-shared', '-fPIC',
                           '-I', os.path.dirname(CORE), '-o', str(so), str(src)])
    lib = C.CDLL(str(so))
    lib.fmt_many.restype = C.c_longlong
    def run(vals, style, prec, p10=None):
        """(text of each value, '' where the device would leave it to the host; number of those)"""
        p10 = np.ascontiguousarray(textfmt.pow10_table() if p10 is None else p10, dtype=np.float64)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        out = np.zeros(v.size * 32 + 8, np.uint8)
        off = np.zeros(v.size + 1, np.int64)
        nh = lib.fmt_many(v.ctypes.data_as(C.c_void_p), C.c_longlong(v.size), textfmt.STYLES[style], prec,
                          p10.ctypes.data_as(C.c_void_p), textfmt.POW10_LO, textfmt.POW10_N,
                          out.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p))
        b = out.tobytes()
        return [b[off[i]:off[i + 1]].decode() for i in range(v.size)], nh
    return run


def reference_pow10():
    """np.power(10.0, k) as the numpy that ran the reference computed it (the F style's digits depend on it)"""
    g = np.load(os.path.join(GOLDEN, 'writer_vectors.npz'))
    assert g['pow10'].size == textfmt.POW10_N
    return g['pow10']


def vectors(prec):
    g = np.load(os.path.join(GOLDEN, 'writer_vectors.npz'))
    logn = synth.lognormal_bits(int(g['n_lognormal']), int(g['seed_lognormal']))
    assert synth.sha256(logn) == str(g['lognormal_sha256']), 'synth.lognormal_bits drifted'
    vals = np.concatenate([g['values'], logn])
    text = (g['F5'] if prec == 5 else np.load(os.path.join(GOLDEN, 'writer_vectors_f11.npz'))['F11']).tobytes()
    lines = text.decode().split('\n')
    assert lines[-1] == '' and len(lines) == vals.size + 1
    return vals, lines[:-1]


def random_doubles(n, seed):
    """every exponent, both signs: uniform 64-bit patterns (nan / inf patterns included)"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(np.float64)


def python_ref(vals, style, prec):
    spec = ('%s.%dE' % (' ' if style == 'E_space' else '', prec))
    return [' ' + format(float(v), spec) for v in vals]


@pytest.mark.parametrize('prec', [11, 5])
@pytest.mark.parametrize('style', ['E', 'E_space'])
def test_e_style_equals_python_format(core, style, prec):
    vals = np.concatenate([random_doubles(1_000_000, prec), synth.lognormal_bits(1_000_000, prec, spread=4),
                           vectors(prec)[0]])
    got, n_host = core(vals, style, prec)
    want = python_ref(vals, style, prec)
    bad = [i for i in range(vals.size) if got[i] and got[i] != want[i]]
    assert not bad, [(repr(vals[i]), got[i], want[i]) for i in bad[:5]]
    mid = (np.abs(vals) > 1e-15) & (np.abs(vals) < 1e30)
    assert all(got[i] for i in np.flatnonzero(mid)), 'the exact range left a value to the host'
    assert n_host > 0


@pytest.mark.parametrize('prec', [11, 5])
def test_f_style_equals_reference_text(core, prec):
    vals, want = vectors(prec)
    got, n_host = core(vals, 'F', prec, reference_pow10())
    bad = [i for i in range(vals.size) if got[i] and got[i] != want[i]]
    assert not bad, [(repr(vals[i]), got[i], want[i]) for i in bad[:5]]
    assert n_host > 0
    # the host fallback writes what the reference writes, for every vector (nan, inf, subnormals included)
    host = textfmt.host_strings(vals, 'F', prec, reference_pow10())
    bad = [i for i in range(vals.size) if host[i] != want[i]]
    assert not bad, [(repr(vals[i]), host[i], want[i]) for i in bad[:5]]


def test_f_style_random_equals_host_formatter(core):
    vals = np.concatenate([random_doubles(200_000, 5), synth.lognormal_bits(200_000, 6)])
    for prec in (11, 5):
        got, n_host = core(vals, 'F', prec)
        want = textfmt.host_strings(vals, 'F', prec)
        bad = [i for i in range(vals.size) if got[i] and got[i] != want[i]]
        assert not bad, [(repr(vals[i]), got[i], want[i]) for i in bad[:5]]
        assert n_host < 0.02 * vals.size


def test_fast_path_covers_chgcar_magnitudes(core):
    rho = synth.synth_density((24, 24, 24), synth.TRICLINIC) * 204.6
    for style in ('E', 'E_space', 'F'):
        _, n_host = core(rho.ravel(), style, 11)
        assert n_host == 0, style


def test_writers_without_gpu_fail_loudly(tmp_path):
    lib = _lib.load()
    if lib.xb_device_count() > 0:
        pytest.skip('a GPU is present')
    rho = np.ones((4, 4, 4))
    info = {'charge_flag': True, 'spin_flag': False, 'element_nums': np.array([1]), 'comment': 'x\n'}
    with pytest.raises(_lib.BaderHipError):
        io_vasp.write('t', np.zeros((1, 3)), np.eye(3) * 4, {'charge': rho}, info, prefix=str(tmp_path) + '/')
    with pytest.raises(_lib.BaderHipError):
        io_cube.write('t', np.ones((1, 3)), np.eye(3) * 4, {'charge': rho}, {'elements': [1], 'comment': 'x\n'},
                      prefix=str(tmp_path) + '/')
    assert not os.listdir(tmp_path)
