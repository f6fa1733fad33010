"""Dipole and quadrupole moments of the density of every atom or Bader volume about its centre -- no counterpart in the
reference (the Henkelman group's `bader` program ships a multipole module; pybader has none).

The sweep runs in libbader_hip.so (xb_moment_sum, csrc/k_moments.h); the definition of what is summed is in
include/bader_hip.h and DESIGN.md section 13, and tests/test_multipole_cpu.py restates it in numpy.

UNITS AND SIGN.  The density counts electrons as positive.  With d the minimum-image vector from a centre to a voxel (in the
length unit of `lattice`) and dV the voxel volume, a row of `moments` holds

    m0 = sum rho dV                     (electrons: the charge of utils.charge_sum)
    m1 = sum rho d dV                   (electrons * length; columns 1-3: x y z)
    m2 = sum rho d d^T dV               (electrons * length^2; columns 4-9: xx xy xz yy yz zz)

An electron carries the charge -e, so the ELECTRONIC dipole is -m1 (in e * length) and the electronic traceless quadrupole
-(3 m2 - tr(m2) I) (in e * length^2).  The nucleus sits at the centre and contributes to neither."""
import numpy as np

from . import _lib
from .utils import ensure_density, ensure_labels

_PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))      # columns 4..9 of a moment row


def moment_sum(density, volumes, lattice, centres, voxel_volume):
    """Moments of `density` over the voxels of every label of `volumes` about `centres`.

    density       host array, or a float32 / float64 device array (as utils.charge_sum takes it)
    volumes       the label map, host or device array; labels < 0 and >= len(centres) are skipped
    lattice       the CELL's lattice, one row per axis
    centres       [n, 3] Cartesian centre of label 0 .. n - 1 (atoms - voxel_offset, or bader_maxima - voxel_offset)
    voxel_volume  every sum is multiplied by it once

    -> (moments f64[n, 10], volume f64[n]); inside utils.resident() nothing is uploaded again."""
    ctx = _lib.default_context()
    shape = tuple(int(n) for n in volumes.shape)
    if ctx.shape != shape:
        ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    ensure_density(ctx, density)
    ensure_labels(ctx, volumes)
    centres = np.ascontiguousarray(centres, dtype=np.float64).reshape(-1, 3)
    if centres.shape[0] == 0:
        return np.zeros((0, 10)), np.zeros(0)
    return ctx.moment_sum(lattice, centres, voxel_volume)


def second_moment(moments):
    """the symmetric matrices m2 [n, 3, 3] of moment rows [n, 10]"""
    m = np.asarray(moments, dtype=np.float64).reshape(-1, 10)
    out = np.empty((m.shape[0], 3, 3), np.float64)
    for k, (i, j) in enumerate(_PAIRS):
        out[:, i, j] = m[:, 4 + k]
        out[:, j, i] = m[:, 4 + k]
    return out


def dipole(moments):
    """the electronic dipole -m1 [n, 3] in e * length (electrons are counted positive in the density)"""
    m = np.asarray(moments, dtype=np.float64).reshape(-1, 10)
    return -m[:, 1:4]


def quadrupole(moments):
    """the electronic traceless quadrupole -(3 m2 - tr(m2) I) [n, 3, 3] in e * length^2.  The diagonal is formed as
    -((2 m_ii - m_jj) - m_kk), so an isotropic m2 gives exact zeros."""
    m2 = second_moment(moments)
    out = -(3.0 * m2)
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        out[:, i, i] = -((2.0 * m2[:, i, i] - m2[:, j, j]) - m2[:, k, k])
    return out
