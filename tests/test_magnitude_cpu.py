"""CPU twin of the magnitude and sign cases of tests/test_gpu_soak.py (soak_vs_oracle.MAGNITUDE_CASES): what makes those GPU
tests meaningful.  It draws the same cases, builds their densities with numpy (synth.synth_density: the device's own synthesis
differs from it by rounding, far below anything asserted here) and asserts that each input reaches the predicate it is for:

  * grad-40 / -44 / -48: max_grad (restated below: central differences with the assignment's tie rule, then T_grad) times 2^k lies
    below the 1E-14 of the stay test for a share of the voxels in [0.05, 0.80] -- gradient steps and ongrid steps mix.
    At least 0.03 of the voxels must have a small gradient that is not zero: a drawn plateau quantum alone fills the share with
    exact zeros, which the plain soak's plateaus already take through the branch.
    Measured (16^3, 20x24x28, 32^3, 24x32x128), all voxels below / those with 0 < max_grad among them:
        neargrid-grad-40  0.163/0.161 0.165/0.164 0.119/0.119 0.059/0.044
        neargrid-grad-44  0.503/0.492 0.409/0.352 0.169/0.113 0.333/0.333
        neargrid-grad-48  0.794/0.789 0.759/0.405 0.727/0.226 0.649/0.649
        ongrid-grad-40    0.132/0.130 0.228/0.227 0.155/0.155 0.110/0.110
        ongrid-grad-44    0.409/0.380 0.428/0.419 0.472/0.471 0.334/0.333
        ongrid-grad-48    0.781/0.779 0.754/0.705 0.757/0.695 0.693/0.184
    (the plain atoms without noise or plateaus: 0.11-0.16, 0.33-0.44, 0.65-0.79)
  * subnormal: every brick maximum times 2^-140 maps to a subnormal or zero float32; overflow: times 2^130 at least one maps to inf.
  * the directed case of fix 1 (soak_vs_oracle.directed_vacuum_case): float32(m) * (1 + 1e-6) < tol < m for its brick, and the
    oracle assigns voxels of that brick to a basin.
  * negative: the oracle's maxima and maps of the shifted density equal those of the unshifted quantised one; overflow: those of the
    scaled density equal the unscaled one's.  (At 2^-140 they do NOT: every step becomes an ongrid step, the oracle's own
    map changes, and the library must follow the oracle there.)"""
import functools

import numpy as np
import pytest

import soak_vs_oracle as soak
from pybader_amd import synth
from pybader_amd.interface import distance_matrix, gradient_transform

FLT_MIN = float(np.finfo(np.float32).tiny)


def max_grad(rho, tg):
    """methods.py:324-334 per voxel: an axis on which the voxel is no smaller than both neighbours contributes 0, else the central
    difference; grad_dir = T_grad . grad with (a + b) + c association; the largest |component|"""
    g = []
    for ax in range(3):
        hi, lo = np.roll(rho, -1, ax), np.roll(rho, 1, ax)
        g.append(np.where((hi <= rho) & (rho >= lo), 0.0, (hi - lo) / 2.0))
    d = [((tg[i, 0] * g[0]) + (tg[i, 1] * g[1])) + (tg[i, 2] * g[2]) for i in range(3)]
    return np.maximum(np.maximum(np.abs(d[0]), np.abs(d[1])), np.abs(d[2]))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """per grid of the case: (case, density, tolerance, dist_mat, T_grad)"""
    method, seed, scale, offset, tols = soak.MAGNITUDE_CASES[name]
    out = []
    for case in soak.draw_cases(len(soak.MAGNITUDE_SHAPES), seed, shapes=soak.MAGNITUDE_SHAPES, tols=tols):
        vl = np.divide(case['lat'], case['shape'])
        rho, tol = soak.finish_density(synth.synth_density(case['shape'], case['lat'], synth.ATOMS8), case, scale, offset)
        out.append((case, rho, tol, distance_matrix(vl), gradient_transform(vl)))
    return out


def brick_maxima(rho):
    """the largest density of every 8^3 brick (cut bricks included)"""
    nb = [(n + 7) // 8 for n in rho.shape]
    pad = np.full([8 * n for n in nb], -np.inf)
    pad[:rho.shape[0], :rho.shape[1], :rho.shape[2]] = rho
    return pad.reshape(nb[0], 8, nb[1], 8, nb[2], 8).max(axis=(1, 3, 5))


def test_the_cases_cover_the_issue():
    scales = {(m, s, o, t is not None and t[0] is not None) for m, _, s, o, t in soak.MAGNITUDE_CASES.values()}
    for m in ('neargrid', 'ongrid'):
        assert {(m, k, None, False) for k in (-40, -44, -48, 130)} <= scales
        assert {(m, -140, None, False), (m, -140, None, True), (m, 0, 4.0, False), (m, 0, 4.0, True)} <= scales
    assert soak.MAGNITUDE_SHAPES == [(16, 16, 16), (20, 24, 28), (32, 32, 32), (24, 32, 128)]


@pytest.mark.parametrize('name', [n for n in soak.MAGNITUDE_CASES if '-grad' in n])
def test_the_gradient_straddles_the_stay_threshold(name):
    shares = []
    for case, rho, tol, dm, tg in inputs(name):
        mg = max_grad(rho, tg)
        shares.append((float((mg < 1E-14).mean()), float(((mg < 1E-14) & (mg > 0)).mean())))
    print(name, ' '.join('%.3f/%.3f' % s for s in shares))
    assert all(0.05 <= s[0] <= 0.80 for s in shares), shares
    assert all(s[1] >= 0.03 for s in shares), 'voxels whose gradient is small but not zero: not plateaus alone'


@pytest.mark.parametrize('name', [n for n in soak.MAGNITUDE_CASES if 'subnormal' in n])
def test_every_brick_potential_is_subnormal(name):
    for case, rho, tol, dm, tg in inputs(name):
        with np.errstate(under='ignore'):
            f = brick_maxima(rho).astype(np.float32)
        assert (np.abs(f) < FLT_MIN).all() and (brick_maxima(rho) > 0).all()
        if tol is not None:    # the tolerance cuts through the grid: there is vacuum and there are voxels to assign
            assert 0 < (rho <= tol).mean() < 1


@pytest.mark.parametrize('name', [n for n in soak.MAGNITUDE_CASES if 'overflow' in n])
def test_brick_potentials_overflow(name):
    for case, rho, tol, dm, tg in inputs(name):
        with np.errstate(over='ignore'):
            f = brick_maxima(rho).astype(np.float32)
        assert np.isinf(f).any() and np.isfinite(rho).all()


@pytest.mark.parametrize('name', [n for n in soak.MAGNITUDE_CASES if 'negative' in n])
def test_negative_cases_hold_both_signs(name):
    for case, rho, tol, dm, tg in inputs(name):
        assert rho.min() < -3.9 and rho.max() > 0
        assert np.array_equal(rho, np.round((rho + 4.0) * 2.0 ** 20) * 2.0 ** -20 - 4.0), 'multiples of 2^-20 minus 4'
        if tol is not None:
            assert tol < 0 and 0 < (rho <= tol).mean() < 1


def same_as_plain(name):
    """the oracle on the case's densities and on the same densities without scale and offset (quantised alike)"""
    method, seed, scale, offset, tols = soak.MAGNITUDE_CASES[name]
    for (case, rho, tol, dm, tg) in inputs(name):
        base = synth.synth_density(case['shape'], case['lat'], synth.ATOMS8)
        plain, ptol = soak.finish_density(base, case, 0, None if offset is None else 0.0)
        assert np.array_equal(plain * 2.0 ** scale - (offset or 0.0) * 2.0 ** scale, rho), 'exact scaling and shift'
        a = soak.oracle_expectation(rho, tol, method, case['mode'], case['iters'], dm, tg)
        b = soak.oracle_expectation(plain, ptol, method, case['mode'], case['iters'], dm, tg)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (name, case['shape'], 'maxima / assignment')
        assert [tuple(x) for x in a[2]] == [tuple(x) for x in b[2]] and np.array_equal(a[3], b[3]), (name, case['shape'], 'refinement')


@pytest.mark.parametrize('name', [n for n in soak.MAGNITUDE_CASES if 'negative' in n or 'overflow' in n])
def test_the_oracle_is_invariant_under_shift_and_upscaling(name):
    same_as_plain(name)


def test_the_oracle_is_not_invariant_at_2_to_minus_140():
    """every step becomes an ongrid step: the expectation of the subnormal cases is the oracle's own map of the scaled density"""
    name = 'neargrid-subnormal'
    differs = 0
    for case, rho, tol, dm, tg in inputs(name):
        assert (max_grad(rho, tg) < 1E-14).all()
        a = soak.oracle_expectation(rho, tol, 'neargrid', case['mode'], case['iters'], dm, tg)
        b = soak.oracle_expectation(rho * 2.0 ** 140, tol, 'neargrid', case['mode'], case['iters'], dm, tg)
        differs += not np.array_equal(a[1], b[1])
    assert differs


def test_the_directed_case_hits_the_rounded_brick_maximum():
    import oracle
    from rough_common import own_map, rank_labels
    rho, dm, tg, tol, brick, m = soak.directed_vacuum_case()
    sl = tuple(slice(8 * b, 8 * b + 8) for b in brick)
    assert m == rho[sl].max()
    with np.errstate(under='ignore'):
        f = float(np.float32(m))
    assert f < m and f * (1 + 1e-6) < tol < m
    assert f + abs(f) * 1e-6 < tol, 'the relative margin alone calls this brick vacuum'
    assert not f + max(abs(f) * 1e-6, FLT_MIN) < tol, 'the floored margin does not'
    vol0, _, _ = oracle.vacuum_assign(rho, np.zeros(rho.shape, np.int32), tol, rho, 1.0)
    lab, maxima = rank_labels(own_map(rho, vol0, dm, tg, main_ties=True))
    assert (lab[sl] >= 0).any() and (lab[sl] == -1).any()
    # whole bricks do lie below the tolerance: the skip would be taken for them if the float image allowed it
    assert (rho.reshape(4, 8, 4, 8, 4, 8).max(axis=(1, 3, 5)) <= tol).any()
