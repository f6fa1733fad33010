"""The constructions of tests/capacity_common.py against the CPU oracle, and the arithmetic that puts every case of
tests/test_gpu_capacity.py on its side of a fixed capacity of the assignment pipeline.  The GPU file trusts density A's closed
form at sizes no oracle is run for; this file is why it may.  If a constant of k_fused.h / host_context.h moves, the test that
fails here names the case that no longer straddles it."""
import os
import re

import numpy as np
import pytest

import capacity_common as cc

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pybader_amd', 'csrc')


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def define(text, name):
    m = re.search(r'^#define\s+' + name + r'\s+(\d+)\b', text, re.M)
    assert m, f'{name} is no longer a plain #define'
    return int(m.group(1))


def test_the_capacities_are_what_the_cases_were_chosen_for():
    fused = source('k_fused.h')
    assert define(fused, 'XB_BOXES_MAX') == cc.XB_BOXES_MAX
    assert define(fused, 'XB_SORT_MAX') == cc.XB_SORT_MAX
    assert define(fused, 'XB_REGIONS_MAX') == cc.XB_REGIONS_MAX
    # k_rank_blocks: one workgroup of 1024 scans 1024 block sums per round
    body = fused[fused.index('void k_rank_blocks('):]
    body = body[:body.index('\n}\n')]
    assert f'base += {cc.RANK_BLOCKS_PER_ROUND}' in body and 'carry += total' in body
    assert '__launch_bounds__(1024) void k_rank_blocks(' in fused
    # the bitmap numbering: 32 voxels per word, 1024 words per workgroup of k_rank_scan
    big = source('host_assign.h')
    assert 'n_words = (c->N + 31) / 32, n_blocks = (n_words + 1023) / 1024' in big
    # the maxima table
    assert 'c->max_cap = (int)std::min<long long>(N, 1 << 22);' in source('host_context.h')
    assert cc.MAX_CAP == 1 << 22
    # box_max is a window of 2^16 ints directly in front of box_first: region ids 1 .. XB_REGIONS_MAX index 0 .. 65534 of it
    assert 'BB_REGMAX = 1 << 16, BB_REGFIRST = 1 << 17' in source('host_stages.h')
    assert cc.XB_REGIONS_MAX <= (1 << 17) - (1 << 16)


def test_the_shapes_straddle_the_capacities():
    assert all(s % 8 == 0 for shape in (*cc.REGION_SHAPES.values(), cc.REGION_SHAPE_SMALL, *cc.SORT_SHAPES.values(),
                                        *cc.SEED_SHAPES.values(), cc.B_NEARGRID_SHAPE) for s in shape)
    # regions: below, at, above XB_BOXES_MAX
    assert {k: cc.n_bricks(s) for k, s in cc.REGION_SHAPES.items()} == {1008: 1008, 1024: 1024, 1056: 1056}
    assert sorted(cc.REGION_SHAPES) == [1008, cc.XB_BOXES_MAX, 1056] and 1008 < cc.XB_BOXES_MAX < 1056
    assert cc.n_bricks(cc.REGION_SHAPE_SMALL) == cc.XB_BOXES_MAX
    # the full-size brick kernels from 80 voxels along z on (host_stages.h, small_grid)
    assert all(min(s[:2]) >= 16 and s[2] >= 80 for s in (*cc.REGION_SHAPES.values(), *cc.SORT_SHAPES.values(), *cc.SEED_SHAPES.values()))
    assert cc.REGION_SHAPE_SMALL[2] < 80 and min(cc.REGION_SHAPE_SMALL) >= 16
    # maxima: below, at, above XB_SORT_MAX
    assert {k: cc.n_bricks(s) for k, s in cc.SORT_SHAPES.items()} == {2040: 2040, 2048: 2048, 2057: 2057}
    assert sorted(cc.SORT_SHAPES) == [2040, cc.XB_SORT_MAX, 2057] and 2040 < cc.XB_SORT_MAX < 2057
    # the small cases hold about a million voxels at the most (2057 bricks: 1 053 184)
    assert all(cc.n_voxels(s) <= 2057 * 512 for s in (*cc.REGION_SHAPES.values(), cc.REGION_SHAPE_SMALL, *cc.SORT_SHAPES.values()))
    # seeds: below, one above, well above XB_REGIONS_MAX
    assert {k: cc.n_bricks(s) for k, s in cc.SEED_SHAPES.items()} == {64512: 64512, 65536: 65536, 67584: 67584}
    assert 64512 < cc.XB_REGIONS_MAX and 65536 == cc.XB_REGIONS_MAX + 1
    # k_rank_blocks: below one round, exactly one round, one round and a carry
    assert [cc.n_rank_blocks(cc.SEED_SHAPES[k]) for k in (64512, 65536, 67584)] == [1008, 1024, 1056]
    assert cc.n_rank_blocks(cc.EXACT_ROUND_SHAPE) == cc.RANK_BLOCKS_PER_ROUND < cc.n_rank_blocks(cc.CARRY_SHAPE)
    # ... and every one of those takes the bitmap numbering: more maxima than the LDS sort holds
    assert all(k > cc.XB_SORT_MAX for k in cc.SEED_SHAPES)
    # the largest bitmap-numbered grid of the suite before these cases: 256^3, 512 blocks, half a round
    assert cc.n_rank_blocks((256, 256, 256)) == 512
    # density B: N / 8 maxima
    assert cc.n_voxels(cc.B_FITS_SHAPE) // 8 == 4194304 == cc.MAX_CAP
    assert cc.n_voxels(cc.B_OVER_SHAPE) // 8 == 4325376 > cc.MAX_CAP
    # the walkers' list for the exact slow path, ovf_cap = min(N, max(2^22, N / 16)): the whole grid at B's neargrid shape
    n = cc.n_voxels(cc.B_NEARGRID_SHAPE)
    assert min(n, max(1 << 22, n // 16)) == n
    # the largest case: 34.6 M voxels
    assert max(cc.n_voxels(s) for s in cc.SEED_SHAPES.values()) == 34603008


@pytest.fixture(scope='module', params=[(32, 40, 48), (128, 64, 128)], ids=lambda s: 'x'.join(map(str, s)))
def case_a(request):
    shape = request.param
    return shape, cc.density_a(shape)


def test_density_a_is_what_the_issue_states(case_a):
    shape, rho = case_a
    x, y, z = 13, 22, 7
    assert rho[x, y, z] == 2 + cc.F8[x % 8] + 1.25 * cc.F8[y % 8] + 1.5 * cc.F8[z % 8]
    assert rho.shape == shape and rho.dtype == np.float64 and rho.flags.c_contiguous
    # every brick repeats the first one bit for bit
    assert np.array_equal(rho, np.tile(rho[:8, :8, :8], tuple(s // 8 for s in shape)))
    lab, mx = cc.labels_a(shape), cc.maxima_a(shape)
    assert lab.dtype == np.int32 and mx.shape == (cc.n_bricks(shape), 3)
    assert np.array_equal(lab[tuple(mx.T)], np.arange(cc.n_bricks(shape)))
    assert np.array_equal(np.bincount(lab.reshape(-1)), np.full(cc.n_bricks(shape), 512))


def test_density_a_ongrid_is_the_closed_form(case_a):
    shape, rho = case_a
    bmax, lab = cc.oracle_ongrid(rho, shape)
    assert bmax.shape[0] == cc.n_bricks(shape)
    assert np.array_equal(bmax, cc.maxima_a(shape))
    assert np.array_equal(lab, cc.labels_a(shape))


def test_density_a_own_trajectory_map_is_the_closed_form(case_a):
    shape, rho = case_a
    bmax, lab = cc.oracle_neargrid(rho, shape)
    assert bmax.shape[0] == cc.n_bricks(shape)
    assert np.array_equal(bmax, cc.maxima_a(shape))
    assert np.array_equal(lab, cc.labels_a(shape))


def test_density_a_is_a_fixed_point_of_the_refinement():
    """the GPU cases at the sort boundary assert the log [(edges, 0), ...] and an unchanged map: so says the oracle, in both modes"""
    shape = cc.SORT_SHAPES[2048]
    rho, want = cc.density_a(shape), cc.labels_a(shape)
    for mode in (('changed', 2), ('all', 2)):
        got, log = cc.oracle_refine(rho, want, shape, mode)
        assert np.array_equal(got, want)
        assert len(log) >= 1 and log[0] == (cc.edges_a(shape), 0) and all(ch == 0 for _, ch in log), log
    assert cc.edges_a(shape) == 296 * 2048


@pytest.fixture(scope='module', params=[(32, 40, 48), cc.B_NEARGRID_SHAPE], ids=lambda s: 'x'.join(map(str, s)))
def case_b(request):
    shape = request.param
    return shape, cc.density_b(shape)


def test_density_b_has_a_maximum_on_every_all_even_voxel(case_b):
    shape, rho = case_b
    even = cc.maxima_b_sorted(shape)
    assert even.shape[0] == cc.n_voxels(shape) // 8
    # by construction: all-even voxels hold at least 1, every other voxel less than 0.5
    mask = np.zeros(shape, bool)
    mask[tuple(even.T)] = True
    assert rho[mask].min() >= 1.0 and rho[~mask].max() < 0.5
    for name, calc in (('ongrid', cc.oracle_ongrid), ('neargrid', cc.oracle_neargrid)):
        bmax, lab = calc(rho, shape)
        assert bmax.shape[0] == cc.n_voxels(shape) // 8, name
        assert np.array_equal(cc.sort_rows(bmax), even), name
        assert lab.min() == 0 and lab.max() == bmax.shape[0] - 1, name
        assert np.array_equal(lab[tuple(bmax.T)], np.arange(bmax.shape[0])), name


def test_density_b_maps_differ_between_the_methods_and_move_under_refinement():
    """why each method needs its own oracle map on B, and which refinement of B is no identity: the own-trajectory map is the
    refinement's fixed point here too, the ONGRID map is not -- its first iteration relabels 233 725 of the 524 288 voxels and the
    second none, in both modes.  The GPU file refines both maps."""
    shape = cc.B_NEARGRID_SHAPE
    rho = cc.density_b(shape)
    _, og = cc.oracle_ongrid(rho, shape)
    _, ng = cc.oracle_neargrid(rho, shape)
    assert not np.array_equal(og, ng)
    edges = cc.n_voxels(shape) * 7 // 8          # every voxel but the maxima's own has a neighbour of another basin
    for mode in (('changed', 2), ('all', 2)):
        got, log = cc.oracle_refine(rho, ng, shape, mode)
        assert np.array_equal(got, ng) and log[0] == (edges, 0) and all(ch == 0 for _, ch in log), log
        got, log = cc.oracle_refine(rho, og, shape, mode)
        assert len(log) == 2 and log[0] == (edges, 233725) and log[1][1] == 0, log      # converges in the second iteration
        assert int((got != og).sum()) == 233725
