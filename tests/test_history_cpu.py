"""The check of the check for tests/test_gpu_history.py (no GPU): the inputs of tests/history_common.py tell a stale upload from a
fresh one for every call kind -- the Hirshfeld, ISA, NCI, isosurface, regions, MBIS, moments, DORI and IGM kinds included --, the
seeded walks reach every kind and every event, no generated step is left out, the oracle-built maps are converged, and the newer
analyses' expectations are no empty sets on any grid (voxels no pro-atom reaches, no empty ISA shell, two components, two NCI
domains, meshes, shares, non-zero moments, DORI and IGM regions of 100 and 50 voxels with a component to label)."""
import collections

import numpy as np
import pytest

import history_common as H
import oracle


@pytest.mark.parametrize('grid', list(H.GRIDS))
def test_every_kind_tells_the_two_inputs_apart(grid):
    """the expectation for (B, atoms) handed to check() as the result of the call on (A, bader) is reported, for every kind: a
    call that read the density or the map of the call before it cannot pass.  The kinds that read only one of the two are told
    apart by that one alone, so the same holds for each input singly where the kind reads it."""
    for kind, (reads_d, reads_m) in H.KINDS.items():
        mine = ('A', 'bader')
        assert H.check(kind, H.as_result(kind, H.expect(kind, grid, *mine), grid), (grid,) + mine) is None, kind
        others = [('B', 'atoms')] + ([('B', 'bader')] if reads_d else []) + ([('A', 'atoms'), ('A', 'noise')] if reads_m else [])
        for other in others:
            msg = H.check(kind, H.as_result(kind, H.expect(kind, grid, *other), grid), (grid,) + mine)
            assert msg is not None and msg.startswith(f'{kind} on {grid} density A map bader: '), (kind, other, msg)


def test_the_newer_kinds_accept_their_own_expectation_on_every_input_a_walk_can_draw():
    """the comparisons of the regions, domains and NCI kinds also ask that the expectation is no empty set (2 components, 50
    shared voxels, 100 counted ones): that holds on every grid, density and map, so a walk's step cannot fail on its input"""
    new = list(H.KINDS)[list(H.KINDS).index('hirshfeld_charges'):]
    for grid in H.GRIDS:
        for kind in new:
            for d in H.densities(grid):
                for m in H.maps(grid):
                    assert H.check(kind, H.as_result(kind, H.expect(kind, grid, d, m), grid), (grid, d, m)) is None


def test_the_float32_density_is_told_from_the_float64_one():
    """setting 4 of the pair matrix computes its expectations from A32.astype(float64): they differ from A's wherever the kind
    returns a float, so a device import that is not the tensor's content cannot pass"""
    # every new kind that returns a float: all but promolecule and mbis_promolecule, which read no density, and nci_histogram,
    # which returns counts (the moments' integer bins differ as well; igm_fields_pro differs in x alone)
    new = [k for k in H.KINDS if k.startswith(('hirshfeld_charges', 'deformation', 'isa_', 'nci_', 'isosurface', 'regions', 'mbis_',
                                               'hirshfeld_moments', 'dori_', 'igm_'))
           and k not in ('nci_histogram', 'mbis_promolecule')]
    assert len(new) == 35
    for kind in ['charge_sum', 'volume_mask', 'weight_own', 'moment_sum', 'laplacian', 'basin_laplacian', 'point_properties'] + new:
        got = H.as_result(kind, H.expect(kind, 'G1', 'A32', 'bader'), 'G1')
        assert H.check(kind, got, ('G1', 'A', 'bader')) is not None, kind


def test_the_walks_reach_every_kind_and_every_event_and_leave_no_step_out():
    calls, events, total, runnable = collections.Counter(), collections.Counter(), 0, 0
    for seed in H.SEEDS:
        steps = H.walk(seed)
        assert steps == H.walk(seed), 'the walk is a function of its seed'
        assert 175 <= len(steps) <= 190, len(steps)
        grid, inside = 'G1', False
        for s in steps:
            total += 1
            op = s['op']
            assert op in ('call', 'enter', 'leave', 'grid', 'mutate', 'fail'), op
            if op == 'grid':
                assert s['grid'] in H.GRIDS and s['grid'] != grid
                grid = s['grid']
                events['shape'] += 1
            else:
                assert s['grid'] == grid
            if op in ('call', 'mutate', 'fail'):
                assert s['kind'] in H.KINDS and s['dname'] in H.densities(grid) and s['mname'] in H.maps(grid), s
                calls[s['kind']] += 2 if op == 'mutate' else 1
            if op == 'enter':
                assert not inside and s['dname'] in ('A', 'B')
                inside = True
                events['resident'] += 1
            if op == 'leave':
                assert inside
                inside = False
            if op == 'mutate':
                assert not inside, 'an in-place edit belongs outside resident()'
                reads_d, reads_m = H.KINDS[s['kind']]
                assert reads_d if s['what'] == 'density' else reads_m
                events['mutate'] += 1
            if op == 'fail':
                assert s['how'] in H.FAILURES
                events['fail'] += 1
            runnable += 1                       # (nothing above let a step through without a branch that runs it)
        assert not inside, 'every walk leaves resident() at its end'
    assert set(calls) == set(H.KINDS) and min(calls.values()) >= 5, sorted(calls.items(), key=lambda kv: kv[1])[:5]
    assert set(events) == set(H.EVENTS) and min(events.values()) >= 3, events
    assert (total - runnable) / total == 0.0


def test_the_edits_of_the_walks_show_in_the_expectation():
    """every 'mutate' step: the expectation after the edit, taken for the result before it, is reported"""
    seen = 0
    for seed in H.SEEDS:
        for s in H.walk(seed):
            if s['op'] != 'mutate':
                continue
            kind, grid, d, m = s['kind'], s['grid'], s['dname'], H.map_for(s['kind'], s['mname'])
            d2, m2 = (d + '+', m) if s['what'] == 'density' else (d, m + '+')
            after = H.as_result(kind, H.expect(kind, grid, d2, m2), grid)
            assert H.check(kind, after, (grid, d2, m2)) is None, s
            assert H.check(kind, after, (grid, d, m)) is not None, s
            seen += 1
    assert seen >= 3
    # ... and of the kinds added with the nine newest analyses, at least 30 can be drawn for such a step
    new = list(H.KINDS)[list(H.KINDS).index('hirshfeld_charges'):]
    assert len(new) == 38 and sum(H.check(k, H.as_result(k, H.expect(k, 'G1', 'A+', 'bader'), 'G1'), ('G1', 'A', 'bader')) is not None
                                  for k in new if H.KINDS[k][0] and k != 'isosurface_of_field') >= 30


NEWEST = list(H.KINDS)[list(H.KINDS).index('mbis_charges'):]      # the MBIS, moments, DORI and IGM kinds


def edit_shows(kind, what, grid, d, m):
    """the expectation after the edit of a 'mutate' step is its own, and is reported when taken for the result before the edit"""
    d2, m2 = (d + '+', m) if what == 'density' else (d, m + '+')
    after = H.as_result(kind, H.expect(kind, grid, d2, m2), grid)
    assert H.check(kind, after, (grid, d2, m2)) is None, (kind, what, grid, d, m)
    return H.check(kind, after, (grid, d, m)) is not None


def test_the_newest_kinds_show_both_edits_on_every_input():
    """walk() leaves no MBIS, moments, DORI or IGM kind out of either edit: the corner block's edit shows in the expectation of
    every one of them on every (grid, density, map) a walk can draw"""
    assert len(NEWEST) == 19
    inputs = [(g, d, m) for g in H.GRIDS for d in H.densities(g) for m in H.maps(g)]
    for kind in NEWEST:
        reads_d, reads_m = H.KINDS[kind]
        if reads_d:
            assert all(edit_shows(kind, 'density', *i) for i in inputs), kind
        if reads_m:
            assert all(edit_shows(kind, 'labels', *i) for i in inputs), kind
    drawn = {s['kind'] for seed in H.SEEDS for s in H.walk(seed) if s['op'] == 'mutate'}
    assert drawn & set(NEWEST)
    # (mode 'pro' takes the free atoms' own gradients: without x the density would not show in igm_fields_pro at all)
    before, after = H.expect('igm_fields_pro', 'G1', 'A', 'atoms'), H.expect('igm_fields_pro', 'G1', 'A+', 'atoms')
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]) and not np.array_equal(before[2], after[2])


def test_the_oracle_built_maps_are_converged():
    """one more refinement of each Bader map changes nothing: the parity of the README applies to them"""
    for grid in H.GRIDS:
        for dname in H.densities(grid):
            b = H.bader(grid, dname)
            v, log = b['refined'].copy(), []
            oracle.refine('neargrid', H.REFINE_MODE, H.density(grid, dname), v, *H.geometry(grid), 1, log=log)
            assert np.array_equal(v, b['refined']) and all(changed == 0 for _, changed in log), (grid, dname, log)
            assert b['log'] == [] or b['log'][-1][1] == 0, (grid, dname, b['log'])


def test_the_inputs_are_what_the_issue_asks_for():
    assert any(s % 8 for s in H.GRIDS['G1']) and H.GRIDS['G1'][2] < 32
    assert H.GRIDS['G2'][0] < 10 and H.GRIDS['G2'][1] < 8 and H.GRIDS['G2'][2] == 33
    g1, g3 = H.GRIDS['G1'], H.GRIDS['G3']
    assert g3[0] > g1[0] and g3[1] < g1[1] and g3[2] < g1[2]
    assert len({int(np.prod(s)) for s in H.GRIDS.values()}) == 3
    for grid in H.GRIDS:
        noise = H.labels(grid, 'noise')
        assert noise.min() == -1 and noise.max() >= H.n_of(grid, 'noise')
        for m in H.maps(grid):
            if m != 'baderN':
                assert H.labels(grid, m).max() < len(H.SITES8)      # surface_distance indexes its sites by label
        vac = H.vacuum_map(grid, 'A') == -1
        assert 0 < vac.sum() < vac.size
    # the merge has something to merge on the noisy density, and does not merge everything
    want, _ = H.expect('merge', 'G1', 'N', 'baderN')
    assert 1 < want['n_survivors'] < H.n_of('G1', 'baderN') and want['converged']
    # the five newest analyses have something to say on every grid and both densities
    for grid in H.GRIDS:
        for d in ('A', 'B'):
            s = H.expect('hirshfeld_charges', grid, d, 'atoms')
            assert s['rest'][1] > 0 and (s['count'] >= 100).all(), 'voxels no pro-atom reaches, and every atom weighs voxels'
            g = H._isa(grid, d)[0]
            assert (g.count > 0).all(), 'no ISA shell is empty'
            assert H.expect('regions', grid, d, 'atoms')['seeds'].size >= 2 and H.expect('regions_below', grid, d, 'atoms')['seeds'].size >= 1
            assert H.expect('nci_domains', grid, d, 'atoms')['seeds'].size >= 2
            for kind in ('isosurface', 'isosurface_of_field'):
                mesh = H.expect(kind, grid, d, 'atoms')
                assert mesh.vertices.shape[0] > 100 and mesh.triangles.shape[0] > 100, (kind, grid, d)
            for kind in ('regions', 'regions_below', 'regions_of_field', 'nci_domains'):
                assert H.expect(kind, grid, d, 'atoms')['shares'][2].sum() >= 50, (kind, grid, d)
            assert H.expect('nci_regions', grid, d, 'atoms')[0][1].sum() >= 100 and H.expect('nci_histogram', grid, d, 'atoms')[0].sum() > 100


def test_the_mbis_moments_dori_and_igm_inputs_say_something_on_every_input_a_walk_can_draw():
    """no voxel beyond the bound, every stockholder bin non-zero, every MBIS shell alive; the DORI and IGM regions hold the voxels
    their comparisons ask for (100 and 50, with a label the sums count) and at least one component, the meshes are no empty sets;
    stockholder IGM has voxels above 0.01 where pro-mode IGM is nearly zero, which is why the regions use it"""
    for grid in H.GRIDS:
        for d in H.densities(grid):
            g, e, rows, (N, sigma), bound = H._mbis(grid, d)
            assert (g.count > 0).all() and (N[H.MBIS_SHELLS[:, None] > np.arange(2)[None, :]] > 0).all(), (grid, d)
            assert len(rows) == H.MBIS['max_iter'] == 5 and H.MBIS['check_every'] == 2 and bound == float(np.abs(H.density(grid, d)).max())
            for kind in ('hirshfeld_moments', 'isa_moments', 'mbis_moments'):
                bins, info, _ = H.expect(kind, grid, d, 'atoms')
                assert (bins != 0).all() and info['beyond_bound'] == 0 and info['pairs'] > 1000, (kind, grid, d)
            dgi = H.expect('igm_fields', grid, d, 'atoms')[1]
            assert (dgi > 0.01).sum() >= (88 if d != 'B' else 25), (grid, d, int((dgi > 0.01).sum()))
            assert H.expect('igm_fields_pro', grid, d, 'atoms')[1].max() < 6.5e-3
            for kind in ('dori_isosurface', 'igm_isosurface'):
                assert H.expect(kind, grid, d, 'atoms').triangles.shape[0] > 100, (kind, grid, d)
            for m in H.maps(grid):
                assert H.expect('dori_regions', grid, d, m)[0][1].sum() >= 100, (grid, d, m)
                assert H.expect('igm_regions', grid, d, m)[0][1].sum() >= 50, (grid, d, m)
                for kind in ('dori_domains', 'igm_domains'):
                    want = H.expect(kind, grid, d, m)
                    assert want['seeds'].size >= 1 and want['count'].sum() >= 50 and want['shares'][2].sum() >= 50, (kind, grid, d, m)
    # both sides of the class bound occur in the DORI region of every grid, and in the IGM region of the noisy density
    for grid in H.GRIDS:
        cnt = H.expect('dori_regions', grid, 'A', 'atoms')[0][1]
        assert cnt[0::3].sum() > 100 and cnt[1::3].sum() > 100, grid
    cnt = H.expect('igm_regions', 'G1', 'N', 'atoms')[0][1]
    assert cnt[0::3].sum() > 100 and cnt[1::3].sum() > 100
