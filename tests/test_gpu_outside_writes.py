"""GPU tests (-m gpu): labels written from outside an assignment between the steps of the ABI, on one context whose cached state
survives from call to call (the public functions re-upload labels and density on every call and never get here).

Grid V: xb_vacuum_assign (with the tolerance, or without one), then a writer -- xb_scatter_voxels or label planes through
xb_copy_planes --, then xb_assign(neargrid), xb_assign(ongrid) or xb_assign_refine(neargrid, all, -1).  With the tolerance the
fused route keeps the bricks that lie wholly below it off the walk list (XB_NOREC) as long as the -1 labels are provably
xb_vacuum_assign's: a label 0 written into such a brick must be walked (first finding: vac_by_tol).  Without a
tolerance the no-vacuum route writes every label itself: a scattered -1 must survive it (has_vacuum).

Grid S: xb_assign(neargrid), then a writer -- a scattered voxel deep inside a certified brick, four planes of another map,
xb_volume_assign, xb_import_labels of a device array, xb_vacuum_assign(tol) --, then xb_refine ('all', -1) and ('changed', 2): the
regions' labels, the bricks' uniformity, the edge lists and the vacuum flag of the assignment must not be trusted for labels it
did not write (test_gpu_neighbour_bits.test_stale_bits_are_never_trusted, extended from the table's neighbour bits to these).

Every expectation is the oracle's on the host-side image of the same sequence (outside_writes_common);
tests/test_outside_writes_cpu.py shows that every cell's expectation differs from the one without the writer.  The skip, the
regions and the bit sweep are shown to be active on the unpatched sequences by brick_labels(), box_stats() and sweep_stats().

Wall time on an MI355X box: 1.6 s for the 27 tests of this module, the oracle's expectations included (the slowest 0.12 s)."""
import numpy as np
import pytest

import outside_writes_common as W
from pybader_amd import _lib

pytestmark = pytest.mark.gpu

NOREC = np.iinfo(np.int32).min      # XB_NOREC: the brick label of a brick kept off the walk list


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def write(ctx, w):
    """the writer's calls; -> whatever must stay alive until the next call has run"""
    if w['kind'] == 'scatter':
        _, known = ctx.gather_voxels(w['idx'])
        ctx.scatter_voxels(w['idx'], w['labels'], known)
    elif w['kind'] == 'planes':
        ctx.copy_planes(0, 1, np.ascontiguousarray(w['planes']), w['xa'], w['xb'])
    elif w['kind'] == 'volume_assign':
        ctx.volume_assign(w['swap'])
    elif w['kind'] == 'import':
        dev = ctx.device_copy(np.ascontiguousarray(w['labels']))
        ctx.import_labels(dev)
        return dev
    elif w['kind'] == 'vacuum_assign':
        ctx.vacuum_assign(w['tol'], 1.0)
    else:
        raise KeyError(w['kind'])


def load_v(ctx, with_tol):
    rho, dm, tg, tol = W.grid_v()
    ctx.set_grid(rho.shape, dm, tg)
    ctx.upload_density(rho)
    ctx.vacuum_assign(tol if with_tol else None, 1.0)


def follow_v(ctx, follower):
    shape = W.grid_v()[0].shape
    got = {}
    if follower == 'neargrid_refine':
        n, log = ctx.assign_refine('neargrid', *W.V_REFINE)
        got['log'] = [tuple(x) for x in log]
    else:
        n = ctx.assign(follower)
    got['maxima'] = np.ravel_multi_index(tuple(ctx.maxima().T), shape) if n else np.zeros(0, np.int64)
    got['map'] = ctx.download_labels(np.int64)
    return got


def test_grid_v_unpatched_skips_the_vacuum_bricks(ctx):
    """the skip is under test: without a writer the assignment marks whole-vacuum bricks XB_NOREC -- every brick the writers
    write label 0 into among them -- and equals the oracle; without the tolerance no brick is marked"""
    load_v(ctx, True)
    got = follow_v(ctx, 'neargrid')
    blab = ctx.brick_labels()
    vac = W.v_vacuum_bricks()
    print('XB_NOREC bricks', int((blab == NOREC).sum()), 'of', blab.size, '; wholly below the tolerance', int(vac.sum()))
    assert (blab == NOREC).sum() > 0 and not (blab == NOREC)[~vac].any()
    for writer in W.V_WRITERS:
        assert all(blab[b] == NOREC for b in W.v_write(writer)['bricks']), writer
    assert W.same(got, W.v_expect(None, 'neargrid'))
    load_v(ctx, False)
    got = follow_v(ctx, 'neargrid')
    assert not (ctx.brick_labels() == NOREC).any()
    assert W.same(got, W.v_expect(None, 'neargrid', False))


@pytest.mark.parametrize('follower', W.V_FOLLOWERS)
@pytest.mark.parametrize('writer', list(W.V_WRITERS))
def test_grid_v_assignment_after_an_outside_write_equals_the_oracle(ctx, writer, follower):
    load_v(ctx, W.V_WRITERS[writer] == 'tol')
    keep = write(ctx, W.v_write(writer))
    got = follow_v(ctx, follower)
    del keep
    want = W.v_expect(writer, follower)
    assert len(got['maxima']) == len(want['maxima']) and np.array_equal(got['maxima'], want['maxima'])
    assert np.array_equal(got['map'], want['map']), int((got['map'] != want['map']).sum())
    assert got.get('log') == want.get('log')
    if W.v_write(writer)['bricks'] and follower != 'ongrid':    # the written bricks were walked this time
        blab = ctx.brick_labels()
        assert all(blab[b] != NOREC for b in W.v_write(writer)['bricks'])


def load_s(ctx):
    rho, dm, tg = W.grid_s()
    ctx.set_grid(rho.shape, dm, tg)
    ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('neargrid')
    assert n == len(W.s_assignment()[1])


def test_grid_s_unpatched_has_regions_and_sweeps_by_bit_masks(ctx):
    """the shortcuts are under test: the assignment certifies bricks -- the scattered voxel's among them --, the refinement's
    edge_find runs by row bit masks, and both equal the oracle"""
    for mode in W.S_REFINES:
        load_s(ctx)
        assert np.array_equal(ctx.download_labels(np.int32), W.s_assignment()[0])
        boxes, box_voxels = ctx.box_stats()
        blab = ctx.brick_labels()
        print('regions', boxes, 'voxels in them', box_voxels, 'certified bricks', int((blab > 0).sum()))
        assert boxes >= 1 and box_voxels >= 512 and (blab > 0).sum() * 512 == box_voxels
        assert blab[tuple(v // 8 for v in W.S_VOXEL)] > 0
        bits0, voxels0 = ctx.sweep_stats()
        log = [tuple(x) for x in ctx.refine(*mode)]
        bits1, voxels1 = ctx.sweep_stats()
        assert bits1 > bits0 and voxels1 == voxels0, 'edge_find by row bit masks'
        want = W.s_expect(None, mode)
        assert log == want['log'] and np.array_equal(ctx.download_labels(np.int32), want['map'])


@pytest.mark.parametrize('mode', W.S_REFINES)
@pytest.mark.parametrize('writer', W.S_WRITERS)
def test_grid_s_refinement_after_an_outside_write_equals_the_oracle(ctx, writer, mode):
    load_s(ctx)
    w = W.s_write(writer)
    keep = write(ctx, w)
    assert np.array_equal(ctx.download_labels(np.int32), w['start']), 'the writer left the map the expectation starts from'
    log = [tuple(x) for x in ctx.refine(*mode)]
    del keep
    got = ctx.download_labels(np.int32)
    want = W.s_expect(writer, mode)
    assert log == want['log'], (log, want['log'])
    assert np.array_equal(got, want['map']), int((got != want['map']).sum())
