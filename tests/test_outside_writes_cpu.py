"""What makes tests/test_gpu_outside_writes.py meaningful, checked on the CPU with the same expectations (outside_writes_common):
every cell's oracle result WITH the writer differs from the result WITHOUT it -- a library that ignored the write, or trusted what it
had cached from before the write, cannot pass the cell.  No cell is exempt.  Also: the inputs are what the cells say they are
(whole bricks below the tolerance, voxels written where they claim, -1 labels present or absent)."""
import numpy as np
import pytest

import outside_writes_common as W


def test_grid_v_has_whole_vacuum_bricks_next_to_others():
    rho, dm, tg, tol = W.grid_v()
    vac = W.v_vacuum_bricks()
    assert rho.shape == (32, 32, 32) and int(vac.sum()) == 50 and vac.size == 64
    assert (W.v_vacuum_map(True) == -1).reshape(4, 8, 4, 8, 4, 8).all(axis=(1, 3, 5)).sum() == 50
    assert not (W.v_vacuum_map(False) == -1).any()


@pytest.mark.parametrize('writer', list(W.V_WRITERS))
def test_grid_v_writers_write_where_they_say(writer):
    rho, dm, tg, tol = W.grid_v()
    w = W.v_write(writer)
    before = W.v_vacuum_map(W.V_WRITERS[writer] == 'tol')
    after = W.v_patched(writer)
    changed = np.argwhere(before != after)
    assert len(changed)
    vac = W.v_vacuum_bricks()
    if w['bricks']:     # label 0 into bricks that lie wholly below the tolerance, and nowhere else
        assert all(vac[b] for b in w['bricks'])
        assert {tuple(int(x) for x in c // 8) for c in changed} == set(w['bricks'])
        assert (after[before != after] == 0).all() and (rho[before != after] <= tol).all()
    else:               # -1 into voxels above the tolerance / into a map without vacuum
        assert (after[before != after] == -1).all()
        assert (rho[before != after] > tol).all() if w['kind'] == 'scatter' else not (before == -1).any()
    if w['kind'] == 'scatter':
        assert len(changed) == w['idx'].size


@pytest.mark.parametrize('follower', W.V_FOLLOWERS)
@pytest.mark.parametrize('writer', list(W.V_WRITERS))
def test_grid_v_the_write_changes_what_the_oracle_returns(writer, follower):
    with_w = W.v_expect(writer, follower)
    without = W.v_expect(None, follower, W.V_WRITERS[writer] == 'tol')
    assert not W.same(with_w, without)
    assert not np.array_equal(with_w['map'], without['map'])


def test_grid_s_is_what_the_module_says():
    rho, dm, tg = W.grid_s()
    lab, maxima = W.s_assignment()
    assert rho.shape == W.S_SHAPE == (16, 16, 128) and len(maxima) == 3
    assert [tuple(int(x) for x in np.unravel_index(m, W.S_SHAPE)) for m in maxima] == [(12, 4, 95), (4, 4, 32), (4, 12, 81)]
    # fewer than one maximum per 8 bricks (the bit sweep's condition), whole sweep tiles of 4 x 8 x 64
    assert 8 * len(maxima) < rho.size // 512 and rho.shape[0] % 4 == 0 and rho.shape[1] % 8 == 0 and rho.shape[2] % 64 == 0
    # the scattered voxel: the centre of a brick whose 10^3 surroundings carry one label -- deep inside its basin
    x, y, z = W.S_VOXEL
    assert (x % 8, y % 8, z % 8) == (4, 4, 4)
    around = np.take(np.take(np.take(lab, range(x - 5, x + 5), 0, mode='wrap'), range(y - 5, y + 5), 1, mode='wrap'), range(z - 5, z + 5), 2, mode='wrap')
    assert (around == lab[W.S_VOXEL]).all()


@pytest.mark.parametrize('writer', W.S_WRITERS)
def test_grid_s_writers_leave_another_valid_map(writer):
    lab, maxima = W.s_assignment()
    w = W.s_write(writer)
    start = w['start']
    assert start.shape == lab.shape and not np.array_equal(start, lab)
    assert start.min() >= (-1 if writer == 'vacuum_assign_tol' else 0) and start.max() < len(maxima)
    if writer == 'scatter_foreign_label':
        assert (start != lab).sum() == 1 and start[W.S_VOXEL] != lab[W.S_VOXEL]
    if writer == 'planes_of_another_map':
        assert {int(c[0]) for c in np.argwhere(start != lab)} == {6, 7, 8, 9}


@pytest.mark.parametrize('mode', W.S_REFINES)
@pytest.mark.parametrize('writer', W.S_WRITERS)
def test_grid_s_the_write_changes_what_the_oracle_returns(writer, mode):
    with_w, without = W.s_expect(writer, mode), W.s_expect(None, mode)
    # (a retrace may heal the written voxels: then the log tells the two apart -- the edges found and the voxels changed)
    assert with_w['log'] != without['log'] or not np.array_equal(with_w['map'], without['map'])
