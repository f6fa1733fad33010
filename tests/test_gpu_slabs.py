"""GPU slab path on ONE GPU: N contexts (one per logical rank) on the same device, driven by N Python
threads through the product's SlabRunner + GpuBackend; halo planes move between the contexts through
the same zero-copy torch views of the device arrays that the RCCL transport uses on a multi-GPU node.
The assembled map must equal the 1-GPU result bit for bit (multi-GPU row)."""
import threading

import numpy as np
import pytest

from conftest import case_density, load_golden
from pybader_amd import _lib, slab, synth
from pybader_amd.interface import distance_matrix, gradient_transform
from torch_comm import block_view, device_views

pytestmark = pytest.mark.gpu


class Shared:
    def __init__(self, n):
        self.n = n
        self.barrier = threading.Barrier(n)
        self.slots = [None] * n
        self.cur = [None] * n
        self.errors = []


class ThreadComm:
    def __init__(self, shared, rank):
        self.sh, self.rank, self.size = shared, rank, shared.n

    def allgather(self, obj):
        self.sh.slots[self.rank] = obj
        self.sh.barrier.wait()
        out = list(self.sh.slots)
        self.sh.barrier.wait()
        return out

    def sum(self, *vals):
        got = self.allgather([int(v) for v in vals])
        return [sum(g[i] for g in got) for i in range(len(vals))]

    def exchange_planes(self, backend, which, sends, recvs):
        import torch
        torch.cuda.synchronize()
        tensor = device_views(backend.ctx)[which]
        self.sh.cur[self.rank] = tensor
        self.sh.barrier.wait()
        for peer, xa, xb in recvs:
            tensor[xa:xb].copy_(self.sh.cur[peer][xa:xb])
        torch.cuda.synchronize()
        self.sh.barrier.wait()

    def share_brick_masks(self, backend, chunks):
        import torch
        views = device_views(backend.ctx)
        for tensor in (views[2], views[3]):      # the move masks, then the bricks' single-maximum voxels
            self.sh.cur[self.rank] = tensor
            self.sh.barrier.wait()
            for r, (first, count) in enumerate(chunks):
                if r != self.rank and count:
                    tensor[first:first + count].copy_(self.sh.cur[r][first:first + count])
            torch.cuda.synchronize()
            self.sh.barrier.wait()

    def gather_rows(self, rows):
        return np.concatenate(self.allgather(np.ascontiguousarray(rows, np.int64)))

    # the exchange blocks of the device-driven step: device-to-device copies between the contexts of this one card
    stream_ordered = True      # (this transport waits for the whole card itself, before and after its copies)

    def allgather_block(self, backend, which, parts):
        import torch
        torch.cuda.synchronize()
        mine = block_view(backend.ctx, which)
        self.sh.cur[self.rank] = mine
        self.sh.barrier.wait()
        for r, (off, n) in enumerate(parts):
            if r != self.rank and n:
                mine[off:off + n].copy_(self.sh.cur[r][off:off + n])
        torch.cuda.synchronize()
        self.sh.barrier.wait()

    def allreduce_block(self, backend):
        import torch
        torch.cuda.synchronize()
        mine = block_view(backend.ctx, 5).view(torch.int64)
        self.sh.cur[self.rank] = mine
        self.sh.barrier.wait()
        total = torch.stack([t[:8] for t in self.sh.cur]).sum(0)
        torch.cuda.synchronize()
        self.sh.barrier.wait()
        mine[8:16].copy_(total)
        torch.cuda.synchronize()
        self.sh.barrier.wait()

    def barrier(self):
        self.sh.barrier.wait()


class ShadowRcclComm(ThreadComm):
    """ThreadComm whose block exchanges first go through the library's RCCL entry points on a ONE-rank communicator per
    context (the collectives are identities there: this rank's part from itself, sums of one) -- the calls, pointers and
    byte ranges of a node run, in the order of a node run -- and then do the real copies between the contexts."""

    def allgather_block(self, backend, which, parts):
        off, n = parts[self.rank]
        backend.ctx.comm_allgather_block(which, [off], [n])
        super().allgather_block(backend, which, parts)

    def allreduce_block(self, backend):
        backend.ctx.comm_allreduce_block()
        super().allreduce_block(backend)


def run_slabs(n, g, rho, method, mode, iters, halo, tol, window=True, shape=None, synth_args=None, label_dtype=np.int32,
              keep_pre=True, margin=8, comm_cls=ThreadComm, options=()):
    """rho=None + synth_args=(lattice, atoms, background): every context generates the density on the device"""
    shape = rho.shape if rho is not None else tuple(shape)
    sh = Shared(n)
    res = [None] * n

    def work(rank):
        try:
            ctx = _lib.Context(0)
            comm = comm_cls(sh, rank)
            for key, value in options:
                ctx.set_option(key, value)
            if comm_cls is ShadowRcclComm:
                ctx.comm_init(0, 1, ctx.comm_unique_id())
            runner = slab.SlabRunner(slab.GpuBackend(ctx, 0), comm, shape, g['dist_mat'], g['T_grad'], halo=halo)
            win = runner.enable_table_window(margin) if window else False
            if rho is not None:
                ctx.upload_density(rho)
            else:
                ctx.synth_density(*synth_args)
            ctx.vacuum_assign(tol, 1.0)
            w0 = ctx.host_waits()
            nb = runner.assign(method)
            w1 = ctx.host_waits()
            x0, x1 = runner.x_range
            pre = ctx.download_labels(label_dtype)[x0:x1].copy() if keep_pre else np.zeros((0,) + tuple(shape[1:]), label_dtype)
            w2 = ctx.host_waits()
            log = runner.refine(mode, iters)
            w3 = ctx.host_waits()
            post = ctx.download_labels(label_dtype)[x0:x1].copy()
            ch, vo = ctx.charge_sum(1.0, nb)
            res[rank] = (x0, pre, post, log, runner.maxima, ch, vo, runner.n_fallbacks, win, ctx.slow_path_stats(), ctx.memory_stats(), runner.n_device_steps, (w1 - w0, w3 - w2), ctx.growth_stats(), bool(getattr(runner, '_step_declined', False)))
            ctx.close()
        except Exception as e:  # noqa: BLE001
            sh.errors.append(repr(e))
            sh.barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not sh.errors, sh.errors
    res.sort(key=lambda r: r[0])
    pre = np.concatenate([r[1] for r in res])
    post = np.concatenate([r[2] for r in res])
    ch = sum(r[5] for r in res)
    vo = sum(r[6] for r in res)
    run_slabs.last_windowed = [r[8] for r in res]
    run_slabs.last_slow = [r[9] for r in res]
    run_slabs.last_memory = [r[10] for r in res]
    run_slabs.last_device_steps = [r[11] for r in res]
    run_slabs.last_host_waits = [r[12] for r in res]
    run_slabs.last_growth = [r[13] for r in res]
    run_slabs.last_declined = [r[14] for r in res]
    print('device-driven steps per rank:', run_slabs.last_device_steps)
    return pre, post, res[0][3], res[0][4], ch, vo, max(r[7] for r in res)


def tol_of(g):
    t = float(g['vacuum_tol'])
    return None if np.isnan(t) else t


@pytest.mark.parametrize('n,name,mode,iters,halo', [
    (2, 'c64_cubic', 'changed', 2, 8),
    (4, 'c64_cubic', 'all', -1, 8),
    (3, 'c40x48x56_tric', 'changed', 2, 8),
    (2, 'c48_cubic_vac', 'all', 2, 6),
    (8, 'c64_cubic', 'changed', 2, 4),
])
def test_neargrid_slabs_equal_one_gpu(n, name, mode, iters, halo):
    g = load_golden(name)
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, rho, 'neargrid', mode, iters, halo, tol_of(g))
    assert np.array_equal(pre, g['ng_F'].astype(np.int32))
    key = f"ng_{mode}_{'inf' if iters < 0 else iters}"
    assert np.array_equal(post, g[key].astype(np.int32))
    assert np.array_equal(np.array(np.unravel_index(maxima, rho.shape)).T, g['ng_bader_max'])
    np.testing.assert_allclose(ch * float(g['voxel_volume']), g['ng_bader_charge'], rtol=1e-9)
    assert all(c == 0 for _, c in log)


@pytest.mark.parametrize('n,name,halo', [(2, 'c64_cubic', 8), (3, 'c40x48x56_tric', 3), (4, 'c40x48x56_tric', 8)])
def test_ongrid_plus_refine_all_slabs_equal_oracle(n, name, halo):
    """ongrid start => many voxels change during refinement (exercises halo refresh between
    iterations and, with the 3-plane halo, the escape fallback)."""
    import oracle
    g = load_golden(name)
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, rho, 'ongrid', 'all', 3, halo, tol_of(g))
    assert np.array_equal(pre, g['og_main'].astype(np.int32))
    v = g['og_main'].astype(np.int32)
    olog = []
    oracle.refine('neargrid', ('all', 3), rho, v, g['dist_mat'], g['T_grad'], 1, log=olog)
    assert log == [tuple(x) for x in olog]
    assert np.array_equal(post, v)
    if halo == 3:
        assert fb > 0, 'the narrow halo is meant to exercise the escape fallback'


@pytest.mark.parametrize('n,name,tag,halo', [(2, 'r64_noise04', 'ng_all_inf', 8), (4, 'r64_noise04', 'ng_changed_2', 8),
                                             (2, 'r40_noise04', 'ng_changed_inf', 6), (3, 'r48_sig5', 'ng_all_inf', 8),
                                             (2, 'r48_sig5_noise', 'ng_changed_2', 8), (2, 'r40_vac_noise', 'ng_changed_2', 8),
                                             (2, 'r32_quant8', 'ng_all_inf', 8), (4, 'r32_quant8', 'ng_changed_inf', 4),
                                             (3, 'r48_sig5_noise', 'ng_all_inf', 6),
                                             # narrow halos: nearly every retrace that moves travels as a walker, for several hops
                                             (4, 'r32_quant8', 'ng_all_inf', 2), (8, 'r32_quant8', 'ng_changed_inf', 3),
                                             (6, 'r48_sig5_noise', 'ng_changed_inf', 3),
                                             # noisy vacuum (thousands of maxima, -1 labels) with a narrow halo
                                             (4, 'r40_vac_noise', 'ng_changed_2', 3), (5, 'r40_vac_noise', 'ng_all_inf', 2)])
def test_rough_densities_slabs_equal_the_pipeline(n, name, tag, halo):
    """Noisy / rounded / plateau densities: with tie voxels (5-digit rounding) the refinement really relabels voxels
    after a neargrid assignment; without them it must change nothing, region stop or not.
    r64: slabs of whole bricks (brick masks + shared maxima, records for the window); r32 with 2 / 4
    slabs the same with tie voxels and thousands of relabelled voxels; r40 / r48 with 3 slabs: slab boundaries inside
    bricks (the full-record window table)."""
    from rough_common import MODES, load_rough, pipeline_maps, refined, vac_tol
    g, rho = load_rough(name)
    if tag not in g.files:
        pytest.skip('mode not recorded for this case')
    maps = pipeline_maps(g, rho)
    want, olog = refined(g, rho, maps, tag)
    if name in ('r48_sig5_noise', 'r32_quant8'):   # (without tie voxels the own-trajectory map is a fixed point of the retraces)
        assert sum(c for _, c in olog) > 0, 'the rounded cases are meant to change labels during the refinement'
    mode, iters = MODES[tag]
    pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, rho, 'neargrid', mode, iters, halo, vac_tol(g))
    assert np.array_equal(maxima, maps['maxima'])
    assert np.array_equal(pre, maps['assign'].astype(np.int32))
    assert [tuple(x) for x in log] == [tuple(x) for x in olog]
    assert np.array_equal(post, want)


def test_slab_contexts_reused_across_assignments():
    """The same N contexts run neargrid, ongrid and neargrid again (a pipeline that keeps its contexts): every piece of
    state a step leaves behind -- table window, region labels, brick uniformity, which label planes are known to be
    zero -- must be rebuilt or invalidated by the next one."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    n = 4
    sh = Shared(n)
    out = [None] * n

    def work(rank):
        try:
            ctx = _lib.Context(0)
            runner = slab.SlabRunner(slab.GpuBackend(ctx, 0), ThreadComm(sh, rank), rho.shape, g['dist_mat'], g['T_grad'], halo=8)
            runner.enable_table_window(8)
            ctx.upload_density(rho)
            x0, x1 = runner.x_range
            got = []
            for method in ('neargrid', 'ongrid', 'neargrid', 'neargrid'):
                ctx.vacuum_assign(None, 1.0)
                runner.assign(method)
                pre = ctx.download_labels(np.int32)[x0:x1].copy()
                log = runner.refine('changed', 2)
                got.append((pre, ctx.download_labels(np.int32)[x0:x1].copy(), log))
            out[rank] = (x0, got)
            ctx.close()
        except Exception as e:  # noqa: BLE001
            sh.errors.append(repr(e))
            sh.barrier.abort()

    ts = [threading.Thread(target=work, args=(r,)) for r in range(n)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not sh.errors, sh.errors
    out.sort(key=lambda r: r[0])
    for k, method in enumerate(('neargrid', 'ongrid', 'neargrid', 'neargrid')):
        pre = np.concatenate([r[1][k][0] for r in out])
        post = np.concatenate([r[1][k][1] for r in out])
        if method == 'neargrid':
            assert np.array_equal(pre, g['ng_F'].astype(np.int32)), k
            assert np.array_equal(post, g['ng_changed_2'].astype(np.int32)), k
        else:
            assert np.array_equal(pre, g['og_main'].astype(np.int32)), k
            assert np.array_equal(post, g['og_ngrefine_changed_2'].astype(np.int32)), k
            assert np.array_equal(np.array(out[0][1][k][2], np.int64).reshape(-1, 2), g['og_ngrefine_changed_2_log']), k


def test_windowed_table_is_used_and_exact():
    """8 slabs of 8 planes on a 64^3 grid with a 8-plane table margin: every rank builds 24 of 64 planes of
    the table; walkers that leave the window fall back to the exact slow kernel."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(8, g, rho, 'neargrid', 'changed', 2, 2, None)
    assert all(run_slabs.last_windowed)
    assert np.array_equal(pre, g['ng_F'].astype(np.int32)) and np.array_equal(post, g['ng_changed_2'].astype(np.int32))
    pre2, post2, *_ = run_slabs(8, g, rho, 'neargrid', 'changed', 2, 2, None, window=False)
    assert not any(run_slabs.last_windowed) and np.array_equal(pre, pre2) and np.array_equal(post, post2)


def test_rccl_transport_through_the_c_abi_single_rank():
    """xb_comm_* with a one-rank communicator: librccl is dlopen'ed, every entry point is exercised (the collectives
    are identities, the brick-mask broadcast has itself as root).  More ranks need more GPUs: RCCL refuses two ranks
    on one device, which bench.py --gpus 2 on this box answers with its host-staged transport (next test)."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    ctx = _lib.Context(0)
    ctx.set_grid(rho.shape, g['dist_mat'], g['T_grad'])
    ctx.upload_density(rho)
    ctx.comm_init(0, 1, ctx.comm_unique_id())
    assert ctx.comm_allreduce([5, -3, 1 << 40]) == [5, -3, 1 << 40]
    info = ctx.comm_info()         # what the communicator says about itself (bench.py puts it into the multi-GPU line)
    assert info['nccl_comm_count'] == 1 and info['nccl_user_rank'] == 0 and info['nccl_device'] == 0 and info['rccl_version'] > 20000, info
    assert ctx.comm_allreduce([7], 'max') == [7] and ctx.comm_allreduce([7], 'min') == [7]
    assert ctx.comm_allgather([4, 9, 2]).tolist() == [4, 9, 2]
    ctx.comm_exchange_planes(0, [], [])
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('neargrid')
    before = ctx.download_labels(np.int32)
    nbr = rho.size // 512
    ctx.comm_share_brick_masks([0], [nbr])
    ctx.comm_exchange_planes(1, [], [])
    assert n == 8 and np.array_equal(ctx.download_labels(np.int32), before)
    with pytest.raises(_lib.BaderHipError):
        ctx.comm_exchange_planes(0, [(0, 0, 1)], [])       # a send to myself is refused
    # the narrowed halo (round 3): 8 basins -> label planes travel as int8, packed before the group and widened behind it.
    # One GPU can run that very code with itself as the peer (XB_OPT_SELF_EXCHANGE): planes [3, 7) -> [40, 44), a second run
    # [60, 62) -> [10, 12) in the same group, then the same with int32 on the wire (XB_CHECK_WIDE_HALO)
    nyz = rho.shape[1] * rho.shape[2]
    ctx.set_option(_lib.XB_OPT_SELF_EXCHANGE, 1)
    for narrow, width in ((1, 1), (0, 4)):
        ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0 if narrow else _lib.XB_CHECK_WIDE_HALO)   # int32 label halos
        ctx.upload_labels(before.astype(np.int8))   # (the wire width follows the uploaded dtype: bader_calc hands refine its int8 map)
        sent0 = ctx.comm_bytes_sent()
        ctx.comm_exchange_planes(0, [(0, 3, 7), (0, 60, 62)], [(0, 40, 44), (0, 10, 12)])
        want = before.copy()
        want[40:44], want[10:12] = before[3:7], before[60:62]
        assert np.array_equal(ctx.download_labels(np.int32), want)
        assert ctx.comm_bytes_sent() - sent0 == 6 * nyz * width
    # the wire width follows whoever wrote the labels last, not the last assignment's basin count -- a map with
    # more basins than the 8-basin assignment above, uploaded for a standalone refine, must cross the halo untruncated
    ctx.set_option(_lib.XB_OPT_CROSS_CHECK, 0)
    many = (before.astype(np.int64) * 37 + (np.arange(before.size).reshape(before.shape) % 29)).astype(np.int32)   # labels 0..287
    assert many.max() > 127
    for up, width in ((many.astype(np.int16), 2), (many, 4)):
        ctx.upload_labels(up)
        sent0 = ctx.comm_bytes_sent()
        ctx.comm_exchange_planes(0, [(0, 3, 7), (0, 60, 62)], [(0, 40, 44), (0, 10, 12)])
        want = many.copy()
        want[40:44], want[10:12] = many[3:7], many[60:62]
        assert np.array_equal(ctx.download_labels(np.int32), want)
        assert ctx.comm_bytes_sent() - sent0 == 6 * nyz * width
    ctx.set_option(_lib.XB_OPT_SELF_EXCHANGE, 0)
    # RcclComm.gather_rows through the device collectives (one rank: what comes back is what went in): the single
    # collective for short contributions, the second one for long ones
    from pybader_amd import comm as pcomm
    rc = pcomm.RcclComm.__new__(pcomm.RcclComm)
    rc.ctx, rc.size, rc.rank, rc.device = ctx, 1, 0, True
    for nrows in (0, 1, pcomm.RcclComm.FAST_ROWS, pcomm.RcclComm.FAST_ROWS + 1, 1000):
        rows = np.arange(nrows * 10, dtype=np.int64).reshape(nrows, 10) - 7
        assert np.array_equal(rc.gather_rows(rows), rows)
    ctx.close()


def test_label_wire_stays_a_collective_value_across_per_rank_writes():
    """xb_scatter_voxels / xb_copy_planes are per-rank events (only the ranks with parked retraces scatter), so
    they must not change the width a label halo travels in unless a label they write does not fit it -- otherwise an int32
    send meets an int8 receive.  xb_label_wire reads the width and lets a scheduler raise it to the ranks' maximum."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    ctxs = [_lib.Context(0) for _ in range(2)]
    for ctx in ctxs:
        ctx.set_grid(rho.shape, g['dist_mat'], g['T_grad'])
        ctx.upload_density(rho)
        ctx.vacuum_assign(None, 1.0)
        assert ctx.assign('neargrid') == 8
    a, b = ctxs
    assert a.label_wire() == 1 and b.label_wire() == 1           # 8 basins: dtype_calc(-8) = int8
    idx = np.array([5, 77, 4099], np.int64)
    lab, kn = a.gather_voxels(idx)
    a.scatter_voxels(idx, lab, kn)                               # one rank scatters labels already on the grid ...
    assert a.label_wire() == b.label_wire() == 1                 # ... and the ranks still agree
    planes = a.download_labels(np.int32)[3:5].copy()
    a.copy_planes(0, True, planes, 3, 5)                         # planes of a peer that ran the same assignment
    assert a.label_wire() == 1
    a.scatter_voxels(idx, np.array([300, 1, 2], np.int32), kn)   # a label int8 does not hold: widened (never truncated)
    assert a.label_wire() == 2 and b.label_wire() == 1
    assert b.label_wire(max(a.label_wire(), b.label_wire())) == 2   # what SlabRunner._agree_label_wire does
    planes[0, 0, 0] = 1 << 20
    b.copy_planes(0, True, planes, 3, 5)
    assert b.label_wire() == 4
    with pytest.raises(_lib.BaderHipError):
        a.label_wire(3)
    for ctx in ctxs:
        ctx.close()


def test_bench_two_ranks_on_one_gpu(tmp_path):
    """`python bench.py --gpus 2` as typed: the script spawns its ranks, they rendezvous over the file/TCP store,
    RCCL refuses two ranks on one device, every rank falls back to the host-staged transport, rank 0 prints ONE
    JSON line whose map statistics equal the one-rank run's."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for n in (1, 2):
        p = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', str(n), '--size', '128', '--steps', '2',
                            '--warmup', '1', '--full', '--no-cpu'], capture_output=True, timeout=600)
        assert p.returncode == 0, p.stderr.decode()[-2000:]
        lines = [l for l in p.stdout.decode().splitlines() if l.strip()]
        assert len(lines) == 1 and lines[0].startswith('{'), lines[:3]   # ONE JSON line on stdout (librccl's greeting goes to stderr)
        outs.append(json.loads(lines[0]))
    one, two = outs
    assert two['n_gpus'] == 2 and 'host-staged-tcp' in two['config']['parallelism']
    assert two['config']['basins'] == one['config']['basins'] == 8
    assert two['config']['refine_log'] == one['config']['refine_log']


@pytest.mark.parametrize('n,name,halo,iters', [(2, 'c64_cubic', 8, 2), (3, 'c40x48x56_tric', 6, 3), (4, 'c40x48x56_tric', 8, -1),
                                               (4, 'c64_cubic', 4, 2)])
def test_ongrid_plus_refine_changed_slabs(n, name, halo, iters):
    """'changed' refinement with relabelled voxels across slabs: edge_check's global greedy scan resolved on every
    rank from the all-gathered list (xb_edge_check_local / _global); logs and maps equal the one-GPU / oracle ones."""
    import oracle
    g = load_golden(name)
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, rho, 'ongrid', 'changed', iters, halo, tol_of(g))
    assert np.array_equal(pre, g['og_main'].astype(np.int32))
    v = g['og_main'].astype(np.int32)
    olog = []
    oracle.refine('neargrid', ('changed', iters), rho, v, g['dist_mat'], g['T_grad'], 1, log=olog)
    assert any(c > 0 for _, c in olog[:1]), 'the case is meant to relabel voxels'
    assert log == [tuple(x) for x in olog]
    assert np.array_equal(post, v)
    if iters == 2:
        assert np.array_equal(post, g['og_ngrefine_changed_2'].astype(np.int32))


def test_a_slab_rank_holds_slab_sized_table_and_scratch():
    """VERDICT r2 missing #2 / next #4: the reference's blocks are copies of the block extent (thread_handlers.py:31-47); a rank
    here keeps the density (replicated by design), labels, flags and the numbering array full size (17 B/voxel + 1 for the
    brick flags) but its gradient-field table (32 B/voxel of the table window) and its two scratch arrays (12 B/voxel) are
    sized by slab + halo: 256^3 on 8 slabs of 32 planes -- same map as one context, a fraction of its bytes per rank."""
    import hashlib
    shape = (256,) * 3
    vl = np.divide(synth.CUBIC6, shape)
    g = {'dist_mat': distance_matrix(vl), 'T_grad': gradient_transform(vl)}
    ctx = _lib.Context(0)
    ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx.vacuum_assign(None, 1.0)
    n = ctx.assign('neargrid')
    log = ctx.refine('changed', 2)
    want = hashlib.sha256(ctx.download_labels(np.int8)).hexdigest()
    one_total, one_table, one_scratch = ctx.memory_stats()
    ctx.close()
    nvox = float(np.prod(shape))
    assert one_table == 32 * nvox and one_scratch == 12 * nvox
    pre, post, slog, mx, ch, vo, fb = run_slabs(8, g, None, 'neargrid', 'changed', 2, 4, None, shape=shape,
                                                synth_args=(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND), label_dtype=np.int8,
                                                keep_pre=False, margin=8)
    assert all(run_slabs.last_windowed)
    assert hashlib.sha256(np.ascontiguousarray(post)).hexdigest() == want and mx.shape[0] == n
    assert [tuple(x) for x in slog] == [tuple(x) for x in log]
    for total, table, scratch in run_slabs.last_memory:
        assert table == 32 * (32 + 2 * 8) * 256 * 256          # the window: slab + 8 planes each side
        assert scratch <= 12 * (32 + 2 * 32) * 256 * 256 + (80 << 20)
        assert total < 0.55 * one_total, (total, one_total)     # (18 of 62 B/voxel stay full size; 0.45 at 1024^3 on 8 slabs)


@pytest.mark.parametrize('n,size,halo,mode,iters', [(4, 128, 8, 'changed', 2), (8, 256, 16, 'all', 2), (2, 128, 6, 'changed', 2)])
def test_device_driven_step_waits_once_per_assignment_and_once_per_pass(n, size, halo, mode, iters):
    """The slab step with its control flow on the device (csrc/slab_step.h): same map as one context, ONE wait of the host
    for the card per assignment and one per refinement pass (the host-driven calls made about fifteen) -- counted inside
    the library (xb_host_waits), per rank."""
    shape = (size,) * 3
    vl = np.divide(synth.CUBIC6, shape)
    g = {'dist_mat': distance_matrix(vl), 'T_grad': gradient_transform(vl)}
    args = (synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    ctx = _lib.Context(0)
    ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
    ctx.synth_density(*args)
    ctx.vacuum_assign(None, 1.0)
    nb = ctx.assign('neargrid')
    ref_log = ctx.refine(mode, iters)
    want = ctx.download_labels(np.int32)
    ctx.close()
    pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, None, 'neargrid', mode, iters, halo, None, shape=shape, synth_args=args,
                                                   keep_pre=False, margin=None)
    assert np.array_equal(post, want) and log == ref_log and len(maxima) == nb
    assert run_slabs.last_device_steps == [1] * n
    passes = len(log) if mode == 'all' else 1
    for a, r in run_slabs.last_host_waits:
        # (a pass whose walkers outlast the blind rounds hands the rest to the host-driven loop: more waits, same result)
        assert a == 1 and (r == passes or fb), run_slabs.last_host_waits


def test_device_driven_step_issues_its_rccl_collectives():
    """The step's block collectives through xb_comm_allgather_block / xb_comm_allreduce_block (csrc/slab_step.h) with real
    blocks, in the order of a node run: each of the two contexts owns a one-rank RCCL communicator (two ranks of ONE
    communicator need two cards), so every collective is an identity and the test transport moves the peers' parts
    afterwards.  The map must come out as always."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(2, g, rho, 'neargrid', 'all', 2, 8, None, comm_cls=ShadowRcclComm)
    assert run_slabs.last_device_steps == [1, 1]
    assert np.array_equal(pre, g['ng_F'].astype(np.int32)) and np.array_equal(post, g['ng_all_2'].astype(np.int32))


def test_device_driven_step_repeats_when_the_growth_outlasts_its_schedule():
    """Status 1 of xb_slab_assign_finish: the kill launches scheduled after the chase (forced to ONE here) did not reach the
    fixpoint -- every rank sees the same verdict (the growth is replicated), nothing downstream ran, the step is repeated
    from pass A with the worst-case schedule.  Same map as always, one repeat per rank, two waits for the assignment."""
    g = load_golden('c64_cubic')
    rho = case_density(g)
    pre, post, log, maxima, ch, vo, fb = run_slabs(4, g, rho, 'neargrid', 'changed', 2, 8, None, options=((_lib.XB_OPT_KILL_LAUNCHES, 1),))
    assert run_slabs.last_device_steps == [1] * 4 and all(r == 1 for r, _ in run_slabs.last_growth)
    assert [a for a, _ in run_slabs.last_host_waits] == [2] * 4
    assert np.array_equal(pre, g['ng_F'].astype(np.int32)) and np.array_equal(post, g['ng_changed_2'].astype(np.int32))


def test_device_driven_step_hands_a_density_with_thousands_of_maxima_to_the_host_driven_calls():
    """Status 2 of xb_slab_assign_finish: a rank's maxima table does not fit the exchange block (1024 rows) -- every rank sees
    it in the gathered tables, declines the numbering, and the scheduler repeats the assignment with the host-driven calls
    (and stays with them for this density).  The map equals the one-context map."""
    shape = (96, 96, 96)
    vl = np.divide(synth.CUBIC6, shape)
    g = {'dist_mat': distance_matrix(vl), 'T_grad': gradient_transform(vl)}
    ctx = _lib.Context(0)
    ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
    ctx.synth_density(synth.CUBIC6, synth.ATOMS8, synth.BACKGROUND)
    rho = np.ascontiguousarray(ctx.download_density() + 3e-2 * np.random.default_rng(11).random(shape))
    ctx.upload_density(rho)
    ctx.vacuum_assign(None, 1.0)
    nb = ctx.assign('neargrid')
    ref_log = ctx.refine('changed', 2)
    want = ctx.download_labels(np.int32)
    ctx.close()
    assert nb > 2048
    pre, post, log, maxima, ch, vo, fb = run_slabs(2, g, rho, 'neargrid', 'changed', 2, 8, None, keep_pre=False)
    assert run_slabs.last_declined == [True, True] and run_slabs.last_device_steps == [0, 0]
    assert np.array_equal(post, want) and log == ref_log and len(maxima) == nb


@pytest.mark.parametrize('seed', [7, 11, 23])
def test_random_decompositions_equal_one_context(seed):
    """A seeded spread of decompositions -- 2 / 4 / 8 slabs, three lattices, halos 3-16, table margins 8-32 and the default,
    every refinement mode, smooth densities and densities with noise far below the basin depths -- through the scheduler
    (the device-driven step wherever it applies, the host-driven calls where it declines) against one context: same map,
    same refinement log, same number of basins."""
    hexa = np.array([[6.0, 0.0, 0.0], [-3.0, 5.196152422706632, 0.0], [0.0, 0.0, 7.0]])
    rng = np.random.default_rng(seed)
    stepped = 0
    for _ in range(6):
        n = int(rng.choice([2, 4, 8]))
        shape = (max(int(rng.choice([64, 128, 192])), 16 * n), int(rng.choice([64, 80, 96])), int(rng.choice([64, 96, 128])))
        lat = [synth.CUBIC6, synth.TRICLINIC, hexa][int(rng.integers(3))]
        noise = float(rng.choice([0.0, 1e-7, 1e-6, 3e-6]))
        halo = int(rng.choice([3, 4, 6, 8, 16]))
        margin = rng.choice([None, 8, 16, 32])
        mode, iters = [('changed', 2), ('all', 2), ('changed', -1), ('all', -1)][int(rng.integers(4))]
        vl = np.divide(lat, shape)
        g = {'dist_mat': distance_matrix(vl), 'T_grad': gradient_transform(vl)}
        ctx = _lib.Context(0)
        ctx.set_grid(shape, g['dist_mat'], g['T_grad'])
        ctx.synth_density(lat, synth.ATOMS8, synth.BACKGROUND)
        rho = ctx.download_density()
        if noise:
            rho = np.ascontiguousarray(rho + noise * np.random.default_rng(1).random(shape))
            ctx.upload_density(rho)
        ctx.vacuum_assign(None, 1.0)
        nb = ctx.assign('neargrid')
        ref_log = ctx.refine(mode, iters)
        want = ctx.download_labels(np.int32)
        ctx.close()
        pre, post, log, maxima, ch, vo, fb = run_slabs(n, g, rho, 'neargrid', mode, iters, halo, None, keep_pre=False,
                                                       margin=None if margin is None else int(margin))
        assert np.array_equal(post, want) and log == ref_log and len(maxima) == nb, (n, shape, noise, halo, margin, mode, iters)
        stepped += run_slabs.last_device_steps[0]
    assert stepped >= 2     # (the device-driven step took its share of the cases)
