"""The analyses' device blocks (pybader_amd/csrc/ctx_buffers.h), compiled alone for the host with g++ and a fake allocator that
counts its calls and its live allocations and can fail the k-th allocation: what reserve, release, release_all,
release_on_shape_change and counted_bytes do to the blocks, and the table of which block a change of shape releases and which
xb_memory_stats counts, spelled out here by name."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'pybader_amd', 'csrc', 'ctx_buffers.h')

BLOCKS = ['w_A', 'w_V', 'w_S', 'w_pending', 'w_list0', 'w_list1', 'w_state', 'm_buf', 'aj_buf', 'mg_buf', 'vo_buf', 'cp_list', 'cp_lut',
          'st_buf', 'nci_buf', 'hs_buf', 'iso_vert', 'iso_col', 'iso_tri', 'iso_cell', 'iso_wrap', 'rg_map', 'rg_seed']
# adjacency, merge, critical (list and table), isosurface, regions; weight, moments, Voronoi, stencil, NCI and Hirshfeld's block stay
ON_SHAPE_CHANGE = {'aj_buf', 'mg_buf', 'cp_list', 'cp_lut', 'iso_vert', 'iso_col', 'iso_tri', 'iso_cell', 'iso_wrap', 'rg_map', 'rg_seed'}
UNCOUNTED = {'w_state'}

SHIM = '#include "ctx_buffers.h"\n' + r'''
#include <cstdlib>
static int live, allocs, frees, waits, fail_at;
struct Fake {
    int wait() { waits++; return 0; }
    int alloc(void **p, buf_size n) {
        if (++allocs == fail_at) return -7;
        *p = std::malloc(n ? n : 1);
        live++;
        return 0;
    }
    void free(void *p) { std::free(p); frees++; live--; }
};
static CtxBuffers B;
extern "C" int n_blocks(void) { return BLK_COUNT; }
extern "C" const char *row(int b, int *shape, int *counted) { *shape = CTX_BLOCKS[b].shape; *counted = CTX_BLOCKS[b].counted; return CTX_BLOCKS[b].name; }
extern "C" void fresh(int fail) { buf_release_all(B, Fake{}); live = allocs = frees = waits = 0; fail_at = fail; }
extern "C" void fail_in(int k) { fail_at = k ? allocs + k : 0; }
extern "C" void calls(int *out) { out[0] = live; out[1] = allocs; out[2] = frees; out[3] = waits; }
extern "C" void blocks(void **p, long long *bytes) { for (int b = 0; b < BLK_COUNT; b++) { p[b] = B.blk[b].p; bytes[b] = (long long)B.blk[b].bytes; } }
extern "C" int reserve(int b, long long bytes, long long slack) { return buf_reserve(B, Fake{}, {{b, (buf_size)bytes, (buf_size)slack}}); }
extern "C" int reserve3(const int *b, const long long *bytes) {
    return buf_reserve(B, Fake{}, {{b[0], (buf_size)bytes[0], 0}, {b[1], (buf_size)bytes[1], 0}, {b[2], (buf_size)bytes[2], 0}});
}
extern "C" void release(int first, int last) { buf_release(B, Fake{}, first, last); }
extern "C" void release_all(void) { buf_release_all(B, Fake{}); }
extern "C" void release_on_shape_change(void) { buf_release_on_shape_change(B, Fake{}); }
extern "C" long long counted_bytes(void) { return (long long)buf_counted_bytes(B); }
'''


class Lib:
    def __init__(self, so):
        self.lib = lib = C.CDLL(so)
        lib.row.restype = C.c_char_p
        lib.counted_bytes.restype = C.c_longlong
        lib.reserve.argtypes = [C.c_int, C.c_longlong, C.c_longlong]
        self.n = lib.n_blocks()

    def calls(self):
        v = (C.c_int * 4)()
        self.lib.calls(v)
        return dict(zip(('live', 'allocs', 'frees', 'waits'), v))

    def blocks(self):
        p, n = (C.c_void_p * self.n)(), (C.c_longlong * self.n)()
        self.lib.blocks(p, n)
        return {BLOCKS[b]: (p[b], n[b]) for b in range(self.n)}

    def reserve(self, name, nbytes, slack=0):
        return self.lib.reserve(BLOCKS.index(name), nbytes, slack)

    def reserve3(self, names, sizes):
        return self.lib.reserve3((C.c_int * 3)(*[BLOCKS.index(x) for x in names]), (C.c_longlong * 3)(*sizes))

    def fill(self):
        """every block holds 100 + its index bytes"""
        for b, name in enumerate(BLOCKS):
            assert self.reserve(name, 100 + b) == 0
        return self.blocks()


@pytest.fixture(scope='module')
def buf(tmp_path_factory):
    gxx = shutil.which('g++') or shutil.which('c++')
    if gxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('ctx_buffers')
    src = d / 'shim.cpp'
    src.write_text(SHIM)
    so = d / 'ctx_buffers.so'
    subprocess.check_call([gxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', os.path.dirname(HEADER), '-o', str(so), str(src)])
    return Lib(str(so))


def test_the_header_is_plain_cxx_and_its_table_is_this_one(buf):
    assert '#include' not in open(HEADER).read()
    assert buf.n == len(BLOCKS)
    for b, name in enumerate(BLOCKS):
        shape, counted = C.c_int(), C.c_int()
        assert buf.lib.row(b, C.byref(shape), C.byref(counted)).decode() == name
        assert (bool(shape.value), bool(counted.value)) == (name in ON_SHAPE_CHANGE, name not in UNCOUNTED), name


def test_reserve_at_or_below_the_held_size_calls_nothing(buf):
    buf.lib.fresh(0)
    assert buf.reserve('m_buf', 4096) == 0
    before, calls = buf.blocks(), buf.calls()
    assert before['m_buf'][0] and before['m_buf'][1] == 4096 and calls == dict(live=1, allocs=1, frees=0, waits=1)
    for want in (4096, 4095, 1, 0):
        assert buf.reserve('m_buf', want) == 0
        assert buf.blocks() == before and buf.calls() == calls, want       # same pointer, same count, no wait


def test_reserve_above_the_held_size_waits_frees_and_allocates_once(buf):
    buf.lib.fresh(0)
    assert buf.reserve('st_buf', 24) == 0 and buf.reserve('st_buf', 25) == 0
    assert buf.calls() == dict(live=1, allocs=2, frees=1, waits=2)
    assert buf.blocks()['st_buf'][1] == 25 and buf.lib.counted_bytes() == 25
    # bytes beyond the counted ones are allocated, not counted, and do not serve a larger request
    assert buf.reserve('w_pending', 10, 6) == 0 and buf.blocks()['w_pending'][1] == 10 and buf.lib.counted_bytes() == 35
    assert buf.reserve('w_pending', 12) == 0 and buf.calls() == dict(live=2, allocs=4, frees=2, waits=4)


def test_a_failing_allocation_leaves_the_block_empty(buf):
    buf.lib.fresh(2)
    assert buf.reserve('hs_buf', 64) == 0
    assert buf.reserve('hs_buf', 128) == -7
    assert buf.blocks()['hs_buf'] == (None, 0) and buf.lib.counted_bytes() == 0 and buf.calls()['live'] == 0
    assert buf.reserve('hs_buf', 128) == 0 and buf.blocks()['hs_buf'][1] == 128


@pytest.mark.parametrize('fail_at', [1, 2, 3])
def test_a_failing_allocation_empties_the_whole_group(buf, fail_at):
    group = ['iso_vert', 'iso_col', 'iso_tri']
    buf.lib.fresh(0)
    assert buf.reserve('nci_buf', 8) == 0                                   # (a bystander)
    bystander, live_before = buf.blocks()['nci_buf'], buf.calls()['live']
    buf.lib.fail_in(fail_at)                                                # the group's k-th allocation fails
    assert buf.reserve3(group, [30, 20, 10]) == -7
    now = buf.blocks()
    assert all(now[g] == (None, 0) for g in group) and now['nci_buf'] == bystander
    assert buf.calls()['live'] == live_before == 1 and buf.lib.counted_bytes() == 8
    buf.lib.fail_in(0)
    assert buf.reserve3(group, [30, 0, 10]) == 0                            # all of it; a block asked for 0 bytes stays empty
    now = buf.blocks()
    assert [now[g][1] for g in group] == [30, 0, 10] and now['iso_col'][0] is None and buf.calls()['live'] == 3
    waits = buf.calls()['waits']
    assert buf.reserve3(group, [30, 0, 11]) == 0 and buf.calls()['waits'] == waits + 1      # one wait for the group, one block regrown
    assert buf.blocks()['iso_vert'] == now['iso_vert'] and buf.blocks()['iso_tri'][1] == 11


def test_release_on_shape_change_empties_exactly_the_named_blocks(buf):
    buf.lib.fresh(0)
    before = buf.fill()
    buf.lib.release_on_shape_change()
    after = buf.blocks()
    for name in BLOCKS:
        assert after[name] == ((None, 0) if name in ON_SHAPE_CHANGE else before[name]), name
    assert buf.calls()['live'] == len(BLOCKS) - len(ON_SHAPE_CHANGE)


def test_release_and_release_all(buf):
    buf.lib.fresh(0)
    before = buf.fill()
    buf.lib.release(BLOCKS.index('cp_list'), BLOCKS.index('cp_lut'))
    after = buf.blocks()
    assert all(after[n] == ((None, 0) if n in ('cp_list', 'cp_lut') else before[n]) for n in BLOCKS)
    buf.lib.release(BLOCKS.index('cp_list'), BLOCKS.index('cp_lut'))        # (an empty block: nothing to free)
    assert buf.calls()['frees'] == 2
    buf.lib.release_all()
    assert buf.calls()['live'] == 0 and buf.lib.counted_bytes() == 0 and set(buf.blocks().values()) == {(None, 0)}


def test_counted_bytes_sums_the_counted_blocks(buf):
    buf.lib.fresh(0)
    buf.fill()
    assert buf.lib.counted_bytes() == sum(100 + b for b, name in enumerate(BLOCKS) if name not in UNCOUNTED)
    assert buf.reserve('w_state', 4000) == 0 and buf.reserve('w_pending', 200, 7) == 0
    assert buf.lib.counted_bytes() == sum(100 + b for b, name in enumerate(BLOCKS) if name not in UNCOUNTED) - (100 + BLOCKS.index('w_pending')) + 200
