// ctx_buffers.h -- the device blocks the analyses keep on a context (xb_ctx inherits CtxBuffers): a pointer and the bytes it counts
// towards xb_memory_stats per block, and the one table that says which blocks a change of the grid's shape releases and which are
// counted.  Plain C++, no include: the memory comes through a policy `Mem` with wait() (the host waits for the context's stream),
// alloc(void **, bytes) (both return 0 or an error code) and free(void *); tests/test_ctx_buffers_cpu.py compiles this file alone
// with a counting fake.
#pragma once
typedef decltype(sizeof 0) buf_size;
enum CtxBlock {
    BLK_W_A, BLK_W_V, BLK_W_S, BLK_W_PENDING, BLK_W_LIST0, BLK_W_LIST1, BLK_W_STATE,   // the weight method (host_weight.h)
    BLK_M, BLK_AJ, BLK_MG, BLK_VO,                      // xb_moment_sum, xb_adjacency, xb_merge_basins, xb_voronoi_assign
    BLK_CP_LIST, BLK_CP_LUT,                            // xb_critical_points: the records, the classification table
    BLK_ST, BLK_NCI, BLK_HS,                            // xb_laplacian_sum, xb_nci_sum / xb_nci_hist, xb_hirshfeld_setup
    BLK_ISO_VERT, BLK_ISO_COL, BLK_ISO_TRI, BLK_ISO_CELL, BLK_ISO_WRAP,   // the mesh of the last xb_isosurface
    BLK_RG_MAP, BLK_RG_SEED,                            // xb_regions_label: the component of every voxel, the components' seeds
    BLK_COUNT
};
// one row per block, in the enum's order.  shape: xb_set_grid releases the block when the grid's shape changes (what it holds was
// made for the old shape; the others are sized by voxel or label counts and refilled by every call).  counted: xb_memory_stats
// counts its bytes (the level loop's few state words never were)
static const struct CtxBlockRow { const char *name; bool shape, counted; } CTX_BLOCKS[BLK_COUNT] = {
    {"w_A", false, true}, {"w_V", false, true}, {"w_S", false, true}, {"w_pending", false, true}, {"w_list0", false, true},
    {"w_list1", false, true}, {"w_state", false, false},
    {"m_buf", false, true}, {"aj_buf", true, true}, {"mg_buf", true, true}, {"vo_buf", false, true},
    {"cp_list", true, true}, {"cp_lut", true, true},
    {"st_buf", false, true}, {"nci_buf", false, true}, {"hs_buf", false, true},
    {"iso_vert", true, true}, {"iso_col", true, true}, {"iso_tri", true, true}, {"iso_cell", true, true}, {"iso_wrap", true, true},
    {"rg_map", true, true}, {"rg_seed", true, true},
};
struct CtxBuffers {
    struct Block { void *p = nullptr; buf_size bytes = 0; } blk[BLK_COUNT];
    template <class T> T *ptr(int b) const { return static_cast<T *>(blk[b].p); }
    buf_size bytes(int b) const { return blk[b].bytes; }
};
// a request: the block, the bytes it must hold (and counts), bytes allocated beyond them that are not counted
struct BufWant { int b; buf_size bytes, slack; };

// frees the blocks first .. last and leaves them empty
template <class Mem> static inline void buf_release(CtxBuffers &B, Mem &&m, int first, int last) {
    for (int b = first; b <= last; b++) {
        if (B.blk[b].p) m.free(B.blk[b].p);
        B.blk[b] = CtxBuffers::Block{};
    }
}
// Grows the blocks of `want` that hold less than asked and never shrinks one: with every block large enough nothing is called, not
// even the wait.  Otherwise one wait, then each block that is too small is freed, allocated and its size recorded.  All or none: when an
// allocation fails every block of the request ends empty and counts 0, and the allocation's code is returned.
template <class Mem, int K> static inline int buf_reserve(CtxBuffers &B, Mem &&m, const BufWant (&want)[K]) {
    bool grow = false;
    for (const BufWant &w : want) grow = grow || B.blk[w.b].bytes < w.bytes;
    if (!grow) return 0;
    int rc = m.wait();
    if (rc) return rc;
    for (int k = 0; k < K && !rc; k++) {
        CtxBuffers::Block &x = B.blk[want[k].b];
        if (x.bytes >= want[k].bytes) continue;
        buf_release(B, m, want[k].b, want[k].b);
        rc = m.alloc(&x.p, want[k].bytes + want[k].slack);
        if (rc) x.p = nullptr;   // (whatever a failed allocation left there)
        else x.bytes = want[k].bytes;
    }
    if (rc)
        for (const BufWant &w : want) buf_release(B, m, w.b, w.b);
    return rc;
}
template <class Mem> static inline void buf_release_all(CtxBuffers &B, Mem &&m) { buf_release(B, m, 0, BLK_COUNT - 1); }
template <class Mem> static inline void buf_release_on_shape_change(CtxBuffers &B, Mem &&m) {
    for (int b = 0; b < BLK_COUNT; b++)
        if (CTX_BLOCKS[b].shape) buf_release(B, m, b, b);
}
static inline buf_size buf_counted_bytes(const CtxBuffers &B) {
    buf_size n = 0;
    for (int b = 0; b < BLK_COUNT; b++)
        if (CTX_BLOCKS[b].counted) n += B.blk[b].bytes;
    return n;
}
