// bader_hip.hip -- libbader_hip.so: HIP kernels + C ABI (include/bader_hip.h) for gfx950.  ONE translation unit:
//   kernels    k_common.h k_masks.h k_fused.h k_trace.h k_ongrid.h k_edges.h k_sums.h k_text.h k_format.h (fmt_core.h) k_interop.h k_weight.h k_cell.h (the cell and tile geometry of the four atom-centred analyses) k_moments.h k_adjacency.h k_merge.h k_voronoi.h k_critical.h k_stencil.h k_nci.h k_dori.h k_hirshfeld.h k_isa.h k_mbis.h k_igm.h k_isosurface.h k_regions.h
//   host side  this file (context struct, options, statistics, timing) + ctx_state.h (the cached-state flags and their invalidation events; plain C++) + ctx_buffers.h (the device blocks the analyses keep, their table and their accounting; plain C++) + host_context.h (life cycle, transfers)
//              + host_assign.h (the table outside an assignment, the assignments) + host_refine.h + host_sums.h + host_slab_table.h (host-driven slab calls) + host_interop.h (device arrays in and out) + host_weight.h (the weight method) + host_cell.h (the host side of k_cell.h) + host_moments.h (moments per label) + host_adjacency.h (surfaces between labels) + host_merge.h (merging volumes by persistence) + host_voronoi.h (the nearest-atom partition) + host_critical.h (critical points and the bond graph) + host_stencil.h (the Laplacian and the Hessian of the density) + host_nci.h (the NCI index: reduced gradient, sign(lambda2) rho, region sums, histogram) + host_dori.h (DORI: the density overlap regions indicator, region sums) + host_hirshfeld.h (Hirshfeld charges, the promolecular and the deformation density) + host_isa.h host_mbis.h (iterative stockholder atoms on the Hirshfeld setup) + host_igm.h (IGM: the independent gradient model on the table setup, region sums) + host_isosurface.h (isosurfaces by marching tetrahedra) + host_regions.h (connected components of a mask: level-set islands, pockets, NCI domains) + host_analyses.h (what the analyses forget with the grid or its shape, their release calls) + comm.h (RCCL through the ABI)
//              + slab_step.h (the slab step with its control flow on the device)
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -shared (see pybader_amd/build.py).
#include "bader_kernels.h"
#include "../../include/bader_hip.h"
#include "ctx_state.h"
#include "ctx_buffers.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <locale.h>   // newlocale, strtod_l: the text reader's host conversions do not depend on LC_NUMERIC
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

// every wait of the host for the card made inside the library is counted (per calling thread: xb_host_waits)
static thread_local long long xb_waits = 0;
static inline hipError_t xb_counted_sync(hipStream_t s) { xb_waits++; return (hipStreamSynchronize)(s); }
#define hipStreamSynchronize(s) xb_counted_sync(s)

// =============================================================================================
// kernels
// =============================================================================================
#include "k_common.h"
#include "k_masks.h"
#include "k_fused.h"
#include "k_trace.h"
#include "k_ongrid.h"
#include "k_edges.h"
#include "k_sums.h"
#include "k_text.h"
#include "k_format.h"
#include "k_interop.h"
#include "k_weight.h"
#include "k_cell.h"
#include "k_moments.h"
#include "k_adjacency.h"
#include "k_merge.h"
#include "k_voronoi.h"
#include "k_critical.h"
#include "k_stencil.h"
#include "k_nci.h"
#include "k_dori.h"
#include "k_hirshfeld.h"
#include "k_isa.h"
#include "k_mbis.h"
#include "k_igm.h"
#include "k_stockmom.h"
#include "k_isosurface.h"
#include "k_regions.h"

// =============================================================================================
// host side
// =============================================================================================
static thread_local std::string g_err;
static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}
#define XB_BIG_CHUNK ((size_t)16 << 20)
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess) return fail(XB_E_HIP, "%s:%d %s: %s", __FILE__, __LINE__, #x, hipGetErrorString(e_)); \
    } while (0)

struct TimedKernel {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> pending;
    double ms = 0.;
    long long launches = 0;
};

namespace xbcomm { struct State; }
struct xb_ctx : CtxState, CtxBuffers {   // (ctx_state.h: the flags of the cached state and the events that drop them; ctx_buffers.h: the analyses' device blocks)
    int device = 0;
    xbcomm::State *comm = nullptr;   // RCCL transport (comm.h), one process per GPU
    struct FmtState *fmt = nullptr;  // density -> text writer between xb_format_begin and xb_format_end (host_format.h)
    hipStream_t stream = nullptr;
    Grid g{};
    bool has_grid = false;
    long long N = 0;
    int halo = 0;
    double *rho = nullptr;
    GradRec *grad = nullptr;   // gradient-field table, 32 B per voxel of the table window (the whole grid on one GPU)
    long long grad_cap = 0;    // records allocated
    long long list_cap = 0;    // ints allocated for `list` (N on one GPU; the slab's planes + scratch on a slab)
    int *ec_buf = nullptr;     // edge_check's two seed / overflow lists when `stage` is too small for them (slabs)
    long long ec_buf_cap = 0;
    double *dist_dev = nullptr; // dist_mat on the device
    int *boxbuf = nullptr;      // seeds / box tables of the table build (BB_* layout)
    int *box_max_tab = nullptr; // region id - 1 -> voxel of the region's maximum (inside boxbuf: BB_BOXMAX or BB_REGMAX)
    int n_boxes = 0;
    long long box_voxels = 0;
    // what xb_set_option keeps (XB_OPT_* in bader_hip.h).  Not here: XB_OPT_KILL_LAUNCHES, which the library raises itself
    // (grow_kill_launches), and XB_OPT_DROP_TABLE, an action on grad_valid / brick_max_valid that keeps no value
    struct Options {
        int boxes = 1, bricks = 1; // XB_OPT_REGIONS: its bits XB_REGIONS_BOXES and XB_REGIONS_BRICKS; trapping regions are built only with both
        // XB_OPT_CROSS_CHECK, a field per XB_CHECK_* bit: 1 (the implementation in use) unless the bit is set
        int mirror = 1;            // pass A: mirror prefilter of the ongrid face test (k_masks.h, bm_mirror)
        int lean = 1;              // persistent trace: the lean walker (k_trace.h, ng_walk_lean); 0: ng_walk_wave (tests compare)
        int mask_diag = 1;         // pass A: the three-product form of T_grad . grad on orthogonal lattices (tests compare)
        int tile_dilate = 1;       // the dilation of the edge sweep tile by tile (k_edge_dilate_tiles) instead of from the edge list (tests compare)
        int narrow_halo = 1;       // label halos travel as dtype_calc(-n_maxima) (int8 / int16) instead of int32 (comm.h)
        int ec_share = 1;          // k_ec_chase: a long queue sheds its surplus into other workgroups' mailboxes (0: every workgroup keeps what it wakes; A/B, XB_CHECK_NO_EC_SHARE)
        int nb_bits = 1;           // lean walker / lean retrace: "no records there" from the neighbour bits of the record in hand (0: the brick label / brick byte per step; tests compare, XB_CHECK_BRICK_LOOKUP)
        int bit_sweep = 1;         // edge sweep of the listed tiles: row bit masks with the dilation fused in (k_edge_sweep_bits); 0: k_edge_flag_listed + k_edge_dilate_tiles (tests compare, XB_CHECK_VOXEL_SWEEP)
        int lean_retrace = 1;      // refinement on one GPU: k_refine_trace_lean where its case holds (host_stages.h, lean_retrace_ok); 0: the generic k_refine_trace there too (tests compare, XB_CHECK_GENERIC_RETRACE)
        int io_tiled = 1;          // xb_import_density: permuted layouts through the LDS tile (0: the plain strided gather; tests and the benchmark compare)
        int dbg = 0;               // XB_OPT_DEBUG: XB_DBG_* bits
        int ec_groups = 256;       // XB_OPT_EC_GROUPS: workgroups of k_ec_chase (at most one per CU)
        int ec_qcap = EC_Q;        // XB_OPT_EC_QCAP: LDS queue entries used per buffer (smaller only in tests)
        int self_exchange = 0;     // XB_OPT_SELF_EXCHANGE, tests only: xb_comm_exchange_planes accepts this rank as its own peer (one GPU exercises pack / send / recv / unpack)
        int async_comm = 0;        // XB_OPT_ASYNC_COMM: collectives return without waiting (they are ordered on the context's stream); the device-driven slab step sets it
        bool weight_no_labels = false;   // XB_OPT_WEIGHT_NO_LABELS: the next xb_weight_sum treats no voxel as vacuum and does not read the labels
    } opt;
    int *ec_share = nullptr;    // the sharing block of k_ec_chase (activity count, mailbox tails and slots), allocated on first use
    std::vector<int64_t> esc_starts, esc_offsets, esc_vox;  // xb_escaped_paths -> xb_escaped_paths_fetch
    unsigned long long *ec_pend = nullptr;  // edge_check's counter word per voxel (8 N bytes, allocated on first use)
    int8_t *ec_pflag = nullptr;             // ... and a flag byte per voxel, set on the processed voxels while their boxes are applied (zero otherwise)
    std::vector<int8_t> esc_complete;
    double vac_tol = 0.;       // xb_vacuum_assign's tolerance while vac_by_tol holds
    bool regions_pending = false;  // labels of certain bricks are written by the relabel pass
    bool buni_halo_safe = false;   // buni_valid, and `st` marks every brick outside the owned planes that is not of a trapping region as mixed:
                                   // it stays right when the peers' halo planes arrive (slabs, xb_assign_finish)
    bool regions_neargrid = false; // the regions in `blab` are closed under NEARGRID moves (k_brick_masks); false: the ongrid pointer field's
    int n_walk = 0;                // bricks on the walk list of the last assignment
    int *walk = nullptr;           // ... and where that list lives (inside `list`)
    int table_margin = -1;         // planes of table each side of the slab (slabs); -1: whole grid
    bool table_prebuilt = false;   // xb_table_finish done: the next xb_assign_trace must not rebuild
    int table_stage = 0;           // windowed build: 1 = records + masks done, 2 = trapping regions done
    std::vector<int> window_seeds; // maxima found in the owned planes (windowed build)
    bool window_ties = true;       // the window holds a voxel whose record depends on the tie rule (windowed build)
    bool slab_sparse = false;      // windowed build by passes A / B (k_masks.h): masks for the own bricks, records for the
                                   // uncertain bricks of the window; false: round 1's full record per window voxel
    int ec_local_n = 0;            // xb_edge_check_local -> xb_edge_check_local_fetch
    int walk_n_out = 0;            // walkers exported by the last xb_refine_trace / xb_walkers_continue ...
    void *walk_out_dev = nullptr;  // ... and where they lie (device)
    std::vector<int64_t> walk_host, res_host;   // ... fetched: walkers (10 int64 each), result pairs (voxel | label << 32)
    int walk_n_res = 0;            // (start voxel, label) pairs of the last xb_walkers_continue
    void *walk_in = nullptr, *walk_out2 = nullptr, *walk_res = nullptr;   // xb_walkers_continue: incoming walkers, re-exported ones, results
    long long walk_cap = 0;
    long long stat_deferred = 0;   // retraces redone by the from-rho kernel (sparse table)
    long long stat_bit_sweeps = 0, stat_voxel_sweeps = 0;   // edge sweeps launched by row bit masks / by the per-voxel kernels
    long long stat_ovf_assign = 0, stat_ovf_refine = 0;   // trajectories handed to the exact slow kernel
    long long stat_lean_retraces = 0, stat_generic_retraces = 0;   // first retraces of an edge list launched as k_refine_trace_lean / as the generic kernel (launch_edge_retrace)
    long long stat_nb_traces = 0, stat_lookup_traces = 0, stat_generic_traces = 0;   // group traces launched with ng_walk_packed / ng_walk_lean / ng_walk_wave (launch_persistent_trace)
    long long stat_wide_traces = 0;   // ... those of the two lean walkers that took 64-bit table offsets (more than 2^27 window voxels; the others take 32-bit ones)
    int max_grid[3] = {0, 0, 0};      // hipDeviceProp_t::maxGridSize of the context's device, read once by xb_create (xb_set_grid's per-axis limits)
    std::vector<int> dbg_retrace_ovf;   // XB_DBG_KEEP_RETRACE_OVERFLOW: the voxels those retraces put on the overflow list, until xb_retrace_overflow takes them
    int *bres_last = nullptr;   // the fused neargrid assignment's per-brick trace results (inside `list`), or null
    int *blab = nullptr;        // brick labels of the trapping regions (inside `list`), or null
    int nbk[3] = {0, 0, 0};
    bool brick_max_blanket = false; // brick_rec bit 1 is set on EVERY flagged brick (nothing is known about the maxima), not only where a maximum was found.  Owned by the writers of bit 1: ensure_grad's two tables for given labels set it; pass A (launch_brick_masks: every neargrid assignment, slabs and windowed tables too) and the ongrid masks (k_og_masks, whose flags the late records of refine_iteration_fused keep) clear it
    int grad_cover = 0;        // 0: the table holds a record for every voxel (of the window); 1: only for the bricks flagged in brick_rec
    unsigned char *brick_rec = nullptr;   // per 8^3 brick: its records exist (k_brick_records), nbr bytes inside blab_buf's allocation
    unsigned long long *nb_tab = nullptr; // per 8^3 brick: the neighbour bits of its records by octant (k_nb_table), behind brick_rec
    void *xbuf = nullptr;      // the device-driven slab step's exchange blocks 3-5 (slab_step.h): tie flags, counters, maxima tables
    int slab_rank = 0, slab_nranks = 0, slab_stage = 0;
    void *wbuf[2] = {nullptr, nullptr};   // ... blocks 6 / 7: the walkers of a refinement pass and their results, one part per rank
    void *wk_in = nullptr;                // the walkers this rank carries on in a round (+ their count)
    int wbuf_ranks = 0, walk_last = -1, walk_round = 0, wcap = 0;
    int walk_send = 0;          // walkers of a rank's part that travel in the pass's own gather (0: the capacity; xb_slab_walk_send)
    int grow_kill_launches = 6;   // XB_OPT_KILL_LAUNCHES: kill launches scheduled after a chase (raised to the worst case by the first assignment that needs more)
    long long stat_grow_retries = 0;
    bool defer_wait = false;     // xb_assign_refine: the assignment queues its result transfer and returns without waiting ...
    bool pending_assign = false; // ... and its results are still to be read (after the refinement's first wait)
    int64_t pending_n_maxima = 0;
    int grad_rule = 0;         // which tie rule the resident table obeys: 0 refinement.py:111, 1 methods.py:324, 2 both
                               // (the density has no voxel where they differ)
    int *labels = nullptr;
    int8_t *known = nullptr;
    int *first = nullptr;      // n^3: min voxel per maximum, then rank per maximum
    int *list = nullptr;       // n^3 ints: compaction list (edges / changed voxels)
    int8_t *st = nullptr;      // per-list-entry status for edge_check
    void *stage = nullptr;     // staging for dtype conversion (N * 8 bytes max)
    size_t stage_bytes = 0;
    int *max_list = nullptr;   // maxima discovered (linear indices)
    int *max_aux = nullptr;
    int max_cap = 0;
    int *ovf_list = nullptr;
    int ovf_cap = 0;
    int *counters = nullptr;   // small device scratch: ints
    int *fs = nullptr;         // state block of the device-side control flow (k_fused.h), inside `counters`
    int *blab_buf = nullptr;   // brick labels of the trapping regions (fused path), nbr ints
    long long blab_alloc = 0;
    static constexpr int trace_waves = 8192;   // waves of the persistent trace: 2048 workgroups of XB_TRACE_WAVES = 4, eight per compute unit
    unsigned long long *counters64 = nullptr;
    double *dsum = nullptr;
    int *host_ints = nullptr;  // pinned
    char *big_pin[2] = {nullptr, nullptr};   // two pinned chunks for the large transfers (staged_h2d / staged_d2h)
    hipEvent_t big_ev[2] = {nullptr, nullptr};
    hipEvent_t io_ev = nullptr;   // orders the device-array entry points against the caller's stream (host_interop.h)
    char *pin = nullptr;       // pinned staging for the small host arrays a step uploads (pageable copies pin pages on the fly)
    size_t pin_bytes = 0;
    std::vector<int> maxima_sorted;  // global, label order
    std::vector<int> local_max, local_first;
    bool first_clean = false;
    int list_n = 0;            // entries of `list` that hold the owned known == -2 voxels while list_valid is set
    bool tiles_listed = false; // the last edge_find swept a tile list whose length is in CT_TILES_OWN (xb_edge_list)
    unsigned timing = 0;   // bit k: timer k records its events (xb_enable_timing)
    TimedKernel tk[XB_TIMER_COUNT];
    long long n_alloc = 0;
    bool thin = false;         // an axis has fewer than 3 voxels: transfers, the vacuum sweep and the weight method only (NEED_GRID)
    // the analyses' device buffers are the blocks of ctx_buffers.h (BLK_*); here: what each keeps of its last call on the host
    // the weight method (host_weight.h): the last call's statistics and results
    long long w_stat[6] = {0, 0, 0, 0, 0, 0};
    bool w_have = false;
    std::vector<int64_t> w_idx;
    std::vector<double> w_charge, w_volume;
    // xb_adjacency (host_adjacency.h): the last call's pairs in key order
    bool aj_have = false;
    int aj_dirs = 0;
    std::vector<int32_t> aj_a, aj_b;
    std::vector<int64_t> aj_facets, aj_sfacet;
    std::vector<double> aj_saddle;
    // xb_merge_basins (host_merge.h): the last call's results
    bool mg_have = false;
    std::vector<int32_t> mg_root, mg_round;
    std::vector<double> mg_pers;
    // xb_critical_points / xb_critical_bonds (host_critical.h): cp_n records of the list on the device are in use; the last call's
    // records sorted by voxel, and the last bond graph.  cp_have falls with every writer of the density
    size_t cp_n = 0, cp_bond_voxels = 0;
    bool cb_have = false;
    std::vector<unsigned long long> cp_rec;
    std::vector<int32_t> cb_a, cb_b;
    std::vector<int64_t> cb_saddles, cb_voxel;
    std::vector<double> cb_rho;
    // xb_hirshfeld_setup (host_hirshfeld.h): hs_have: its buffer holds a setup, made on the shape hs_geom records (xb_set_grid drops
    // it with the shape)
    size_t hs_acc = 0;   // (where the results start, in doubles)
    bool hs_have = false;
    int64_t hs_n = 0;
    int hs_cus = 0;   // compute units of the device (sizes the sums' launch)
    HsGeom hs_geom{};
    // xb_isa_setup (host_isa.h): hs_isa: the setup is an ISA one (a Hirshfeld setup with one table per atom, whose buffer also
    // holds what the iteration needs, from the double isa_x on).  isa_cur: which of the two table areas hs_geom.pairs points to
    bool hs_isa = false;
    size_t isa_x = 0, isa_pairs0 = 0;
    int isa_e = 0, isa_cur = 0;
    double isa_bound = 0.;
    // xb_mbis_setup (host_mbis.h): hs_mbis: the setup is an MBIS one (the Hirshfeld setup's geometry with one cutoff per atom, whose
    // buffer also holds the table, the parameters and the bins, from the double mbis_x on).  M: the largest shell count, the row
    // stride of the parameters; MS: the least of 1, 2, 4, 8 that holds it; mbis_e: eN, eS, eV, eR; mbis_cur: the current parameter area
    bool hs_mbis = false;
    size_t mbis_x = 0;
    int mbis_M = 0, mbis_MS = 0, mbis_cur = 0, mbis_e[4] = {0, 0, 0, 0};
    int64_t mbis_J = 0, mbis_KE = 0;
    double mbis_bound = 0., mbis_vv = 0.;
    std::vector<int32_t> mbis_shells;
    // xb_stockholder_moments (host_stockmom.h): what its exponents need of the current setup: the largest cutoff, the largest and the
    // total pair count (sm_cmax < 0: not counted yet -- a plain Hirshfeld setup before its first moments call)
    double sm_rmax = 0.;
    long long sm_cmax = -1, sm_pairs = 0;
    // xb_isosurface (host_isosurface.h): the mesh of the last call on the device has iso_v vertices and iso_t triangles; its two
    // scalars and the per-label volumes.  iso_have falls with every writer of the density
    size_t iso_v = 0, iso_t = 0;
    double iso_area = 0., iso_volume = 0.;
    std::vector<double> iso_vbl;
    // xb_regions_label (host_regions.h): rg_m components with rg_members voxels in them, whether they are the NCI region's and the
    // stencil they were made with; the last xb_regions_shares triplets.  rg_have falls with every writer of the density
    size_t rg_m = 0, rg_members = 0;
    bool rg_sh_have = false, rg_nci = false, rg_timed = false;
    double rg_ms[4] = {0., 0., 0., 0.};   // XB_DOMAINS_TIMES: tile, link, flatten, numbering of the last labelling
    StCoeffs rg_K{};
    std::vector<int32_t> rg_sh_comp, rg_sh_lab;
    std::vector<int64_t> rg_sh_cnt;
};

// utils.dtype_calc(-n) as a byte width (utils.py:25-37): the narrowest signed type for labels 0..n-1 and -1
static inline int label_wire_for(long long n) { return 2 * n <= 255 ? 1 : (2 * n <= 65535 ? 2 : 4); }
// the narrowest signed width that holds each of n labels (host array); *any_negative: one of them is below 0
static inline int labels_fit_wire(const int32_t *lab, long long n, bool *any_negative = nullptr) {
    int32_t lo = 0, hi = 0;
    for (long long i = 0; i < n; i++) { lo = std::min(lo, lab[i]); hi = std::max(hi, lab[i]); }
    if (any_negative) *any_negative = lo < 0;
    return (lo >= -128 && hi <= 127) ? 1 : ((lo >= -32768 && hi <= 32767) ? 2 : 4);
}
static inline unsigned nblocks(long long n) { return (unsigned)((n + TPB - 1) / TPB); }
static GridL light(const Grid &g) {
    GridL l;
    l.nx = g.nx; l.ny = g.ny; l.nz = g.nz; l.nyz = g.nyz;
    l.x0 = g.x0; l.x1 = g.x1; l.vx0 = g.vx0; l.vlen = g.vlen;
    l.wx0 = g.wx0; l.wlen = g.wlen; l.wbase = g.wbase; l.ntot = g.ntot;
    l.use24 = ((long long)g.nx * g.ny < (1 << 24)) && g.nz < (1 << 24);
    l.main_ties = g.main_ties;
    return l;
}

// temporary device memory that is released on every return path
template <typename T>
struct DevBuf {
    T *p = nullptr;
    hipError_t alloc(size_t n) { return hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)); }
    ~DevBuf() { hipFree(p); }
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
};

// the memory behind the analyses' blocks (ctx_buffers.h): the context's stream to wait for, hipMalloc, hipFree
struct HipMem {
    hipStream_t stream;
    int wait() { HIPCHK(hipStreamSynchronize(stream)); return XB_OK; }
    int alloc(void **p, size_t bytes) { HIPCHK(hipMalloc(p, bytes)); return XB_OK; }
    void free(void *p) { hipFree(p); }
};
template <int K> static int reserve(xb_ctx *c, const BufWant (&want)[K]) { return buf_reserve(*c, HipMem{c->stream}, want); }
static int reserve(xb_ctx *c, int b, size_t bytes) { return reserve(c, {{b, bytes, 0}}); }
static void release(xb_ctx *c, int first, int last) { buf_release(*c, HipMem{c->stream}, first, last); }

// the 14-distance form of the grid for the tiled field kernels; false when dist_mat is not symmetric
static bool sym_grid(const Grid &g, GridS &s) {
    s.nx = g.nx; s.ny = g.ny; s.nz = g.nz; s.nyz = g.nyz;
    s.x0 = g.x0; s.x1 = g.x1; s.vx0 = g.vx0; s.vlen = g.vlen; s.wx0 = g.wx0; s.wlen = g.wlen; s.wbase = g.wbase; s.ntot = g.ntot;
    s.main_ties = g.main_ties;
    for (int k = 0; k < 9; k++) s.T[k] = g.T[k];
    auto at = [&](int idx) {
        const int ix = idx / 9, iy = (idx / 3) % 3, iz = idx % 3;
        return g.dist[((ix + 2) % 3) * 9 + ((iy + 2) % 3) * 3 + ((iz + 2) % 3)];
    };
    for (int idx = 0; idx <= 13; idx++) {
        const double a = at(idx), b = at(26 - idx);
        if (std::memcmp(&a, &b, sizeof a) != 0) return false;
        s.dsym[idx] = a;
    }
    return true;
}

// Mirror prefilter of pass A (k_masks.h, bm_mirror): which axes of dist_mat are mirror symmetric (bit j: d(+1 on axis j) ==
// d(-1 on axis j) for all nine pairs -- that lattice vector is orthogonal to the other two) and the margin scale
// 2^-48 (1 + 1/d_min).  dist_mat is indexed 0, +1, -1 (index 2 == -1).
static void mirror_prefilter(const Grid &g, int &mirror, double &mu_scale) {
    mirror = 0;
    double dmin = 0.;
    bool first = true;
    for (int i = 0; i < 27; i++)
        if (i != 0) { dmin = first ? g.dist[i] : std::min(dmin, g.dist[i]); first = false; }
    if (!(dmin > 0.) || !std::isfinite(dmin)) { mu_scale = 0.; return; }
    for (int ax = 0; ax < 3; ax++) {
        bool ok = true;
        for (int u = 0; u < 3 && ok; u++)
            for (int v = 0; v < 3 && ok; v++) {
                int ip[3], im[3];
                ip[ax] = 1; im[ax] = 2;
                ip[(ax + 1) % 3] = im[(ax + 1) % 3] = u;
                ip[(ax + 2) % 3] = im[(ax + 2) % 3] = v;
                const double a = g.dist[ip[0] * 9 + ip[1] * 3 + ip[2]], b = g.dist[im[0] * 9 + im[1] * 3 + im[2]];
                ok = std::memcmp(&a, &b, sizeof a) == 0;
            }
        if (ok) mirror |= 1 << ax;
    }
    mu_scale = std::ldexp(1. + 1. / dmin, -48);
}

struct ScopedTimer {
    xb_ctx *c;
    int which;
    hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(xb_ctx *c_, int w) : c(c_), which(w) {
        if ((c->timing >> which) & 1u) {
            hipEventCreate(&a);
            hipEventCreate(&b);
            hipEventRecord(a, c->stream);
        }
    }
    ~ScopedTimer() {
        if ((c->timing >> which) & 1u) {
            hipEventRecord(b, c->stream);
            c->tk[which].pending.push_back({a, b});
        }
    }
};

extern "C" {

const char *xb_last_error(void) { return g_err.c_str(); }

#include "host_context.h"
#include "host_stages.h"
#include "host_format.h"
#include "host_assign.h"
#include "host_refine.h"
#include "host_sums.h"
#include "host_slab_table.h"
#include "host_interop.h"
#include "host_weight.h"
#include "host_cell.h"
#include "host_moments.h"
#include "host_adjacency.h"
#include "host_merge.h"
#include "host_voronoi.h"
#include "host_critical.h"
#include "host_stencil.h"
#include "host_nci.h"
#include "host_dori.h"
#include "host_hirshfeld.h"
#include "host_isa.h"
#include "host_mbis.h"
#include "host_igm.h"
#include "host_stockmom.h"
#include "host_isosurface.h"
#include "host_regions.h"
#include "host_analyses.h"

int xb_set_option(xb_ctx *c, int key, int value) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    bool ok = true;   // false: the key's value is out of range (reported as the unknown key is)
    switch (key) {
    case XB_OPT_REGIONS: c->opt.boxes = (value & XB_REGIONS_BOXES) != 0; c->opt.bricks = (value & XB_REGIONS_BRICKS) != 0; break;
    case XB_OPT_CROSS_CHECK:
        if (!(ok = value >= 0 && value < 2 * XB_CHECK_GENERIC_RETRACE)) break;
        c->opt.mirror = !(value & XB_CHECK_NO_MIRROR);
        c->opt.lean = !(value & XB_CHECK_GENERIC_WALKER);
        c->opt.mask_diag = !(value & XB_CHECK_FULL_TGRAD);
        c->opt.tile_dilate = !(value & XB_CHECK_LIST_DILATE);
        c->opt.narrow_halo = !(value & XB_CHECK_WIDE_HALO);
        c->opt.ec_share = !(value & XB_CHECK_NO_EC_SHARE);
        c->opt.io_tiled = !(value & XB_CHECK_IO_GATHER);
        c->opt.nb_bits = !(value & XB_CHECK_BRICK_LOOKUP);
        c->opt.bit_sweep = !(value & XB_CHECK_VOXEL_SWEEP);
        c->opt.lean_retrace = !(value & XB_CHECK_GENERIC_RETRACE);
        break;
    case XB_OPT_DEBUG: c->opt.dbg = value; break;
    case XB_OPT_EC_GROUPS: if ((ok = value >= 1 && value <= 4096)) c->opt.ec_groups = value; break;
    case XB_OPT_EC_QCAP: if ((ok = value >= 2 && value <= EC_Q)) c->opt.ec_qcap = value; break;
    case XB_OPT_DROP_TABLE: if (value == XB_DROP_TABLE_AND_MAXIMA) drop_table_and_maxima(*c); else drop_table(*c); break;   // (a refinement rebuilds the table)
    case XB_OPT_KILL_LAUNCHES: if ((ok = value >= 1)) c->grow_kill_launches = value; break;
    case XB_OPT_SELF_EXCHANGE: c->opt.self_exchange = value != 0; break;
    case XB_OPT_ASYNC_COMM: c->opt.async_comm = value != 0; break;
    case XB_OPT_WEIGHT_NO_LABELS: c->opt.weight_no_labels = value != 0; break;
    default: ok = false;
    }
    if (!ok) return fail(XB_E_ARG, "xb_set_option: unknown key %d", key);
    return XB_OK;
}
int xb_growth_stats(xb_ctx *c, int64_t *retries, int64_t *kill_launches) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (retries) *retries = c->stat_grow_retries;
    if (kill_launches) *kill_launches = c->grow_kill_launches;
    return XB_OK;
}
int xb_deferred_stats(xb_ctx *c, int64_t *refine_total) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (refine_total) *refine_total = c->stat_deferred;
    return XB_OK;
}
int xb_sweep_stats(xb_ctx *c, int64_t *bit_sweeps, int64_t *voxel_sweeps) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (bit_sweeps) *bit_sweeps = c->stat_bit_sweeps;
    if (voxel_sweeps) *voxel_sweeps = c->stat_voxel_sweeps;
    return XB_OK;
}
int xb_retrace_stats(xb_ctx *c, int64_t *lean_launches, int64_t *generic_launches) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (lean_launches) *lean_launches = c->stat_lean_retraces;
    if (generic_launches) *generic_launches = c->stat_generic_retraces;
    return XB_OK;
}
int xb_trace_stats(xb_ctx *c, int64_t *nb_lean_launches, int64_t *lookup_lean_launches, int64_t *generic_launches, int64_t *wide_lean_launches) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (wide_lean_launches) *wide_lean_launches = c->stat_wide_traces;
    if (nb_lean_launches) *nb_lean_launches = c->stat_nb_traces;
    if (lookup_lean_launches) *lookup_lean_launches = c->stat_lookup_traces;
    if (generic_launches) *generic_launches = c->stat_generic_traces;
    return XB_OK;
}
int xb_retrace_overflow(xb_ctx *c, int32_t *out, int64_t capacity, int64_t *n) {
    if (!c || !n || capacity < 0 || (capacity > 0 && !out)) return fail(XB_E_ARG, "xb_retrace_overflow: null ctx / count, or a capacity without a buffer");
    *n = (int64_t)c->dbg_retrace_ovf.size();
    if (capacity >= *n) {   // (handed over: the next retraces start a new record)
        std::copy(c->dbg_retrace_ovf.begin(), c->dbg_retrace_ovf.end(), out);
        c->dbg_retrace_ovf.clear();
    }
    return XB_OK;
}
int xb_slow_path_stats(xb_ctx *c, int64_t *assign_total, int64_t *refine_total) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (assign_total) *assign_total = c->stat_ovf_assign;
    if (refine_total) *refine_total = c->stat_ovf_refine;
    return XB_OK;
}
// device bytes this context holds for the grid: density, labels, flags, numbering, the table (its window), scratch
int xb_memory_stats(xb_ctx *c, int64_t *bytes_total, int64_t *bytes_table, int64_t *bytes_scratch) {
    if (!c || !c->has_grid) return fail(XB_E_STATE, "xb_memory_stats: no grid");
    const long long N = c->N;
    const long long table = c->grad_cap * (long long)sizeof(GradRec);
    const long long scratch = c->list_cap * 4 + (long long)c->stage_bytes + c->ec_buf_cap * 4 + (c->ec_pend ? 8 * N + 16 : 0) +
                              (long long)buf_counted_bytes(*c) /* what the analyses keep: the blocks of ctx_buffers.h */;
    const long long fixed = 8 * N /* rho */ + 4 * N /* labels */ + (N + 16) /* known */ + 4 * N /* first */ + N /* st */ +
                            2LL * c->max_cap * 4 + (long long)c->ovf_cap * 4 + c->blab_alloc * 13 + (long long)c->walk_cap * 3 * 80 +
                            (1 << 22) /* boxbuf */;
    if (bytes_total) *bytes_total = fixed + table + scratch;
    if (bytes_table) *bytes_table = table;
    if (bytes_scratch) *bytes_scratch = scratch;
    return XB_OK;
}
int xb_box_stats(xb_ctx *c, int64_t *n_boxes, int64_t *box_voxels) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    if (n_boxes) *n_boxes = c->n_boxes;
    if (box_voxels) *box_voxels = c->box_voxels;
    return XB_OK;
}
int xb_brick_labels(xb_ctx *c, int32_t *out, int64_t capacity, int64_t dims[3]) {
    if (!c || !c->has_grid) return fail(XB_E_STATE, "xb_brick_labels: no grid");
    if (!c->blab) return fail(XB_E_STATE, "xb_brick_labels: no trapping regions on this context (no neargrid assignment yet)");
    const int64_t nbr = (int64_t)c->nbk[0] * c->nbk[1] * c->nbk[2];
    if (dims) { dims[0] = c->nbk[0]; dims[1] = c->nbk[1]; dims[2] = c->nbk[2]; }
    if (!out) return XB_OK;
    if (capacity < nbr) return fail(XB_E_ARG, "xb_brick_labels: capacity too small");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(out, c->blab, nbr * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
#ifdef XB_DEBUG_COUNT
// the lean walkers / the retraces note their step counts per start voxel in a buffer of their own (tools/walk_lengths.py)
int xb_debug_steps(xb_ctx *c, int on, signed char *host_out) {
    static signed char *buf = nullptr;
    if (host_out && buf) {
        if (hipMemcpy(host_out, buf, (size_t)c->N, hipMemcpyDeviceToHost) != hipSuccess) return XB_E_HIP;
    }
    if (on && !buf && hipMalloc(&buf, (size_t)c->N) != hipSuccess) return XB_E_HIP;
    if (on && hipMemset(buf, 0, (size_t)c->N) != hipSuccess) return XB_E_HIP;
    signed char *p = on ? buf : nullptr;
    return hipMemcpyToSymbol(HIP_SYMBOL(xb_dbg_steps), &p, sizeof p) == hipSuccess ? XB_OK : XB_E_HIP;
}
int xb_debug_counts(unsigned long long *out, int reset) {
    hipDeviceSynchronize();
    if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(xb_dbg), sizeof(unsigned long long) * 65536) != hipSuccess) return XB_E_HIP;
    if (reset) {
        static unsigned long long z[65536];
        if (hipMemcpyToSymbol(HIP_SYMBOL(xb_dbg), z, sizeof z) != hipSuccess) return XB_E_HIP;
    }
    return XB_OK;
}
#endif
int xb_enable_timing(xb_ctx *c, int on) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    // 0: off; 1: every timer; otherwise bit k + 1 switches timer k on (an event pair costs ~10 us of an idle stream between
    // dependent kernels: a benchmark times its step with the dominant kernel's timer alone)
    c->timing = on == 0 ? 0u : (on == 1 ? (1u << XB_TIMER_COUNT) - 1u : ((unsigned)on >> 1));
    return XB_OK;
}
int xb_kernel_time_reset(xb_ctx *c) {
    if (!c) return fail(XB_E_ARG, "null ctx");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (TimedKernel &t : c->tk) {
        for (auto &p : t.pending) { hipEventDestroy(p.first); hipEventDestroy(p.second); }
        t.pending.clear();
        t.ms = 0.;
        t.launches = 0;
    }
    return XB_OK;
}
int xb_kernel_time(xb_ctx *c, int which, double *ms_total, int64_t *launches) {
    if (!c || which < 0 || which >= XB_TIMER_COUNT) return fail(XB_E_ARG, "xb_kernel_time: bad argument");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    TimedKernel &t = c->tk[which];
    for (auto &p : t.pending) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, p.first, p.second));
        t.ms += ms;
        t.launches++;
        hipEventDestroy(p.first);
        hipEventDestroy(p.second);
    }
    t.pending.clear();
    if (ms_total) *ms_total = t.ms;
    if (launches) *launches = t.launches;
    return XB_OK;
}

}  // extern "C"

#include "comm.h"
#include "slab_step.h"
