// host_stages.h -- host side, part 2b: the launches of the stages every assignment path shares (the fused one-GPU
// assignments, the host-driven calls, the windowed slab table and the device-driven slab step), one function per stage,
// and the small policies they agree on.  Each function issues exactly the launches its callers issued before; where the
// paths differ, the difference is a parameter.

// layout of the small device int buffer of the region growth (c->boxbuf): maximum / first brick of up to XB_REGIONS_MAX
// regions (k_seed_bricks)
enum { BB_TOTAL = 1 << 20, BB_REGMAX = 1 << 16, BB_REGFIRST = 1 << 17 };

static bool table_windowed(const xb_ctx *c) { return c->g.wlen < c->g.nx; }
// the brick kernels' form for grids below 16 voxels on an axis or 80 along z (k_masks.h)
static int small_grid(const Grid &g) { return g.nx < 16 || g.ny < 16 || g.nz < 80; }
// the step bound of every trajectory
static int trace_maxsteps(const Grid &g) { return 8 * (g.nx + g.ny + g.nz) + 64; }
// slabs: the regions' brick labels stop a retrace when the labels are this assignment's, there is no vacuum and
// the density has no tie voxel (the windowed masks are built under the assignment's tie rule only)
static const int *slab_regions_of(const xb_ctx *c) {
    const Grid &g = c->g;
    return (table_windowed(c) && c->blab && c->regions_labels && !c->has_vacuum && (c->grad_rule == 2 || c->slab_sparse) &&
            g.nx % 8 == 0 && g.ny % 8 == 0 && g.nz % 8 == 0) ? c->blab : nullptr;
}

// The prologue of an assignment: `counts` (n ints) zeroed, `first` refilled when a previous assignment did not finish (it may
// hold stale minima); invalidate: the label-derived state (brick uniformity, region labels, edge lists) goes too.
static_assert(CT_REDO == CT_N_MAX + 15, "a host-driven assignment zeroes CT_N_MAX .. CT_REDO at once");
static int begin_assignment(xb_ctx *c, int *counts, int n, bool invalidate) {
    HIPCHK(hipMemsetAsync(counts, 0, n * sizeof(int), c->stream));
    if (!c->first_clean) {
        k_fill<int><<<4096, TPB, 0, c->stream>>>(c->first, XB_INT_MAX, c->N);
        HIPCHK(hipGetLastError());
    }
    c->first_clean = false;
    c->regions_pending = false;
    if (invalidate) { drop_label_marks(*c); drop_edge_lists(*c); }
    return XB_OK;
}

// Pass A (k_brick_masks) over the planes x0..x1 under the assignment's tie rule (methods.py:324, the template argument): brick
// move masks, single maxima, potentials (bpot, may be null) and the tie flag.  part: the grid cuts its last bricks.
static void launch_brick_masks(xb_ctx *c, bool part, bool allow_diag, int *bmask, int *bmaxv, int *bpot) {
    const Grid &g = c->g;
    const dim3 grid((g.nz + GT_Z - 1) / GT_Z, (g.ny + GT_Y - 1) / GT_Y, (g.x1 - g.x0 + GT_X - 1) / GT_X);
    GridS gs;
    const bool sym = sym_grid(g, gs);
    int mirror = 0;
    double mu_scale = 0.;
    if (sym && c->opt.mirror) mirror_prefilter(g, mirror, mu_scale);
    // (an orthogonal lattice has a diagonal T_grad: exact zeros off the diagonal)
    const bool diag = allow_diag && c->opt.mask_diag && g.T[1] == 0. && g.T[2] == 0. && g.T[3] == 0. && g.T[5] == 0. && g.T[6] == 0. && g.T[7] == 0.;
    auto launch = [&](auto kernel, const auto &gt) {
        kernel<<<grid, TPB, 0, c->stream>>>(gt, c->rho, small_grid(g), bmask, bmaxv, c->fs + FS_TIES, g.x0, mu_scale, mirror, bpot);
    };
    if (!sym) launch(part ? k_brick_masks<Grid, 1, false, true> : k_brick_masks<Grid, 1, false>, g);
    else if (part) launch(diag ? k_brick_masks<GridS, 1, true, true> : k_brick_masks<GridS, 1, false, true>, gs);
    else launch(diag ? k_brick_masks<GridS, 1, true> : k_brick_masks<GridS, 1, false>, gs);
    c->brick_max_blanket = false;   // (pass A flags the bricks that hold a maximum, and only those)
}

// Pass B (k_brick_records): the 32-byte records of the listed bricks (list[0 .. *n_dev)), or of every brick whose
// brick_rec byte asks for them (list null).  Every caller writes ALL the records the table is then said to hold -- the walk
// list of an assignment after k_grow_finish has cleared the brick bytes, or every flagged brick -- never some bricks next to
// older ones.  So a launch over a whole-grid table of whole bricks can mark in every record which neighbour bricks hold none
// (grad_nb; a list must then be the bricks with blab <= 0 that are no vacuum bricks: the walk list), and every other launch --
// a slab's window, a grid that cuts its last bricks -- writes zeros there and says so.
static bool nb_bits_ok(const xb_ctx *c) { return c->grad_valid && c->grad_nb && c->opt.nb_bits; }
static void launch_brick_records(xb_ctx *c, const int *list, const int *n_dev, int nbr, int nb1, int nb2) {
    const Grid &g = c->g;
    const bool part = g.nx % BRK || g.ny % BRK || g.nz % BRK;
    const bool mark = !table_windowed(c) && g.x0 == 0 && g.x1 == g.nx && !part && (!list || c->blab) && c->nb_tab;
    c->grad_nb = mark;
    if (mark)   // (the bricks that hold records are known: the labels after the walk list was made, or the flags)
        k_nb_table<<<(nbr + 255) / 256, 256, 0, c->stream>>>(nbr / (nb1 * nb2), nb1, nb2, list ? c->blab : nullptr, c->brick_rec, c->nb_tab);
    auto launch = [&](auto kernel, const auto &gt) {
        kernel<<<4096, TPB, 0, c->stream>>>(gt, c->rho, c->grad, list, n_dev, nbr, nb1, nb2, c->brick_rec, small_grid(g),
                                            mark ? c->nb_tab : nullptr);
    };
    GridS gs;
    if (sym_grid(g, gs)) launch(k_brick_records<GridS>, gs);
    else launch(k_brick_records<Grid>, g);
}

// Region growth over the brick arrays of pass A: seeds are the bricks that hold exactly one maximum (no cubes, no cap on the
// number of maxima); they are not fixed: the kill iteration certifies them like every other brick.  chase: provisional labels
// by one chase along the brick potentials instead of ~6 propagation launches.  Leaves the brick labels in blab_buf.
static void launch_region_growth(xb_ctx *c, int nb0, int nb1, int nb2, int *bmask, int *bmaxv, int *bpot, int *seed, int *buf0,
                                 int *buf1, int *box_max, int *box_first, bool chase) {
    const int nbr = nb0 * nb1 * nb2;
    int *fs = c->fs;
    k_seed_bricks<<<(nbr + 255) / 256, 256, 0, c->stream>>>(nbr, bmask, bmaxv, fs, seed, buf0, box_max, box_first);
    if (chase) {   // (buf1 doubles as the parent array)
        k_grow_parent<<<(nbr + TPB - 1) / TPB, TPB, 0, c->stream>>>(nb0, nb1, nb2, bmask, bpot, seed, buf1);
        k_grow_chase<<<(nbr + TPB - 1) / TPB, TPB, 0, c->stream>>>(nbr, buf1, seed, buf0, 4 * (nb0 + nb1 + nb2) + 64, fs);
    } else
        k_seed_finish<<<1, 1, 0, c->stream>>>(fs);
    // the worst-case schedule; after a chase only the kill iteration is left, which dies out within a few bricks of the
    // dividing surfaces: a short schedule first, and a repeat of the whole assignment with the long one (FS_GROW_RETRY)
    // for the rare density whose cascade runs deeper
    const int long_schedule = 2 * ((std::max(std::max(nb0, nb1), nb2) + BG - 1) / BG) + 12;
    const int launches = chase ? std::min(long_schedule, c->grow_kill_launches) : long_schedule;
    const dim3 ggrid((nb2 + BG - 1) / BG, (nb1 + BG - 1) / BG, (nb0 + BG - 1) / BG);
    for (int l = 0; l < launches; l++)   // each returns at once when the growth has finished (phase on the device)
        k_brick_grow_dev<<<ggrid, BG * BG * BG, 0, c->stream>>>(nb0, nb1, nb2, bmask, seed, buf0, buf1, fs, BG, 0);
    k_grow_finish<<<64, TPB, 0, c->stream>>>(nbr, seed, buf0, buf1, fs, c->blab_buf, box_first, bmask, c->brick_rec, 0, chase && launches < long_schedule ? 1 : 0);
}

// The bricks of the table window (it may wrap round the grid) outside the regions -> list[0 .. *count): the ones that get
// records (k_brick_walk_list; skip: a flag that says there is nothing to list)
static void launch_window_bricks(xb_ctx *c, int *list, int *count, const int *skip) {
    const Grid &g = c->g;
    const int nb0 = c->nbk[0], per_plane = c->nbk[1] * c->nbk[2], nbr = nb0 * per_plane;
    const int w0 = g.wx0 / BRK, wn = g.wlen / BRK, run1 = std::min(wn, nb0 - w0);
    const unsigned grid = (nbr + 16 * TPB - 1) / (16 * TPB);
    k_brick_walk_list<<<grid, TPB, 0, c->stream>>>(nbr, w0 * per_plane, (w0 + run1) * per_plane, c->blab, list, count, skip);
    if (wn > run1) k_brick_walk_list<<<grid, TPB, 0, c->stream>>>(nbr, 0, (wn - run1) * per_plane, c->blab, list, count, skip);
}

// One GPU: the bricks of the whole grid outside the regions -> walk[0 .. *FS_N_WALK) in Morton order of their coordinates
// (k_brick_walk_list_morton; bpot: with a vacuum tolerance the bricks below it stay off the list).  The codes enumerate the cube
// of 2^bits bricks per axis that holds the grid; beyond XB_MORTON_BITS bits -- an axis of more than 8192 voxels -- they no longer
// fit the code word (1u << 3 * bits wrapped, and the list held a few bricks of the grid's corner: 64 of 65 536 basins found on
// 16 x 16 x 524288), and the list is made in linear brick order.
static void launch_walk_list(xb_ctx *c, int nb0, int nb1, int nb2, int *walk, const int *bpot, double vac_tol) {
    int bits = 0;
    while ((1 << bits) < std::max(std::max(nb0, nb1), nb2)) bits++;
    const bool linear = bits > XB_MORTON_BITS;
    const unsigned n_codes = linear ? (unsigned)(nb0 * nb1 * nb2) : 1u << (3 * bits);
    k_brick_walk_list_morton<<<(n_codes + 16 * TPB - 1) / (16 * TPB), TPB, 0, c->stream>>>(nb0, nb1, nb2, n_codes, linear ? 1 : 0, c->blab, walk,
                                                                                          c->fs + FS_N_WALK, c->fs + FS_GROW_RETRY, bpot, vac_tol);
}

// The persistent trace of the walk list's bricks (k_ng_trace_g): workgroups of XB_TRACE_WAVES waves, one brick per pull
// (per-XCD cursors over the list, its length on the device).  lean_ok: the lean walker, the own brick's records in LDS, when
// the index products fit 24 bits (32-bit table offsets up to 2^27 window voxels); otherwise the generic walker (XB_CHECK_GENERIC_WALKER:
// the tests' cross-check; planes or rows beyond 2^24 voxels), which tests every start voxel.  bres: per walk-list brick, did
// all its voxels end on one maximum (the lean walker only).  A trajectory that leaves a table window lands on a list (in
// `stage`, its length on the device) and is redone by the kernel that derives missing records from rho.  Returns whether the
// lean walker runs.
static bool launch_persistent_trace(xb_ctx *c, bool lean_ok, bool part, const int *box_max, const int *walk, int has_vacuum, int *bres) {
    const Grid &g = c->g;
    const int groups = std::max(1, c->trace_waves / XB_TRACE_WAVES);
    const int lean = lean_ok && light(g).use24 && c->opt.lean ? ((long long)g.wlen * g.nyz <= (1LL << 27) ? 4 : 3) : 0;
    const bool window = table_windowed(c);
    int *ovf = window ? (int *)c->stage : c->ovf_list;
    const int ovf_cap = window ? (int)std::min<size_t>(c->stage_bytes / sizeof(int), 0x7fffffffu) : c->ovf_cap;
    // (the neighbour bits: whole bricks, the whole grid, and a table that vouches for them -- else the brick label per step)
    const bool nb = lean && !window && !part && nb_bits_ok(c);
    (nb ? c->stat_nb_traces : lean ? c->stat_lookup_traces : c->stat_generic_traces)++;
    if (lean == 3) c->stat_wide_traces++;
    auto kernel = !lean ? k_ng_trace_g<2, 0>
                : nb ? (lean == 4 ? k_ng_trace_g<2, 4, false, false, true> : k_ng_trace_g<2, 3, false, false, true>)
                : window ? (lean == 4 ? k_ng_trace_g<2, 4, true> : k_ng_trace_g<2, 3, true>)
                : part ? (lean == 4 ? k_ng_trace_g<2, 4, false, true> : k_ng_trace_g<2, 3, false, true>)
                : (lean == 4 ? k_ng_trace_g<2, 4> : k_ng_trace_g<2, 3>);
    kernel<<<groups, XB_WAVE * XB_TRACE_WAVES, 0, c->stream>>>(light(g), c->grad, box_max, c->blab, c->nbk[1], c->nbk[2], walk, c->fs, c->labels,
                                                               c->first, c->max_list, c->max_cap, ovf, ovf_cap, trace_maxsteps(g), has_vacuum,
                                                               8, 1, lean ? bres : nullptr);
    if (window)
        k_ng_trace_list<2><<<512, TPB, 0, c->stream>>>(light(g), c->grad, box_max, c->blab, c->nbk[1], c->nbk[2], ovf, c->fs + FS_N_OVF, c->labels,
                                                       c->first, c->max_list, c->fs + FS_N_MAX, c->max_cap, c->ovf_list, c->counters + CT_N_OVF,
                                                       c->ovf_cap, trace_maxsteps(g), c->rho, c->dist_dev, has_vacuum);
    return lean != 0;
}

// The relabel after the numbering, then `first` left clean (INT_MAX everywhere) for the next assignment.  regions: the
// trapping regions brick by brick (one brick-label lookup per 8 rows; 16-byte stores when the rows are aligned; the launch
// covers 4-plane groups from x0 on) and, unless buni is BUNI_NONE, the per-brick label uniformity the edge sweep wants: the
// regions' bricks from their labels, the walk-list bricks from bres or by a scan, and -- BUNI_MIXED, a slab -- every other
// brick counted as mixed, right whatever the peers' halo planes bring.  Otherwise every voxel by its maximum's rank.
// fs: the device-driven paths -- each launch is gated on the device numbering (FS_SORT_OK), and the counts of regions, walk
// list and maxima are read there; without it the host's counts (c->n_boxes, c->n_walk, n_maxima).
enum { BUNI_NONE, BUNI_SCAN, BUNI_MIXED };
static void launch_relabel(xb_ctx *c, int *fs, int n_maxima, bool regions, const int *box_max, int buni, const int *bres) {
    const Grid &g = c->g;
    const GridL gl = light(g);
    const int nb1 = c->nbk[1], nb2 = c->nbk[2], nbr = c->nbk[0] * nb1 * nb2;
    const int *gate = fs ? fs + FS_SORT_OK : nullptr, *n_walk_dev = fs ? fs + FS_N_WALK : nullptr;
    int *ubuf = reinterpret_cast<int *>(c->st);
    if (regions) {
        const int v = g.nz % 4 == 0 ? 4 : 1;
        (v == 4 ? k_relabel_regions_brick<4> : k_relabel_regions_brick<1>)<<<dim3((g.nz / v + 63) / 64, nb1, (g.x1 - g.x0 + RELABEL_X - 1) / RELABEL_X), TPB, 0, c->stream>>>(
            gl, c->labels, c->first, c->blab, nb1, nb2, box_max, fs, gate, fs ? -1 : c->n_boxes);
        if (buni == BUNI_MIXED) k_fill<int><<<(nbr + 4 * TPB - 1) / (4 * TPB), TPB, 0, c->stream>>>(ubuf, XB_MIXED, nbr);
        if (buni != BUNI_NONE && bres)
            k_buni_after_relabel<<<(nbr + 255) / 256, 256, 0, c->stream>>>(nbr, c->blab, box_max, c->first, ubuf, gate, c->walk, n_walk_dev, bres);
        else if (buni != BUNI_NONE) {
            k_buni_after_relabel<<<(nbr + 255) / 256, 256, 0, c->stream>>>(nbr, c->blab, box_max, c->first, ubuf, gate, nullptr, nullptr, nullptr);
            if (fs) k_label_uniform_list<<<2048, TPB, 0, c->stream>>>(gl, c->labels, nb1, nb2, c->walk, 0, n_walk_dev, gate, ubuf);
            else if (c->n_walk)
                k_label_uniform_list<<<(c->n_walk + 3) / 4, TPB, 0, c->stream>>>(gl, c->labels, nb1, nb2, c->walk, c->n_walk, nullptr, nullptr, ubuf);
        }
    } else
        k_relabel<<<nblocks((long long)(g.x1 - g.x0) * g.nyz), TPB, 0, c->stream>>>(g, c->labels, c->first, gate);
    if (fs) k_reset_first<<<8, 256, 0, c->stream>>>(c->first, c->max_aux, 0, fs + FS_N_MAX, gate);
    else if (n_maxima) k_reset_first<<<(unsigned)((n_maxima + 255) / 256), 256, 0, c->stream>>>(c->first, c->max_aux, n_maxima, nullptr, nullptr);
}

// The bookkeeping once the maxima are numbered and the labels relabelled: `sorted` holds the nmax maxima in numbering order
// (null: c->maxima_sorted holds them already); `first` is clean again.
static void numbering_done(xb_ctx *c, const int *sorted, int nmax, int64_t *n_maxima) {
    if (sorted) c->maxima_sorted.assign(sorted, sorted + nmax);
    c->label_wire = label_wire_for(nmax);
    c->regions_pending = false;
    c->first_clean = true;
    if (n_maxima) *n_maxima = nmax;
}

// k_refine_trace with what every retrace passes alike: the table, labels / known, the density and distances of the from-rho
// form, the step bound.  (C++ linkage: the host parts are included inside an extern "C" block)
extern "C++" template <int K, bool RHO, bool RESUME = false, bool EXPORT = false, bool NB = false>
static void launch_refine_trace(xb_ctx *c, unsigned grid, int block, const int *list, int n_host, const int *n_dev, int *changed, int *escaped,
                                int *ovf_list, int *ovf_count, int ovf_cap, const unsigned char *brec, int *defer_list, int *defer_count,
                                int regions_ok, const int *region_blab, const WalkerIO &wio) {
    k_refine_trace<K, RHO, RESUME, EXPORT, NB><<<grid, block, 0, c->stream>>>(light(c->g), c->grad, c->labels, c->known, list, n_host, n_dev, changed,
                                                                           escaped, ovf_list, ovf_count, ovf_cap, trace_maxsteps(c->g), c->rho,
                                                                           c->dist_dev, brec, defer_list, defer_count, regions_ok, region_blab, wio);
}

// The first retrace of an edge list (a two-voxel window, on the table).  One GPU's common case takes k_refine_trace_lean
// (k_edges.h): the table is the whole grid's (no window, no slab), of whole bricks whose records carry valid neighbour bits (brec
// and nb_bits_ok), the labels are the last neargrid assignment's without vacuum (regions_ok: nothing is deferred, a retrace ends
// on the first brick without records), there are no slab regions, index products fit 24 bits and record byte offsets 32.
// Everything else -- and everything under XB_CHECK_GENERIC_RETRACE -- takes the generic kernel as before: with the neighbour bits
// where the table vouches for them (not on a slab), with the brick byte per step otherwise.
static bool lean_retrace_ok(const xb_ctx *c, const unsigned char *brec, bool slab, int regions_ok, const int *region_blab) {
    const Grid &g = c->g;
    return c->opt.lean_retrace && brec && !slab && nb_bits_ok(c) && regions_ok && !region_blab && !table_windowed(c) && g.x0 == 0 && g.x1 == g.nx &&
           g.vlen == g.nx && light(g).use24 && c->N <= (1LL << 27);
}
static void launch_edge_retrace(xb_ctx *c, unsigned grid, int block, const int *list, int n_host, const int *n_dev, int *changed, int *escaped,
                                int *ovf_count, const unsigned char *brec, bool slab, int *defer_list, int *defer_count, int regions_ok,
                                const int *region_blab) {
    if (lean_retrace_ok(c, brec, slab, regions_ok, region_blab)) {
        // (the lean kernel neither defers nor escapes -- regions_ok holds and there is no slab --: `escaped`, `defer_list` and
        // `defer_count` stay as the caller cleared them, and its from-rho pass finds an empty list)
        c->stat_lean_retraces++;
        k_refine_trace_lean<<<grid, block, 0, c->stream>>>(light(c->g), c->grad, c->labels, c->known, list, n_host, n_dev, changed, c->ovf_list, ovf_count,
                                                           c->ovf_cap, trace_maxsteps(c->g), brec);
        return;
    }
    c->stat_generic_retraces++;
    // (NB: `missing` from the neighbour bits of the record in hand -- a whole-grid table that vouches for them)
    (brec && !slab && nb_bits_ok(c) ? launch_refine_trace<2, false, false, false, true> : launch_refine_trace<2, false>)(
        c, grid, block, list, n_host, n_dev, changed, escaped, c->ovf_list, ovf_count, c->ovf_cap, brec, defer_list, defer_count, regions_ok, region_blab,
        WalkerIO{});
}
// XB_DBG_KEEP_RETRACE_OVERFLOW (tests): what the retraces just waited for put on the overflow list -- ovf_list[0 .. novf) -- is
// copied to the host before the middle tier and the exact slow kernel work it off; xb_retrace_overflow hands it out.
static int keep_retrace_overflow(xb_ctx *c, int novf) {
    if (!(c->opt.dbg & XB_DBG_KEEP_RETRACE_OVERFLOW) || novf <= 0) return XB_OK;
    const size_t at = c->dbg_retrace_ovf.size();
    c->dbg_retrace_ovf.resize(at + (size_t)novf);
    HIPCHK(hipMemcpyAsync(c->dbg_retrace_ovf.data() + at, c->ovf_list, (size_t)novf * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
