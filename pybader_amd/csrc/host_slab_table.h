// host_slab_table.h -- host side, part 6: the table window of a slab and the host-driven slab table calls (xb_table_build /
// xb_table_finish: the fallback of slab_step.h), raw device pointers and plane copies for the transports.


int xb_set_table_window(xb_ctx *c, int64_t margin) {
    NEED_GRID("xb_set_table_window");
    Grid &g = c->g;
    drop_table(*c);
    c->table_stage = 0;
    const int own = g.x1 - g.x0;
    if (margin < 0 || own == g.nx) { g.wx0 = 0; g.wlen = g.nx; c->table_margin = -1; g.wbase = 0; return XB_OK; }
    if (g.nx % 8 || g.ny % 8 || g.nz % 8 || g.x0 % 8 || g.x1 % 8)
        return fail(XB_E_ARG, "xb_set_table_window: grid and slab must be made of whole 8^3 bricks");
    const int m8 = (int)((std::max<int64_t>(margin, c->halo) + 7) / 8) * 8;
    if (own + 2 * m8 >= g.nx) { g.wx0 = 0; g.wlen = g.nx; c->table_margin = -1; g.wbase = 0; return XB_OK; }
    g.wx0 = ((g.x0 - m8) % g.nx + g.nx) % g.nx;
    g.wlen = own + 2 * m8;
    c->table_margin = m8;
    return need_grad(c);     // the table shrinks to the window: 32 B per voxel of slab + margins instead of the grid
}
static bool slab_sparse_ok(const xb_ctx *c) {
    const Grid &g = c->g;
    return c->opt.boxes && c->opt.bricks && table_windowed(c) && g.nx % BRK == 0 && g.ny % BRK == 0 && g.nz % BRK == 0 &&
           g.x0 % BRK == 0 && g.x1 % BRK == 0 && g.ny >= 16 && g.nz >= 16 && 7LL * (c->N / (BRK * BRK * BRK)) <= c->N;
}
int xb_table_build(xb_ctx *c, int64_t *n_local_seeds) {
    NEED_GRID_RAW("xb_table_build");   // (no label is read here: a deferred labels := 0 stays deferred)
    if (int rc = need_grad(c)) return rc;
    c->slab_sparse = false;
    if (slab_sparse_ok(c)) {
        // pass A over the OWN planes: move masks, maxima count and the single maximum of every own brick (k_brick_masks);
        // the scheduler shares both arrays, xb_table_finish grows the regions and builds the records of the window
        Grid &g = c->g;
        const int nb1 = g.ny / BRK, nb2 = g.nz / BRK, nbr = (g.nx / BRK) * nb1 * nb2;
        if (int rc = ensure_brick_bytes(c, nbr)) return rc;
        int *fs = c->fs, *bmask = c->list + nbr, *bmaxv = c->list + 4 * nbr;
        HIPCHK(hipMemsetAsync(fs, 0, FS_TOTAL * sizeof(int), c->stream));
        g.main_ties = 1;
        {
            ScopedTimer t_growth(c, XB_TIMER_MASKS_GROWTH);
            ScopedTimer t_masks(c, XB_TIMER_BRICK_MASKS);
            launch_brick_masks(c, false, false, bmask, bmaxv, nullptr);
        }
        HIPCHK(hipGetLastError());
        int ties = 0;
        HIPCHK(hipMemcpyAsync(c->host_ints, fs + FS_TIES, sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        ties = c->host_ints[0];
        c->window_ties = ties != 0;
        c->window_seeds.clear();
        c->grad_valid = true;     // (records follow in xb_table_finish)
        c->grad_cover = 1;
        c->grad_rule = 1;
        c->blab = nullptr;
        c->n_boxes = 0; c->box_voxels = 0;
        c->table_stage = 1;
        c->slab_sparse = true;
        if (n_local_seeds) *n_local_seeds = 0;
        return XB_OK;
    }
    if (int rc = ensure_grad(c, true, true, true)) return rc;
    if (n_local_seeds) *n_local_seeds = table_windowed(c) ? (int64_t)c->window_seeds.size() : 0;
    return XB_OK;
}
int xb_table_local_seeds(xb_ctx *c, int64_t *out, int64_t capacity) {
    NEED_GRID_RAW("xb_table_local_seeds");   // (no label is read here: a deferred labels := 0 stays deferred)
    if ((int64_t)c->window_seeds.size() > capacity) return fail(XB_E_ARG, "xb_table_local_seeds: capacity too small");
    for (size_t i = 0; i < c->window_seeds.size(); i++) out[i] = c->window_seeds[i];
    return XB_OK;
}
int xb_brick_masks(xb_ctx *c, void **dev_ptr, int64_t *n_bricks, int64_t *own_first, int64_t *own_count) {
    NEED_GRID_RAW("xb_brick_masks");   // (no label is read here: a deferred labels := 0 stays deferred)
    const Grid &g = c->g;
    if (g.nx % 8 || g.ny % 8 || g.nz % 8) return fail(XB_E_STATE, "xb_brick_masks: grid is not made of whole bricks");
    const int64_t nbr = c->N / 512, per_plane = (int64_t)(g.ny / 8) * (g.nz / 8);
    if (dev_ptr) *dev_ptr = (void *)(c->list + nbr);
    if (n_bricks) *n_bricks = nbr;
    if (own_first) *own_first = (g.x0 / 8) * per_plane;
    if (own_count) *own_count = ((g.x1 - g.x0) / 8) * per_plane;
    return XB_OK;
}
int xb_table_ties(xb_ctx *c, int64_t *has_ties) {
    NEED_GRID_RAW("xb_table_ties");   // (no label is read here: a deferred labels := 0 stays deferred)
    if (c->table_stage < 1 || !c->grad_valid) return fail(XB_E_STATE, "xb_table_ties: call xb_table_build first");
    if (has_ties) *has_ties = c->window_ties ? 1 : 0;
    return XB_OK;
}
int xb_table_finish(xb_ctx *c, const int64_t *seeds, int64_t n_seeds, int64_t any_ties) {
    NEED_GRID_RAW("xb_table_finish");   // (no label is read here: a deferred labels := 0 stays deferred)
    if (c->table_stage < 1 || !c->grad_valid) return fail(XB_E_STATE, "xb_table_finish: call xb_table_build first");
    // the records serve both tie rules (and the regions are closed for the refinement's retraces too) only when NO
    // rank's window holds a tie voxel
    c->grad_rule = any_ties ? 1 : 2;
    if (c->slab_sparse) {
        // every rank holds every brick's mask / maximum now: the same seeding + growth as on one GPU (replicated: the brick
        // arrays are tiny), then the 32-byte records for the uncertain bricks of THIS rank's window
        Grid &g = c->g;
        const int nb0 = g.nx / BRK, nb1 = g.ny / BRK, nb2 = g.nz / BRK, nbr = nb0 * nb1 * nb2;
        int *fs = c->fs;
        int *seed = c->list, *bmask = c->list + nbr, *buf0 = c->list + 2 * nbr, *buf1 = c->list + 3 * nbr, *bmaxv = c->list + 4 * nbr,
            *reclist = c->list + 5 * nbr;
        int *box_max = c->boxbuf + BB_REGMAX, *box_first = c->boxbuf + BB_REGFIRST;
        c->box_max_tab = box_max;
        ScopedTimer t_growth(c, XB_TIMER_MASKS_GROWTH);
        launch_region_growth(c, nb0, nb1, nb2, bmask, bmaxv, nullptr, seed, buf0, buf1, box_max, box_first, false);
        c->blab = c->blab_buf;
        c->nbk[0] = nb0; c->nbk[1] = nb1; c->nbk[2] = nb2;
        launch_window_bricks(c, reclist, fs + FS_N_WALK, nullptr);
        {
            ScopedTimer t_records(c, XB_TIMER_BRICK_RECORDS);
            g.main_ties = 1;
            launch_brick_records(c, reclist, fs + FS_N_WALK, nbr, nb1, nb2);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(c->host_ints, fs, FS_COUNT * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        c->n_boxes = c->host_ints[FS_N_BOXES];
        c->box_voxels = (long long)c->host_ints[FS_N_CERTAIN] * BRK * BRK * BRK;
        if (!c->host_ints[FS_GROW_CONVERGED] || c->n_boxes == 0) c->blab = nullptr;   // no regions: plain tracing of the slab
        c->table_stage = 2;
        c->table_prebuilt = true;
        return XB_OK;
    }
    // (no trapping regions on this route: the records of every voxel of the window are there, the slab is traced in full)
    (void)seeds; (void)n_seeds;
    c->table_stage = 2;
    c->table_prebuilt = true;
    return XB_OK;
}

void *xb_labels_ptr(xb_ctx *c) {
    if (!c) return nullptr;
    settle_labels(c);
    c->have_labels = true;   // (whoever holds the pointer may write them)
    return (void *)c->labels;
}
void *xb_known_ptr(xb_ctx *c) { return c ? (void *)c->known : nullptr; }
void *xb_density_ptr(xb_ctx *c) {
    if (c) density_pointer_out(*c);   // (whoever holds the pointer may write it)
    return c ? (void *)c->rho : nullptr;
}
int64_t xb_plane_elems(xb_ctx *c) { return c ? c->g.nyz : 0; }

int xb_copy_planes(xb_ctx *c, int which, int to_device, void *host, int64_t xa, int64_t xb) {
    NEED_GRID("xb_copy_planes");
    if (xa < 0 || xb > c->g.nx || xa > xb) return fail(XB_E_ARG, "xb_copy_planes: bad plane range");
    const size_t es = which == 0 ? 4 : 1;
    char *dev = which == 0 ? (char *)c->labels : (char *)c->known;
    const size_t off = (size_t)xa * c->g.nyz * es, bytes = (size_t)(xb - xa) * c->g.nyz * es;
    // (a slab's halo planes come from peers that ran the same assignment: the regions' labels stay what they are)
    // (planes from outside: any label may arrive -- but the halo's wire width must stay a collectively agreed value, so it is
    // widened only when a label of these planes does not fit it: never for planes of peers that ran the same assignment)
    // On the whole grid nothing is known of the planes: no label mark survives and the vacuum counts as back, -1 among them or not.
    // (the -1 labels are no longer xb_vacuum_assign's either way: a plane may zero a voxel below the tolerance)
    const bool whole = c->g.x1 - c->g.x0 == c->g.nx;
    if (to_device && which == 0) {
        bool any_negative = false;
        const int wire = labels_fit_wire((const int32_t *)host, (xb - xa) * c->g.nyz, &any_negative);
        labels_patched(*c, wire, any_negative || whole, whole ? LABEL_MARKS_NONE : (c->buni_halo_safe ? LABEL_MARKS_BOTH : LABEL_MARKS_REGIONS), false);
    } else if (to_device) {   // planes of `known`
        drop_edge_lists(*c); c->has_vacuum = c->has_vacuum || whole;
        c->buni_valid = c->buni_valid && c->buni_halo_safe && !whole;
        if (whole) drop_label_marks(*c);
    }
    if (to_device) HIPCHK(hipMemcpyAsync(dev + off, host, bytes, hipMemcpyHostToDevice, c->stream));
    else HIPCHK(hipMemcpyAsync(host, dev + off, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

// The narrowest signed width (1 / 2 / 4 bytes) that holds every resident label: what a label halo travels in
// (xb_comm_exchange_planes).  It changes in calls that every rank of a slab run makes with the same arguments (numbering,
// uploads, vacuum_assign, volume_assign); `widen_to` (1, 2, 4; 0: only ask) raises it so that a scheduler can make the ranks
// agree after a per-rank event (max over the ranks) -- send and receive sizes must match.
int xb_label_wire(xb_ctx *c, int widen_to, int *wire_out) {
    if (!c) return fail(XB_E_ARG, "xb_label_wire: null context");
    if (widen_to != 0 && widen_to != 1 && widen_to != 2 && widen_to != 4) return fail(XB_E_ARG, "xb_label_wire: width must be 0, 1, 2 or 4");
    c->label_wire = std::max(c->label_wire, widen_to);
    if (wire_out) *wire_out = c->label_wire;
    return XB_OK;
}

int xb_brick_masks_copy(xb_ctx *c, int to_device, int32_t *host, int64_t first, int64_t count) {
    NEED_GRID_RAW("xb_brick_masks_copy");   // (no label is read here: a deferred labels := 0 stays deferred)
    const int64_t nbr = c->N / 512;
    if (!host || first < 0 || count < 0 || first + count > nbr) return fail(XB_E_ARG, "xb_brick_masks_copy: bad chunk");
    // host holds 2 * count ints: the move masks of the chunk, then the single-maximum voxels (k_brick_masks)
    int *masks = c->list + nbr, *maxvox = c->list + 4 * nbr;
    if (to_device) {
        HIPCHK(hipMemcpyAsync(masks + first, host, count * sizeof(int), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(maxvox + first, host + count, count * sizeof(int), hipMemcpyHostToDevice, c->stream));
    } else {
        HIPCHK(hipMemcpyAsync(host, masks + first, count * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(host + count, maxvox + first, count * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
