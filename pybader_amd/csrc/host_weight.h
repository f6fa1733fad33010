// host_weight.h -- host side, part 8: the weight method (k_weight.h).  xb_weight_sum reads the resident density as the partition
// field rho and the resident labels for their -1 marks only; it writes neither.  The integrand q is rho itself, a host array or a
// device array (checked and ordered as xb_import_density), and goes straight into the accumulator A.
//
// Buffers: S (8 N bytes) lives in `stage` where that holds the grid (always on one GPU); A, V (8 N each), pending (N) and the two
// work lists (4 N each) are the context's own, allocated by the first call on a grid and kept while the grid stays or until
// xb_weight_release; whether S needs a buffer of its own is decided with that allocation (`stage` never shrinks under a grid).
// They are the blocks BLK_W_* of ctx_buffers.h.  (`list` is not borrowed: the walk list of the last assignment lives in it across calls.)
//
// Scheduling: a batch is W_BATCH level launches (each sizes itself from the device-side list length) followed by one launch of
// the single-workgroup tail, which takes over while the frontier holds at most W_CROSS voxels; the host waits once per batch to
// read the state.  Every batch on a non-empty frontier finishes at least one voxel, so the loop ends after at most N batches; an
// empty frontier with voxels left over is an error code, never a spin.

#define W_BATCH 32        // level launches per batch (one host wait per batch)
#define W_CROSS 2048      // frontiers up to this many voxels run in the single-workgroup tail (two voxels per thread)
#define W_LEVEL_GROUPS 1024   // workgroups of a level launch (four per compute unit, striding over the list): each takes one ticket

// the last call's results go (the blocks BLK_W_A .. BLK_W_STATE are released by the caller)
static void weight_forget(xb_ctx *c) {
    c->w_have = false;
    std::vector<int64_t>().swap(c->w_idx); std::vector<double>().swap(c->w_charge); std::vector<double>().swap(c->w_volume);
}
// device bytes of the weight buffers as xb_memory_stats counts them: 25 N, and 8 N more with an S of their own
static long long weight_bytes(const xb_ctx *c) {
    long long n = 0;
    for (int b = BLK_W_A; b <= BLK_W_LIST1; b++) n += (long long)c->bytes(b);
    return n;
}

static int weight_alpha(const char *who, const double alpha[27], WAlpha &al) {
    if (!alpha) return fail(XB_E_ARG, "%s: null alpha", who);
    auto neg = [](int i) { return i == 0 ? 0 : 3 - i; };
    for (int n = 0; n < 27; n++) {
        const double a = alpha[n];
        const int m = neg(n / 9) * 9 + neg((n / 3) % 3) * 3 + neg(n % 3);
        if (!(a >= 0.) || !std::isfinite(a)) return fail(XB_E_ARG, "%s: alpha[%d] = %g is not a finite weight >= 0", who, n, a);
        if (std::memcmp(&a, &alpha[m], sizeof a) != 0) return fail(XB_E_ARG, "%s: alpha is not symmetric (entries %d and %d)", who, n, m);
        al.a[n] = a;
    }
    if (alpha[0] != 0.) return fail(XB_E_ARG, "%s: the centre weight must be 0", who);
    return XB_OK;
}

// everything a call needs before the integrand arrives: a whole grid on this context, the weights, the buffers
static int weight_prepare(xb_ctx *c, const char *who, const double alpha[27], double voxel_volume, WAlpha &al) {
    if (int rc = analysis_ready(c, who, "the weight method needs", NEED_WHOLE)) return rc;
    if (!std::isfinite(voxel_volume)) return fail(XB_E_ARG, "%s: bad voxel volume", who);
    if (int rc = weight_alpha(who, alpha, al)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const size_t N = (size_t)c->N;
    // all or none; pending takes whole 32-bit words beyond N (the decrement's atomic) and counts N; S only where `stage` cannot hold it
    const BufWant want[] = {{BLK_W_A, N * sizeof(double), 0}, {BLK_W_V, N * sizeof(double), 0}, {BLK_W_PENDING, N, ((N + 7) & ~(size_t)3) - N},
                            {BLK_W_LIST0, N * sizeof(int), 0}, {BLK_W_LIST1, N * sizeof(int), 0}, {BLK_W_STATE, WS_COUNT * sizeof(int), 0},
                            {BLK_W_S, c->stage_bytes < N * sizeof(double) ? N * sizeof(double) : 0, 0}};
    if (int rc = reserve(c, want)) return rc;
    c->w_have = false;
    return XB_OK;
}

// passes 1 and 2 on an initialised A, then the maxima and their sums into the context's host vectors
static int weight_run(xb_ctx *c, const char *who, const WAlpha &al, double voxel_volume, int64_t *n_maxima) {
    const Grid &g = c->g;
    const long long N = c->N;
    double *const w_A = c->ptr<double>(BLK_W_A), *const w_V = c->ptr<double>(BLK_W_V), *const w_S = c->ptr<double>(BLK_W_S);
    unsigned char *const w_pending = c->ptr<unsigned char>(BLK_W_PENDING);
    int *const w_list[2] = {c->ptr<int>(BLK_W_LIST0), c->ptr<int>(BLK_W_LIST1)}, *const w_state = c->ptr<int>(BLK_W_STATE);
    double *S = w_S ? w_S : (double *)c->stage;
    if (!w_S) stage_clobbered(*c);   // (S goes into `stage`)
    const int *labels = (c->has_vacuum && !c->opt.weight_no_labels) ? c->labels : nullptr;
    HIPCHK(hipMemsetAsync(w_state, 0, WS_COUNT * sizeof(int), c->stream));
    const long long tiles = (long long)((g.nx + WT_X - 1) / WT_X) * ((g.ny + WT_Y - 1) / WT_Y) * ((g.nz + WT_Z - 1) / WT_Z);
    if (tiles > XB_INT_MAX) return fail(XB_E_LIMIT, "%s: %lld tiles exceed the launch grid", who, tiles);
    k_w_flux<<<(unsigned)tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, al, c->rho, labels, S, w_pending, w_list[0], w_state);
    HIPCHK(hipGetLastError());
    int ws[WS_COUNT];
    long long batches = 0;
    for (;;) {
        for (int k = 0; k < W_BATCH; k++)
            k_w_level<<<W_LEVEL_GROUPS, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, al, c->rho, S, w_A, w_V, w_pending, w_list[0], w_list[1], w_state);
        k_w_tail<<<1, W_TAIL_THREADS, 0, c->stream>>>(g.nx, g.ny, g.nz, al, c->rho, S, w_A, w_V, w_pending, w_list[0], w_list[1], w_state, W_CROSS);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(ws, w_state, sizeof ws, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        batches++;
        if (ws[WS_N0 + ws[WS_CUR]] == 0) break;
        if (batches > N) return fail(XB_E_STATE, "%s: no end after %lld batches", who, batches);   // (cannot happen: a batch finishes a voxel)
    }
    c->w_stat[0] = ws[WS_LEVELS]; c->w_stat[1] = ws[WS_BATCHED]; c->w_stat[2] = ws[WS_TAIL]; c->w_stat[3] = batches;
    c->w_stat[4] = ws[WS_DONE]; c->w_stat[5] = ws[WS_PEAK];
    if (ws[WS_DONE] != ws[WS_TOTAL])
        return fail(XB_E_STATE, "%s: the frontier is empty after %d levels with %d of %d voxels finished (a NaN in the density?)", who,
                    ws[WS_LEVELS], ws[WS_DONE], ws[WS_TOTAL]);
    // the maxima: listed in any order, sorted by voxel index here (the C-order scan order the library numbers maxima in)
    k_w_maxima<<<(unsigned)std::min<long long>(nblocks(N), 4096), TPB, 0, c->stream>>>(S, N, w_list[0], w_state);
    HIPCHK(hipGetLastError());
    int M = 0;
    HIPCHK(hipMemcpyAsync(&M, w_state + WS_NMAX, sizeof M, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int> idx(M);
    std::vector<double> av(2 * (size_t)M);
    if (M) {
        DevBuf<double> out;
        HIPCHK(out.alloc(2 * (size_t)M));
        k_w_gather<<<nblocks(M), TPB, 0, c->stream>>>(w_list[0], M, w_A, w_V, out.p);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(idx.data(), w_list[0], (size_t)M * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(av.data(), out.p, 2 * (size_t)M * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    std::vector<int> order(M);
    for (int k = 0; k < M; k++) order[k] = k;
    std::sort(order.begin(), order.end(), [&](int a, int b) { return idx[a] < idx[b]; });
    c->w_idx.resize(M); c->w_charge.resize(M); c->w_volume.resize(M);
    for (int k = 0; k < M; k++) {
        c->w_idx[k] = idx[order[k]];
        c->w_charge[k] = av[order[k]] * voxel_volume;
        c->w_volume[k] = av[(size_t)M + order[k]] * voxel_volume;
    }
    c->w_have = true;
    if (n_maxima) *n_maxima = M;
    return XB_OK;
}

int xb_weight_sum(xb_ctx *c, const double alpha[27], double voxel_volume, const double *q_host, int64_t *n_maxima) {
    WAlpha al;
    if (int rc = weight_prepare(c, "xb_weight_sum", alpha, voxel_volume, al)) return rc;
    if (q_host) {
        if (int rc = staged_h2d(c, c->ptr<double>(BLK_W_A), q_host, (size_t)c->N * sizeof(double))) return rc;
    } else
        HIPCHK(hipMemcpyAsync(c->ptr<double>(BLK_W_A), c->rho, (size_t)c->N * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    return weight_run(c, "xb_weight_sum", al, voxel_volume, n_maxima);
}

// the integrand from a device array: dtype, strides, allocation and stream ordering as xb_import_density checks them
int xb_weight_sum_device(xb_ctx *c, const double alpha[27], double voxel_volume, const void *dev_ptr, int dtype,
                         const int64_t stride[3], void *stream, int64_t *n_maxima) {
    ANALYSIS_NEED_GRID("xb_weight_sum_device");
    const size_t isz = io_float_size(dtype);
    if (!isz) return fail(XB_E_ARG, "xb_weight_sum_device: dtype code %d is neither XB_F32 nor XB_F64", dtype);
    if (!stride) return fail(XB_E_ARG, "xb_weight_sum_device: null stride");
    if ((uintptr_t)dev_ptr % isz) return fail(XB_E_ARG, "xb_weight_sum_device: %p is not aligned to its %zu-byte elements", dev_ptr, isz);
    HIPCHK(hipSetDevice(c->device));
    const int64_t shape[3] = {c->g.nx, c->g.ny, c->g.nz};
    uintptr_t lo, hi;
    if (int rc = io_check(c, "xb_weight_sum_device", dev_ptr, isz, shape, stride, &lo, &hi)) return rc;
    WAlpha al;
    if (int rc = weight_prepare(c, "xb_weight_sum_device", alpha, voxel_volume, al)) return rc;
    if (io_overlaps(lo, hi, c->ptr<double>(BLK_W_A), (size_t)c->N * 8)) return fail(XB_E_ARG, "xb_weight_sum_device: the source overlaps the library's accumulator");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = io_after_caller(c, s)) return rc;
    if (int rc = dtype == XB_F32 ? io_import_density(c, (const float *)dev_ptr, stride, c->ptr<double>(BLK_W_A)) : io_import_density(c, (const double *)dev_ptr, stride, c->ptr<double>(BLK_W_A))) return rc;
    if (int rc = io_before_caller(c, s)) return rc;
    return weight_run(c, "xb_weight_sum_device", al, voxel_volume, n_maxima);
}

int xb_weight_fetch(xb_ctx *c, int64_t *max_idx, double *charge, double *volume, int64_t capacity) {
    if (!c || !c->w_have) return fail(XB_E_STATE, "xb_weight_fetch: no finished xb_weight_sum on this context");
    const int64_t M = (int64_t)c->w_idx.size();
    if (capacity < M) return fail(XB_E_ARG, "xb_weight_fetch: capacity %lld below the %lld maxima", (long long)capacity, (long long)M);
    for (int64_t k = 0; k < M; k++) {
        if (max_idx) max_idx[k] = c->w_idx[k];
        if (charge) charge[k] = c->w_charge[k];
        if (volume) volume[k] = c->w_volume[k];
    }
    return XB_OK;
}

// the last xb_weight_sum: out = {levels, levels run as batched launches, levels run in the single-workgroup tail, batches (host
// waits of the level loop), voxels finished, largest frontier a batched level handed on, device bytes of the weight buffers}
int xb_weight_stats(xb_ctx *c, int64_t out[7]) {
    if (!c || !out) return fail(XB_E_ARG, "xb_weight_stats: null argument");
    for (int k = 0; k < 6; k++) out[k] = c->w_stat[k];
    out[6] = weight_bytes(c);
    return XB_OK;
}
