// host_nci.h -- host side, part 16: the NCI index (k_nci.h).  The three calls read the resident density (xb_nci_sum the resident
// labels too) of the whole grid and write neither.
//
// One block of the context (ctx_buffers.h), in 8-byte words:
//   BLK_NCI   xb_nci_sum: sum of rho [3 n], sum of rho^2 [3 n], counts [3 n] (64-bit integers)
//             xb_nci_hist: the thresholds T(e_j) [n_s + 1], the edges of x [n_x + 1], the counts [n_s n_x] (64-bit integers)
// xb_nci_field with host outputs writes s into `stage` (N doubles on a whole grid: need_scratch) and x into a temporary buffer of
// N doubles, and copies from there.

// T(e) of the definition: a = C e, a2 = a a, T = (a2 a2) a2
static inline double nci_threshold(double e) {
    const double a = XB_NCI_C * e, a2 = a * a;
    return (a2 * a2) * a2;
}

int xb_nci_field(xb_ctx *c, const double lattice[9], int flags, double *s_host, double *x_host, void *s_dev, void *x_dev) {
    ANALYSIS_NEED_GRID("xb_nci_field");
    if (!lattice) return fail(XB_E_ARG, "xb_nci_field: null argument");
    const bool host = s_host && x_host && !s_dev && !x_dev, dev = s_dev && x_dev && !s_host && !x_host;
    if (!host && !dev) return fail(XB_E_ARG, "xb_nci_field: either both host outputs or both device outputs are wanted");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_nci_field: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_nci_field", lattice, false, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const size_t bytes = (size_t)c->N * sizeof(double);
    double *ds = (double *)s_dev, *dx = (double *)x_dev;
    DevBuf<double> tmp;
    if (dev) {
        uintptr_t lo[2], hi[2];
        void *const out[2] = {s_dev, x_dev};
        for (int k = 0; k < 2; k++) {
            if (int rc = io_check_dense(c, "xb_nci_field", out[k], sizeof(double), &lo[k], &hi[k])) return rc;
            if (io_overlaps(lo[k], hi[k], c->rho, bytes)) return fail(XB_E_ARG, "xb_nci_field: a destination overlaps the resident density");
        }
        if (lo[0] < hi[1] && lo[1] < hi[0]) return fail(XB_E_ARG, "xb_nci_field: the two destinations overlap");
    } else {
        if (c->stage_bytes < bytes) return fail(XB_E_STATE, "xb_nci_field: the scratch buffer holds no whole grid");
        HIPCHK(tmp.alloc((size_t)c->N));
        stage_clobbered(*c);
        ds = (double *)c->stage;
        dx = tmp.p;
    }
    if (flags & XB_STENCIL_GATHER) k_nci_field_gather<<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, ds, dx);
    else k_nci_field<<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, ds, dx);
    HIPCHK(hipGetLastError());
    if (host) {
        if (int rc = staged_d2h(c, s_host, ds, bytes)) return rc;   // (waits)
        return staged_d2h(c, x_host, dx, bytes);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

int xb_nci_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, double s_cut, double rho_cut, double rho_split,
               int flags, int64_t *count, double *charge, double *charge2) {
    ANALYSIS_NEED_GRID("xb_nci_sum");
    if (!lattice || !count || !charge || !charge2) return fail(XB_E_ARG, "xb_nci_sum: null argument");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_nci_sum: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    if (n < 1) return fail(XB_E_ARG, "xb_nci_sum: %lld labels", (long long)n);
    if (!std::isfinite(s_cut) || !std::isfinite(rho_cut) || !std::isfinite(rho_split) || s_cut < 0. || rho_cut < 0. || rho_split < 0.)
        return fail(XB_E_ARG, "xb_nci_sum: the thresholds (%g, %g, %g) must be finite and not negative", s_cut, rho_cut, rho_split);
    if (n > XB_INT_MAX / 3) return fail(XB_E_LIMIT, "xb_nci_sum: %lld labels exceed %d", (long long)n, XB_INT_MAX / 3);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_nci_sum", lattice, true, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const Grid &g = c->g;
    const size_t keys = 3 * (size_t)n, want = 3 * keys;
    if (int rc = reserve(c, BLK_NCI, want * sizeof(double))) return rc;
    double *ds = c->ptr<double>(BLK_NCI), *dq = ds + keys;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(dq + keys);
    HIPCHK(hipMemsetAsync(ds, 0, want * sizeof(double), c->stream));
    const NciCuts C{nci_threshold(s_cut), rho_cut, rho_split};
    const bool bins = n <= NCI_LABELS_LDS;
    if (flags & XB_STENCIL_GATHER) {
        if (bins) k_nci_sum_gather<true><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
        else k_nci_sum_gather<false><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
    } else {
        if (bins) k_nci_sum<true><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
        else k_nci_sum<false><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
    }
    HIPCHK(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts travel as they are");
    HIPCHK(hipMemcpyAsync(charge, ds, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(charge2, dq, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(count, dc, keys * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < keys; i++) {
        charge[i] *= voxel_volume;
        charge2[i] *= voxel_volume;
    }
    return XB_OK;
}

// edges[0 .. n]: finite and strictly increasing (and, with `positive`, none below 0)
static int nci_edges_ok(const char *what, const double *e, int64_t n, bool positive) {
    for (int64_t j = 0; j <= n; j++) {
        if (!std::isfinite(e[j])) return fail(XB_E_ARG, "xb_nci_hist: %s edge %lld is not finite", what, (long long)j);
        if (positive && e[j] < 0.) return fail(XB_E_ARG, "xb_nci_hist: %s edge %lld is negative (%g)", what, (long long)j, e[j]);
        if (j && !(e[j - 1] < e[j])) return fail(XB_E_ARG, "xb_nci_hist: the %s edges do not increase strictly at %lld", what, (long long)j);
    }
    return XB_OK;
}

int xb_nci_hist(xb_ctx *c, const double lattice[9], const double *s_edges, int64_t n_s, const double *x_edges, int64_t n_x, int flags,
                int64_t *counts) {
    ANALYSIS_NEED_GRID("xb_nci_hist");
    if (!lattice || !s_edges || !x_edges || !counts) return fail(XB_E_ARG, "xb_nci_hist: null argument");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_nci_hist: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    if (n_s < 1 || n_x < 1) return fail(XB_E_ARG, "xb_nci_hist: %lld x %lld bins", (long long)n_s, (long long)n_x);
    if (n_s > XB_NCI_BINS_MAX || n_x > XB_NCI_BINS_MAX || n_s * n_x > XB_NCI_BINS_MAX)
        return fail(XB_E_LIMIT, "xb_nci_hist: %lld x %lld bins exceed %d", (long long)n_s, (long long)n_x, XB_NCI_BINS_MAX);
    if (int rc = nci_edges_ok("s", s_edges, n_s, true)) return rc;
    if (int rc = nci_edges_ok("x", x_edges, n_x, false)) return rc;
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_nci_hist", lattice, false, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const size_t cells = (size_t)(n_s * n_x), n_t = (size_t)n_s + 1, n_e = (size_t)n_x + 1;
    if (int rc = reserve(c, BLK_NCI, (n_t + n_e + cells) * sizeof(double))) return rc;
    std::vector<double> tab(n_t + n_e);
    for (size_t j = 0; j < n_t; j++) tab[j] = nci_threshold(s_edges[j]);
    for (size_t j = 0; j < n_e; j++) tab[n_t + j] = x_edges[j];
    double *dt = c->ptr<double>(BLK_NCI), *de = dt + n_t;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(de + n_e);
    HIPCHK(hipMemcpyAsync(dt, tab.data(), tab.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dc, 0, cells * sizeof(unsigned long long), c->stream));
    const bool lds = cells <= NCI_HIST_LDS;
    const int ns = (int)n_s, nb = (int)n_x;
    if (flags & XB_STENCIL_GATHER) {
        if (lds) k_nci_hist_gather<true><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dt, ns, de, nb, dc);
        else k_nci_hist_gather<false><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dt, ns, de, nb, dc);
    } else {
        if (lds) k_nci_hist<true><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dt, ns, de, nb, dc);
        else k_nci_hist<false><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dt, ns, de, nb, dc);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(counts, dc, cells * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (`tab` lives until here)
    return XB_OK;
}
