// host_dori.h -- host side, part 17: DORI, the density overlap regions indicator (k_dori.h).  The two calls read the resident
// density (xb_dori_sum the resident labels too) of the whole grid and write neither.
//
// xb_dori_sum uses the NCI sums' block of the context (ctx_buffers.h), in 8-byte words:
//   BLK_NCI   sum of rho [3 n], sum of rho^2 [3 n], counts [3 n] (64-bit integers)
// xb_dori_field with host outputs writes gamma into `stage` (N doubles on a whole grid: need_scratch) and x, when it is asked for,
// into a temporary buffer of N doubles, and copies from there.

int xb_dori_field(xb_ctx *c, const double lattice[9], double rho_min, int flags, double *g_host, double *x_host, void *g_dev, void *x_dev) {
    ANALYSIS_NEED_GRID("xb_dori_field");
    if (!lattice) return fail(XB_E_ARG, "xb_dori_field: null argument");
    const bool host = g_host && !g_dev && !x_dev, dev = g_dev && !g_host && !x_host;
    if (!host && !dev)
        return fail(XB_E_ARG, "xb_dori_field: gamma is wanted on the host or on the device, and x (optional) on the same side");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_dori_field: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    if (!std::isfinite(rho_min) || rho_min < 0.) return fail(XB_E_ARG, "xb_dori_field: rho_min (%g) must be finite and not negative", rho_min);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_dori_field", lattice, false, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const size_t bytes = (size_t)c->N * sizeof(double);
    double *dg = (double *)g_dev, *dx = (double *)x_dev;
    DevBuf<double> tmp;
    if (dev) {
        uintptr_t lo[2] = {0, 0}, hi[2] = {0, 0};
        void *const out[2] = {g_dev, x_dev};
        for (int k = 0; k < 2; k++) {
            if (!out[k]) continue;
            if (int rc = io_check_dense(c, "xb_dori_field", out[k], sizeof(double), &lo[k], &hi[k])) return rc;
            if (io_overlaps(lo[k], hi[k], c->rho, bytes)) return fail(XB_E_ARG, "xb_dori_field: a destination overlaps the resident density");
        }
        if (x_dev && lo[0] < hi[1] && lo[1] < hi[0]) return fail(XB_E_ARG, "xb_dori_field: the two destinations overlap");
    } else {
        if (c->stage_bytes < bytes) return fail(XB_E_STATE, "xb_dori_field: the scratch buffer holds no whole grid");
        if (x_host) HIPCHK(tmp.alloc((size_t)c->N));
        stage_clobbered(*c);
        dg = (double *)c->stage;
        dx = x_host ? tmp.p : nullptr;
    }
    if (flags & XB_STENCIL_GATHER) k_dori_field_gather<<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, rho_min, dg, dx);
    else k_dori_field<<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, rho_min, dg, dx);
    HIPCHK(hipGetLastError());
    if (host) {
        if (int rc = staged_d2h(c, g_host, dg, bytes)) return rc;   // (waits)
        return x_host ? staged_d2h(c, x_host, dx, bytes) : XB_OK;
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

int xb_dori_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, double d_cut, double rho_min, double rho_split,
                int flags, int64_t *count, double *charge, double *charge2) {
    ANALYSIS_NEED_GRID("xb_dori_sum");
    if (!lattice || !count || !charge || !charge2) return fail(XB_E_ARG, "xb_dori_sum: null argument");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_dori_sum: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    if (n < 1) return fail(XB_E_ARG, "xb_dori_sum: %lld labels", (long long)n);
    if (!std::isfinite(rho_min) || !std::isfinite(rho_split) || rho_min < 0. || rho_split < 0.)
        return fail(XB_E_ARG, "xb_dori_sum: the thresholds (%g, %g) must be finite and not negative", rho_min, rho_split);
    if (!(d_cut > 0. && d_cut <= 1.)) return fail(XB_E_ARG, "xb_dori_sum: d_cut (%g) must lie in (0, 1]", d_cut);
    if (n > XB_INT_MAX / 3) return fail(XB_E_LIMIT, "xb_dori_sum: %lld labels exceed %d", (long long)n, XB_INT_MAX / 3);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_dori_sum", lattice, true, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const Grid &g = c->g;
    const size_t keys = 3 * (size_t)n, want = 3 * keys;
    if (int rc = reserve(c, BLK_NCI, want * sizeof(double))) return rc;
    double *ds = c->ptr<double>(BLK_NCI), *dq = ds + keys;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(dq + keys);
    HIPCHK(hipMemsetAsync(ds, 0, want * sizeof(double), c->stream));
    const DoriCuts C{d_cut, rho_min, rho_split};
    const bool bins = n <= NCI_LABELS_LDS;
    if (flags & XB_STENCIL_GATHER) {
        if (bins) k_dori_sum_gather<true><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
        else k_dori_sum_gather<false><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
    } else {
        if (bins) k_dori_sum<true><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
        else k_dori_sum<false><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, C, ds, dq, dc);
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
