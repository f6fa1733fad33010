// host_stencil.h -- host side, part 14: the Laplacian and the Hessian of the density (k_stencil.h).  The three calls read the
// resident density (xb_laplacian_sum the resident labels too) of the whole grid and write neither.
//
// One block of the context (ctx_buffers.h), in 8-byte words:
//   BLK_ST   xb_laplacian_sum's results: sum[n], the sum of magnitudes [n], the counts [n] (64-bit integers)
// xb_laplacian_field with a host output writes into `stage` (N doubles on a whole grid: need_scratch) and copies from there;
// xb_stencil_points keeps nothing (two temporary buffers of m and 10 m words).

static_assert(sizeof(StCoeffs) == XB_STENCIL_COEFFS * sizeof(double), "StCoeffs is the array of xb_stencil_coeffs");

// the coefficients of the definition (include/bader_hip.h), every operation in the order written there
int xb_stencil_coeffs(const double lattice[9], int64_t nx, int64_t ny, int64_t nz, double out[XB_STENCIL_COEFFS]) {
    if (!lattice || !out) return fail(XB_E_ARG, "xb_stencil_coeffs: null argument");
    if (nx < 1 || ny < 1 || nz < 1)
        return fail(XB_E_ARG, "xb_stencil_coeffs: every axis needs >= 1 voxel (got %lld x %lld x %lld)", (long long)nx, (long long)ny, (long long)nz);
    const double n[3] = {(double)nx, (double)ny, (double)nz};
    double A[3][3], C[3][3], M[3][3], G[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[i][j] = lattice[3 * i + j] / n[i];
    for (int i = 0; i < 3; i++)
        for (int a = 0; a < 3; a++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
            C[i][a] = A[i1][a1] * A[i2][a2] - A[i1][a2] * A[i2][a1];
        }
    const double det = (A[0][0] * C[0][0] + A[0][1] * C[0][1]) + A[0][2] * C[0][2];
    if (det == 0. || !std::isfinite(det)) return fail(XB_E_ARG, "xb_stencil_coeffs: the lattice is singular (determinant %g)", det);
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < 3; i++) M[a][i] = C[i][a] / det;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G[i][j] = (M[0][i] * M[0][j] + M[1][i] * M[1][j]) + M[2][i] * M[2][j];
    static const int PI[3] = {0, 0, 1}, PJ[3] = {1, 2, 2};                                 // the terms 01, 02, 12
    static const int HA[6] = {0, 0, 0, 1, 1, 2}, HB[6] = {0, 1, 2, 1, 2, 2};               // the components xx xy xz yy yz zz
    double *t = out, *w = out + 9, *h = out + 15;
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < 3; i++) t[3 * a + i] = 0.5 * M[a][i];
    for (int i = 0; i < 3; i++) w[i] = G[i][i];
    for (int k = 0; k < 3; k++) w[3 + k] = 0.5 * G[PI[k]][PJ[k]];
    for (int c = 0; c < 6; c++) {
        const int a = HA[c], b = HB[c];
        for (int i = 0; i < 3; i++) h[6 * c + i] = M[a][i] * M[b][i];
        for (int k = 0; k < 3; k++) h[6 * c + 3 + k] = 0.25 * (M[a][PI[k]] * M[b][PJ[k]] + M[a][PJ[k]] * M[b][PI[k]]);
    }
    return XB_OK;
}

// what the three calls check alike once they have a grid and sound arguments of their own: the whole grid, a density (and
// labels), the lattice
static int stencil_ready(xb_ctx *c, const char *who, const double *lattice, bool labels, StCoeffs *K) {
    if (int rc = analysis_ready(c, who, "the stencil needs", NEED_WHOLE | NEED_RHO | (labels ? NEED_LABELS : 0))) return rc;
    return xb_stencil_coeffs(lattice, c->g.nx, c->g.ny, c->g.nz, reinterpret_cast<double *>(K));
}
static unsigned stencil_tiles(const Grid &g) {   // (at most N)
    return (unsigned)((long long)((g.nx + ST_TX - 1) / ST_TX) * ((g.ny + ST_TY - 1) / ST_TY) * ((g.nz + ST_TZ - 1) / ST_TZ));
}

int xb_laplacian_field(xb_ctx *c, const double lattice[9], int flags, double *out_host, void *out_dev) {
    ANALYSIS_NEED_GRID("xb_laplacian_field");
    if (!lattice) return fail(XB_E_ARG, "xb_laplacian_field: null argument");
    if ((out_host != nullptr) == (out_dev != nullptr)) return fail(XB_E_ARG, "xb_laplacian_field: exactly one of out_host and out_dev is wanted");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_laplacian_field: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_laplacian_field", lattice, false, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    double *dst = (double *)out_dev;
    if (out_dev) {
        uintptr_t lo, hi;
        if (int rc = io_check_dense(c, "xb_laplacian_field", out_dev, sizeof(double), &lo, &hi)) return rc;
        if (io_overlaps(lo, hi, c->rho, (size_t)c->N * 8)) return fail(XB_E_ARG, "xb_laplacian_field: the destination overlaps the resident density");
    } else {
        if (c->stage_bytes < (size_t)c->N * sizeof(double)) return fail(XB_E_STATE, "xb_laplacian_field: the scratch buffer holds no whole grid");
        stage_clobbered(*c);
        dst = (double *)c->stage;
    }
    if (flags & XB_STENCIL_GATHER) k_laplacian_field_gather<<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dst);
    else k_laplacian_field<<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, dst);
    HIPCHK(hipGetLastError());
    if (out_host) return staged_d2h(c, out_host, dst, (size_t)c->N * sizeof(double));   // (waits)
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

int xb_laplacian_sum(xb_ctx *c, const double lattice[9], int64_t n, double voxel_volume, int flags, double *sum, double *abs_sum,
                     double *volume) {
    ANALYSIS_NEED_GRID("xb_laplacian_sum");
    if (!lattice || !sum || !abs_sum || !volume) return fail(XB_E_ARG, "xb_laplacian_sum: null argument");
    if (flags & ~XB_STENCIL_GATHER) return fail(XB_E_ARG, "xb_laplacian_sum: unknown flag bits 0x%x", flags & ~XB_STENCIL_GATHER);
    if (n < 1) return fail(XB_E_ARG, "xb_laplacian_sum: %lld labels", (long long)n);
    if (n > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_laplacian_sum: %lld labels exceed %d", (long long)n, XB_INT_MAX);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_laplacian_sum", lattice, true, &K)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const Grid &g = c->g;
    const size_t want = 3 * (size_t)n;
    if (int rc = reserve(c, BLK_ST, want * sizeof(double))) return rc;
    double *ds = c->ptr<double>(BLK_ST), *dm = ds + n;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(dm + n);
    HIPCHK(hipMemsetAsync(ds, 0, want * sizeof(double), c->stream));
    const bool bins = n <= ST_BINS;
    if (flags & XB_STENCIL_GATHER) {
        if (bins) k_laplacian_sum_gather<true><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, ds, dm, dc);
        else k_laplacian_sum_gather<false><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, ds, dm, dc);
    } else {
        if (bins) k_laplacian_sum<true><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, ds, dm, dc);
        else k_laplacian_sum<false><<<stencil_tiles(g), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, (int)n, K, ds, dm, dc);
    }
    HIPCHK(hipGetLastError());
    std::vector<unsigned long long> cn(n);
    HIPCHK(hipMemcpyAsync(sum, ds, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(abs_sum, dm, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cn.data(), dc, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; i++) {
        sum[i] *= voxel_volume;
        abs_sum[i] *= voxel_volume;
        volume[i] = (double)cn[i] * voxel_volume;
    }
    return XB_OK;
}

int xb_stencil_points(xb_ctx *c, const double lattice[9], const int64_t *lin, int64_t m, double *out) {
    ANALYSIS_NEED_GRID("xb_stencil_points");
    if (m < 0) return fail(XB_E_ARG, "xb_stencil_points: %lld voxels", (long long)m);
    if (!lattice || (m > 0 && (!lin || !out))) return fail(XB_E_ARG, "xb_stencil_points: null argument");
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_stencil_points", lattice, false, &K)) return rc;
    for (int64_t i = 0; i < m; i++)
        if (lin[i] < 0 || lin[i] >= (int64_t)c->N)
            return fail(XB_E_ARG, "xb_stencil_points: index %lld (entry %lld) lies outside [0, %lld)", (long long)lin[i], (long long)i, c->N);
    if (m == 0) return XB_OK;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    DevBuf<long long> d_lin;
    DevBuf<double> d_out;
    HIPCHK(d_lin.alloc((size_t)m));
    HIPCHK(d_out.alloc((size_t)m * XB_STENCIL_POINT_VALUES));
    static_assert(sizeof(long long) == sizeof(int64_t), "lin travels as it is");
    HIPCHK(hipMemcpyAsync(d_lin.p, lin, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    k_stencil_points<<<nblocks(m), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, K, d_lin.p, (long long)m, d_out.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, d_out.p, (size_t)m * XB_STENCIL_POINT_VALUES * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
