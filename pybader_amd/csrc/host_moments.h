// host_moments.h -- host side, part 9: moments of the density per label about a centre (k_moments.h).  xb_moment_sum reads the
// resident density and labels over the owned planes and writes neither.
//
// One block of the context (BLK_M, ctx_buffers.h), in doubles:
//   [0, 112)     the head of host_cell.h: the 27 image vectors, computed exactly as the definition writes them, and the lattice
//   then         the position table of k_ms_tables, 3 * (nx + ny + nz)
//   then         the centres (3 n), the sums (10 n), the counts (n, 64-bit integers)

int xb_moment_sum(xb_ctx *c, const double lattice[9], const double *centres_cart, int64_t n, double voxel_volume, double *moments,
                  double *volume) {
    ANALYSIS_NEED_GRID("xb_moment_sum");
    if (!lattice || !centres_cart || !moments || !volume) return fail(XB_E_ARG, "xb_moment_sum: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_moment_sum: %lld labels", (long long)n);
    if (n > XB_INT_MAX / MS_TERMS) return fail(XB_E_LIMIT, "xb_moment_sum: %lld labels exceed %d", (long long)n, XB_INT_MAX / MS_TERMS);
    if (int rc = analysis_ready(c, "xb_moment_sum", "", NEED_RHO | NEED_LABELS)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const Grid &g = c->g;
    const long long own = (long long)(g.x1 - g.x0) * g.nyz;
    const size_t len = (size_t)g.nx + g.ny + g.nz;
    const size_t o_tab = CELL_HEAD, o_cen = o_tab + 3 * len, o_sum = o_cen + 3 * (size_t)n, o_cnt = o_sum + MS_TERMS * (size_t)n;
    const size_t want = o_cnt + (size_t)n;
    if (int rc = reserve(c, BLK_M, want * sizeof(double))) return rc;
    double head[CELL_HEAD];
    double *buf = c->ptr<double>(BLK_M);
    unsigned long long *dcn = reinterpret_cast<unsigned long long *>(buf + o_cnt);
    if (int rc = cell_head(c, lattice, head, buf)) return rc;
    MsImages img;
    memcpy(img.pbc, head, sizeof img.pbc);
    HIPCHK(hipMemcpyAsync(buf + o_cen, centres_cart, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(buf + o_sum, 0, (MS_TERMS + 1) * (size_t)n * sizeof(double), c->stream));
    MsGeom G;
    G.tab = buf + o_tab; G.pbc_dev = buf; G.centres = buf + o_cen;
    G.nx = g.nx; G.ny = g.ny; G.nz = g.nz; G.nyz = g.nyz;
    {
        ScopedTimer timer(c, XB_TIMER_MOMENTS);
        cell_tables(c, buf + 96, buf + o_tab);
        const unsigned blocks = nblocks((own + MS_PER_THREAD - 1) / MS_PER_THREAD);
        if (n <= MS_BINS) k_moment_sum_lds<<<blocks, TPB, 0, c->stream>>>(g, G, img, c->rho, c->labels, (int)n, buf + o_sum, dcn);
        else k_moment_sum_glb<<<blocks, TPB, 0, c->stream>>>(g, G, img, c->rho, c->labels, (int)n, buf + o_sum, dcn);
    }
    hipError_t e = hipGetLastError();
    std::vector<unsigned long long> cn(n);
    if (e == hipSuccess) e = hipMemcpyAsync(moments, buf + o_sum, MS_TERMS * (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(cn.data(), dcn, (size_t)n * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return fail(XB_E_HIP, "xb_moment_sum: %s", hipGetErrorString(e));
    for (int64_t i = 0; i < MS_TERMS * n; i++) moments[i] *= voxel_volume;
    for (int64_t i = 0; i < n; i++) volume[i] = (double)cn[i] * voxel_volume;
    return XB_OK;
}
