// host_moments.h -- host side, part 9: moments of the density per label about a centre (k_moments.h).  xb_moment_sum reads the
// resident density and labels over the owned planes and writes neither.
//
// One block of the context (BLK_M, ctx_buffers.h), in doubles:
//   [0, 96)      the 27 image vectors (81 used), computed here exactly as the definition writes them
//   [96, 112)    the lattice (9 used)
//   then         the position table of k_ms_tables, 3 * (nx + ny + nz)
//   then         the centres (3 n), the sums (10 n), the counts (n, 64-bit integers)

#define MS_HEAD 112

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
    const size_t o_tab = MS_HEAD, o_cen = o_tab + 3 * len, o_sum = o_cen + 3 * (size_t)n, o_cnt = o_sum + MS_TERMS * (size_t)n;
    const size_t want = o_cnt + (size_t)n;
    if (int rc = reserve(c, BLK_M, want * sizeof(double))) return rc;
    double head[MS_HEAD] = {0.};
    MsImages img;
    for (int x = -1; x < 2; x++)
        for (int y = -1; y < 2; y++)
            for (int z = -1; z < 2; z++)
                for (int j = 0; j < 3; j++) {
                    const int i = (x + 1) * 9 + (y + 1) * 3 + (z + 1);
                    img.pbc[i][j] = (lattice[j] * (double)x + lattice[3 + j] * (double)y) + lattice[6 + j] * (double)z;
                    head[3 * i + j] = img.pbc[i][j];
                }
    for (int k = 0; k < 9; k++) head[96 + k] = lattice[k];
    double *buf = c->ptr<double>(BLK_M);
    unsigned long long *dcn = reinterpret_cast<unsigned long long *>(buf + o_cnt);
    HIPCHK(hipMemcpyAsync(buf, head, sizeof head, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(buf + o_cen, centres_cart, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(buf + o_sum, 0, (MS_TERMS + 1) * (size_t)n * sizeof(double), c->stream));
    MsGeom G;
    G.tab = buf + o_tab; G.pbc_dev = buf; G.centres = buf + o_cen;
    G.nx = g.nx; G.ny = g.ny; G.nz = g.nz; G.nyz = g.nyz;
    {
        ScopedTimer timer(c, XB_TIMER_MOMENTS);
        k_ms_tables<<<nblocks(3 * (long long)len), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, buf + 96, buf + o_tab);
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
