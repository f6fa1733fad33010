// host_voronoi.h -- host side, part 12: the Voronoi partition (k_voronoi.h).  xb_voronoi_assign writes the resident labels -- a
// label writer like xb_upload_labels, with everything that call invalidates -- and reads the resident density only for the vacuum.
//
// One block of the context (BLK_VO, ctx_buffers.h), in doubles, laid out as
// xb_moment_sum's:
//   [0, 96)      the 27 image vectors (81 used), computed here exactly as the definition writes them
//   [96, 112)    the lattice (9 used)
//   then         the position table of k_ms_tables, 3 * (nx + ny + nz)
//   then         the atoms (3 n), the two statistics words

#define VO_HEAD 112

int xb_voronoi_assign(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, double vac_tol, int flags,
                      int64_t stats[3]) {
    ANALYSIS_NEED_GRID("xb_voronoi_assign");
    if (!lattice || !atoms_cart) return fail(XB_E_ARG, "xb_voronoi_assign: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_voronoi_assign: %lld atoms", (long long)n);
    if (flags & ~XB_VORONOI_FULL_SEARCH) return fail(XB_E_ARG, "xb_voronoi_assign: unknown flag bits 0x%x", flags & ~XB_VORONOI_FULL_SEARCH);
    if (n > XB_INT_MAX / 27) return fail(XB_E_LIMIT, "xb_voronoi_assign: %lld atoms exceed %d", (long long)n, XB_INT_MAX / 27);
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(lattice[k])) return fail(XB_E_ARG, "xb_voronoi_assign: the lattice is not finite");
    for (int64_t k = 0; k < 3 * n; k++)
        if (!std::isfinite(atoms_cart[k])) return fail(XB_E_ARG, "xb_voronoi_assign: atom %lld is not finite", (long long)(k / 3));
    if (int rc = analysis_ready(c, "xb_voronoi_assign", "the partition needs", NEED_WHOLE)) return rc;
    const Grid &g = c->g;
    const bool use_vac = vac_tol == vac_tol;
    if (use_vac && !c->have_rho) return fail(XB_E_STATE, "xb_voronoi_assign: a vacuum tolerance, and no density on this grid yet");
    HIPCHK(hipSetDevice(c->device));
    const size_t len = (size_t)g.nx + g.ny + g.nz;
    const size_t o_tab = VO_HEAD, o_at = o_tab + 3 * len, o_st = o_at + 3 * (size_t)n, want = o_st + 1;
    if (int rc = reserve(c, BLK_VO, want * sizeof(double))) return rc;
    // every label of the grid is overwritten (vac_by_tol falls: the other labels are atoms, not the zeros an assignment expects next to its vacuum marks)
    labels_overwritten(*c, label_wire_for(n), use_vac);
    double head[VO_HEAD] = {0.};
    VoGeom G;
    for (int x = -1; x < 2; x++)
        for (int y = -1; y < 2; y++)
            for (int z = -1; z < 2; z++)
                for (int j = 0; j < 3; j++)
                    head[3 * ((x + 1) * 9 + (y + 1) * 3 + (z + 1)) + j] = (lattice[j] * (double)x + lattice[3 + j] * (double)y) + lattice[6 + j] * (double)z;
    G.len = 0.;
    for (int k = 0; k < 3; k++) G.len += std::sqrt((lattice[3 * k] * lattice[3 * k] + lattice[3 * k + 1] * lattice[3 * k + 1]) + lattice[3 * k + 2] * lattice[3 * k + 2]);
    for (int k = 0; k < 9; k++) G.lat[k] = head[96 + k] = lattice[k];
    double *buf = c->ptr<double>(BLK_VO);
    unsigned int *dst = reinterpret_cast<unsigned int *>(buf + o_st);
    G.tab = buf + o_tab; G.pbc = buf; G.atoms = buf + o_at;
    G.nx = g.nx; G.ny = g.ny; G.nz = g.nz; G.n = (int)n;
    G.ntx = (g.nx + VO_TILE - 1) / VO_TILE; G.nty = (g.ny + VO_TILE - 1) / VO_TILE; G.ntz = (g.nz + VO_TILE - 1) / VO_TILE;
    const long long tiles = (long long)G.ntx * G.nty * G.ntz;   // (at most N: fits the launch grid)
    const int forced = (flags & XB_VORONOI_FULL_SEARCH) != 0;
    HIPCHK(hipMemcpyAsync(buf, head, sizeof head, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(buf + o_at, atoms_cart, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(double), c->stream));
    k_ms_tables<<<nblocks(3 * (long long)len), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, buf + 96, buf + o_tab);
    k_voronoi<<<(unsigned)tiles, 256, 0, c->stream>>>(G, c->rho, use_vac ? 1 : 0, vac_tol, forced, c->labels, dst);
    hipError_t e = hipGetLastError();
    unsigned int st[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(st, dst, sizeof st, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host arrays may go, the statistics are here)
    if (e != hipSuccess) return fail(XB_E_HIP, "xb_voronoi_assign: %s", hipGetErrorString(e));
    if (stats) {
        const long long full = forced ? tiles : (long long)st[0];
        stats[0] = tiles - full;
        stats[1] = full;
        stats[2] = st[1];
    }
    return XB_OK;
}
