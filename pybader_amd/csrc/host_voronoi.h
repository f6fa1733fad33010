// host_voronoi.h -- host side, part 12: the Voronoi partition (k_voronoi.h).  xb_voronoi_assign writes the resident labels -- a
// label writer like xb_upload_labels, with everything that call invalidates -- and reads the resident density only for the vacuum.
//
// One block of the context (BLK_VO, ctx_buffers.h), in doubles:
//   [0, 112)     the head of host_cell.h: the 27 image vectors, computed exactly as the definition writes them, and the lattice
//   then         the position table of k_ms_tables, 3 * (nx + ny + nz)
//   then         the atoms (3 n), the two statistics words

int xb_voronoi_assign(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, double vac_tol, int flags,
                      int64_t stats[3]) {
    ANALYSIS_NEED_GRID("xb_voronoi_assign");
    if (!lattice || !atoms_cart) return fail(XB_E_ARG, "xb_voronoi_assign: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_voronoi_assign: %lld atoms", (long long)n);
    if (flags & ~XB_VORONOI_FULL_SEARCH) return fail(XB_E_ARG, "xb_voronoi_assign: unknown flag bits 0x%x", flags & ~XB_VORONOI_FULL_SEARCH);
    if (n > XB_INT_MAX / 27) return fail(XB_E_LIMIT, "xb_voronoi_assign: %lld atoms exceed %d", (long long)n, XB_INT_MAX / 27);
    if (int rc = cell_check("xb_voronoi_assign", lattice, atoms_cart, n)) return rc;
    if (int rc = analysis_ready(c, "xb_voronoi_assign", "the partition needs", NEED_WHOLE)) return rc;
    const Grid &g = c->g;
    const bool use_vac = vac_tol == vac_tol;
    if (use_vac && !c->have_rho) return fail(XB_E_STATE, "xb_voronoi_assign: a vacuum tolerance, and no density on this grid yet");
    HIPCHK(hipSetDevice(c->device));
    const size_t len = (size_t)g.nx + g.ny + g.nz;
    const size_t o_tab = CELL_HEAD, o_at = o_tab + 3 * len, o_st = o_at + 3 * (size_t)n, want = o_st + 1;
    if (int rc = reserve(c, BLK_VO, want * sizeof(double))) return rc;
    // every label of the grid is overwritten (vac_by_tol falls: the other labels are atoms, not the zeros an assignment expects next to its vacuum marks)
    labels_overwritten(*c, label_wire_for(n), use_vac);
    double head[CELL_HEAD];
    double *buf = c->ptr<double>(BLK_VO);
    unsigned int *dst = reinterpret_cast<unsigned int *>(buf + o_st);
    VoGeom G;
    cell_geom(G, g, lattice, VO_TILE, buf + o_tab);
    G.pbc = buf; G.atoms = buf + o_at; G.n = (int)n;
    const long long tiles = (long long)G.ntx * G.nty * G.ntz;   // (at most N: fits the launch grid)
    const int forced = (flags & XB_VORONOI_FULL_SEARCH) != 0;
    if (int rc = cell_head(c, lattice, head, buf)) return rc;
    HIPCHK(hipMemcpyAsync(buf + o_at, atoms_cart, 3 * (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(dst, 0, sizeof(double), c->stream));
    cell_tables(c, buf + 96, buf + o_tab);
    k_voronoi<<<(unsigned)tiles, 256, 0, c->stream>>>(G, c->rho, use_vac ? 1 : 0, vac_tol, forced, c->labels, dst);
    hipError_t e = hipGetLastError();
    unsigned int st[2] = {0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(st, dst, sizeof st, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);   // (the host arrays may go, the statistics are here)
    if (e != hipSuccess) return fail(XB_E_HIP, "xb_voronoi_assign: %s", hipGetErrorString(e));
    tile_route_stats(stats, tiles, forced, st);
    return XB_OK;
}
