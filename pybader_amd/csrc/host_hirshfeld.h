// host_hirshfeld.h -- host side, part 15: Hirshfeld (stockholder) charges, the promolecular and the deformation density
// (k_hirshfeld.h).  xb_hirshfeld_setup puts everything that belongs to the grid's shape, the cell, the atoms and the pro-atom
// tables on the device; xb_hirshfeld_sum and xb_hirshfeld_field read the resident density and write nothing resident.
//
// One block of the context (BLK_HS, ctx_buffers.h; xb_hirshfeld_release frees it), in doubles:
//   [0, 16)      the lattice (9 used)
//   then         the position table of k_ms_tables, 3 * (nx + ny + nz)
//   then         per species r_cut, rc2, inv_h2 (3 S)
//   then         per species K pairs (f[k], f[k+1] - f[k]) (2 S K; starts at an even word: 16-byte loads)
//   then         the image list, 4 words per image (q[3], then atom and species as two ints)
//   then         the results: charge[n], volume[n], the rest's density sum, its voxel count (64-bit), the two statistics words
//   then         only in an ISA setup (host_isa.h), from the next even word: the second table area, counts, bins, qsum rows, a counter
//   or           only in an MBIS setup (host_mbis.h), from the next even word: the exp table, two parameter areas, counts, bins, rows
// The setup is valid for the shape it was made on (hs_geom records it): xb_set_grid drops it when the shape changes, free_grid with the
// buffer.  Nothing else the context holds enters it -- not the density, not the labels, not dist_mat.

#define HS_HEAD 16

static void hirshfeld_forget(xb_ctx *c) { c->hs_have = false; c->hs_isa = false; c->hs_mbis = false; c->sm_cmax = -1; }

// the inverse of the lattice by cofactors, in the order section 18 writes them (A = the lattice itself); false: det is 0 or not finite
static bool hs_inverse(const double *lat, double M[3][3]) {
    double C[3][3];
    for (int i = 0; i < 3; i++)
        for (int a = 0; a < 3; a++) {
            const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, a1 = (a + 1) % 3, a2 = (a + 2) % 3;
            C[i][a] = lat[3 * i1 + a1] * lat[3 * i2 + a2] - lat[3 * i1 + a2] * lat[3 * i2 + a1];
        }
    const double det = (lat[0] * C[0][0] + lat[1] * C[0][1]) + lat[2] * C[0][2];
    if (det == 0. || !std::isfinite(det)) return false;
    for (int a = 0; a < 3; a++)
        for (int i = 0; i < 3; i++) M[a][i] = C[i][a] / det;
    return true;
}

// what the list needs checked; the ranges lo[a][i] .. hi[a][i] and the list's length
static int hs_ranges(const char *who, const double *lattice, const double *atoms, const int32_t *species, int64_t n, const double *r_cut,
                     int64_t S, std::vector<int> &lo, std::vector<int> &hi, int64_t *count) {
    if (!lattice || !atoms || !species || !r_cut) return fail(XB_E_ARG, "%s: null argument", who);
    if (n < 1) return fail(XB_E_ARG, "%s: %lld atoms", who, (long long)n);
    if (S < 1) return fail(XB_E_ARG, "%s: %lld species", who, (long long)S);
    if (n > XB_INT_MAX) return fail(XB_E_LIMIT, "%s: %lld atoms exceed %d", who, (long long)n, XB_INT_MAX);
    if (int rc = cell_check(who, lattice, atoms, n)) return rc;
    for (int64_t a = 0; a < n; a++)
        if (species[a] < 0 || species[a] >= S) return fail(XB_E_ARG, "%s: atom %lld has species %d, outside [0, %lld)", who, (long long)a, species[a], (long long)S);
    for (int64_t s = 0; s < S; s++)
        if (!std::isfinite(r_cut[s]) || !(r_cut[s] > 0.)) return fail(XB_E_ARG, "%s: r_cut[%lld] = %g is not a positive finite number", who, (long long)s, r_cut[s]);
    double M[3][3];
    if (!hs_inverse(lattice, M)) return fail(XB_E_ARG, "%s: the lattice is singular", who);
    // Axis i: a voxel has the fractional coordinate g in [0, 1), the image x of atom a the coordinate f + x, and the two lie at
    // least |f + x - g| h_i apart (h_i the cell's height along i, 1 / h_i = the length of column i of M).  So only shifts with
    // -rho < f + x < 1 + rho, rho = r_cut / h_i, can reach a voxel.  MARGIN: f and rho are formed from M, whose entries carry a
    // relative error of a few u times the condition number of the cell; 2^-20 (1 + |f| + rho) covers every cell with a condition
    // number below 2^30, and floor / ceil then widen the range to whole shifts.  A wider range adds zero terms only.
    lo.resize(3 * (size_t)n); hi.resize(3 * (size_t)n);
    long double total = 0;
    for (int64_t a = 0; a < n; a++) {
        long double per = 1;
        for (int i = 0; i < 3; i++) {
            const double f = (atoms[3 * a] * M[0][i] + atoms[3 * a + 1] * M[1][i]) + atoms[3 * a + 2] * M[2][i];
            const double g = std::sqrt((M[0][i] * M[0][i] + M[1][i] * M[1][i]) + M[2][i] * M[2][i]);
            const double rho = r_cut[species[a]] * g;
            const double m = 0x1p-20 * ((1. + std::fabs(f)) + rho);
            const double l = std::floor((-rho - f) - m), h = std::ceil(((1. + rho) - f) + m);
            if (!(std::fabs(l) < 0x1p30) || !(std::fabs(h) < 0x1p30))
                return fail(XB_E_LIMIT, "%s: atom %lld needs shifts %g .. %g along axis %d", who, (long long)a, l, h, i);
            lo[3 * a + i] = (int)l; hi[3 * a + i] = (int)h;
            per *= (long double)(h - l + 1.);
        }
        total += per;
    }
    if (total > (long double)XB_INT_MAX) return fail(XB_E_LIMIT, "%s: %.0Lf images exceed %d", who, total, XB_INT_MAX);
    *count = (int64_t)total;
    return XB_OK;
}

int xb_hirshfeld_images(const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n, const double *r_cut,
                        int64_t n_species, int64_t *out_count, int32_t *out_images, int64_t capacity) {
    if (!out_count) return fail(XB_E_ARG, "xb_hirshfeld_images: null argument");
    std::vector<int> lo, hi;
    int64_t count = 0;
    if (int rc = hs_ranges("xb_hirshfeld_images", lattice, atoms_cart, species, n, r_cut, n_species, lo, hi, &count)) return rc;
    *out_count = count;
    if (!out_images) return XB_OK;
    if (capacity < count) return fail(XB_E_ARG, "xb_hirshfeld_images: capacity %lld below the %lld images", (long long)capacity, (long long)count);
    int32_t *o = out_images;
    for (int64_t a = 0; a < n; a++)
        for (int x = lo[3 * a]; x <= hi[3 * a]; x++)
            for (int y = lo[3 * a + 1]; y <= hi[3 * a + 1]; y++)
                for (int z = lo[3 * a + 2]; z <= hi[3 * a + 2]; z++) { o[0] = (int32_t)a; o[1] = x; o[2] = y; o[3] = z; o += 4; }
    return XB_OK;
}

static int hs_build(xb_ctx *c, const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n, const double *r_cut,
                    int64_t S, int64_t K, const std::vector<int> &lo, const std::vector<int> &hi, int64_t count, size_t extra,
                    size_t *o_extra, const std::vector<double> &pairs);

int xb_hirshfeld_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n,
                       const double *tables, const double *r_cut, int64_t n_species, int64_t knots) {
    if (!c) return fail(XB_E_ARG, "xb_hirshfeld_setup: null ctx");
    if (int rc = analysis_ready(c, "xb_hirshfeld_setup", "the weights need", NEED_WHOLE)) return rc;
    if (!tables) return fail(XB_E_ARG, "xb_hirshfeld_setup: null argument");
    if (knots < 1) return fail(XB_E_ARG, "xb_hirshfeld_setup: %lld knots", (long long)knots);
    std::vector<int> lo, hi;
    int64_t count = 0;
    if (int rc = hs_ranges("xb_hirshfeld_setup", lattice, atoms_cart, species, n, r_cut, n_species, lo, hi, &count)) return rc;
    const int64_t S = n_species, K = knots;
    if (K > (1 << 26) || S > (1 << 26) / K) return fail(XB_E_LIMIT, "xb_hirshfeld_setup: %lld species of %lld knots exceed 2^26 table entries", (long long)S, (long long)K);
    for (int64_t s = 0; s < S; s++) {
        const double *f = tables + s * (K + 1);
        for (int64_t k = 0; k <= K; k++)
            if (!std::isfinite(f[k]) || f[k] < 0.) return fail(XB_E_ARG, "xb_hirshfeld_setup: table %lld holds %g at knot %lld", (long long)s, f[k], (long long)k);
        if (f[K] != 0.) return fail(XB_E_ARG, "xb_hirshfeld_setup: table %lld ends with %g, not with 0", (long long)s, f[K]);
    }
    std::vector<double> pairs(2 * (size_t)S * K);
    for (int64_t s = 0; s < S; s++) {
        const double *f = tables + s * (K + 1);
        for (int64_t k = 0; k < K; k++) {
            pairs[2 * (s * K + k)] = f[k];
            pairs[2 * (s * K + k) + 1] = f[k + 1] - f[k];
        }
    }
    return hs_build(c, lattice, atoms_cart, species, n, r_cut, S, K, lo, hi, count, 0, nullptr, pairs);
}

// the checked arguments become the setup: the block is sized (`extra` more doubles behind the results, from the even word
// *o_extra on: xb_isa_setup's), filled and its geometry recorded.  pairs: per species the K table pairs
static int hs_build(xb_ctx *c, const double lattice[9], const double *atoms_cart, const int32_t *species, int64_t n, const double *r_cut,
                    int64_t S, int64_t K, const std::vector<int> &lo, const std::vector<int> &hi, int64_t count, size_t extra,
                    size_t *o_extra, const std::vector<double> &pairs) {
    const Grid &g = c->g;
    HIPCHK(hipSetDevice(c->device));
    hirshfeld_forget(c);   // (whatever fails from here on leaves no setup behind)
    HIPCHK(hipDeviceGetAttribute(&c->hs_cus, hipDeviceAttributeMultiprocessorCount, c->device));
    const size_t len = (size_t)g.nx + g.ny + g.nz;
    size_t o_tab = HS_HEAD, o_sp = o_tab + 3 * len, o_pairs = o_sp + 3 * (size_t)S;
    o_pairs += o_pairs & 1;
    const size_t o_img = o_pairs + 2 * (size_t)S * K, o_acc = o_img + 4 * (size_t)count;
    size_t want = o_acc + 2 * (size_t)n + 3;
    if (extra) {
        want += want & 1;
        *o_extra = want;
        want += extra;
    }
    if (int rc = reserve(c, BLK_HS, want * sizeof(double))) return rc;
    // the host image of everything but the position table and the results
    std::vector<double> host(o_acc, 0.);
    for (int k = 0; k < 9; k++) host[k] = lattice[k];
    for (int64_t s = 0; s < S; s++) {
        const double rc2 = r_cut[s] * r_cut[s];
        host[o_sp + 3 * s] = r_cut[s]; host[o_sp + 3 * s + 1] = rc2; host[o_sp + 3 * s + 2] = (double)K / rc2;
    }
    std::copy(pairs.begin(), pairs.end(), host.begin() + o_pairs);
    static_assert(sizeof(HsImage) == 4 * sizeof(double), "an image is four words of the buffer");
    HsImage *im = reinterpret_cast<HsImage *>(host.data() + o_img);
    for (int64_t a = 0; a < n; a++)
        for (int x = lo[3 * a]; x <= hi[3 * a]; x++)
            for (int y = lo[3 * a + 1]; y <= hi[3 * a + 1]; y++)
                for (int z = lo[3 * a + 2]; z <= hi[3 * a + 2]; z++, im++) {
                    for (int j = 0; j < 3; j++) im->q[j] = atoms_cart[3 * a + j] + cell_shift(lattice, x, y, z, j);
                    im->a = (int)a; im->s = species[a];
                }
    double *buf = c->ptr<double>(BLK_HS);
    HIPCHK(hipMemcpyAsync(buf, host.data(), HS_HEAD * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(buf + o_sp, host.data() + o_sp, (o_acc - o_sp) * sizeof(double), hipMemcpyHostToDevice, c->stream));
    cell_tables(c, buf, buf + o_tab);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));   // (`host` goes)
    HsGeom &G = c->hs_geom;
    cell_geom(G, g, lattice, HS_TILE, buf + o_tab);
    G.img = reinterpret_cast<const HsImage *>(buf + o_img); G.sp = buf + o_sp;
    G.pairs = reinterpret_cast<const double2 *>(buf + o_pairs);
    G.n_img = (unsigned int)count; G.K = (int)K;
    c->hs_n = n; c->hs_acc = o_acc;
    c->sm_rmax = *std::max_element(r_cut, r_cut + S);   // (xb_stockholder_moments' exponents)
    c->hs_have = true;
    return XB_OK;
}

// what the two calls check alike: a grid, the whole of it, a setup made on its shape
static int hirshfeld_ready(xb_ctx *c, const char *who) {
    if (!c) return fail(XB_E_ARG, "%s: null ctx", who);
    if (int rc = analysis_ready(c, who, "the weights need", NEED_WHOLE)) return rc;
    const Grid &g = c->g;
    if (!c->hs_have || c->hs_geom.nx != g.nx || c->hs_geom.ny != g.ny || c->hs_geom.nz != g.nz)
        return fail(XB_E_STATE, "%s: no xb_hirshfeld_setup for this grid's shape", who);
    return XB_OK;
}
static long long hirshfeld_tiles(const HsGeom &G) { return (long long)G.ntx * G.nty * G.ntz; }   // (at most N: fits an int and the launch grid)
// the sums' launch: HS_ROUNDS times the workgroups the device holds at once (HS_SUM_WAVES per compute unit), which the dispatcher
// deals out as others end; never more than one per tile
static unsigned hirshfeld_groups(const xb_ctx *c) {
    return (unsigned)std::min<long long>(hirshfeld_tiles(c->hs_geom), (long long)HS_ROUNDS * HS_SUM_WAVES * std::max(c->hs_cus, 1));
}

int xb_hirshfeld_sum(xb_ctx *c, double voxel_volume, int flags, double *charge, double *volume, double rest[2], int64_t stats[3]) {
    if (int rc = hirshfeld_ready(c, "xb_hirshfeld_sum")) return rc;
    if (c->hs_mbis) return fail(XB_E_STATE, "xb_hirshfeld_sum: the setup of this grid is xb_mbis_setup's: its pro-atoms are no radial tables");
    if (!charge || !volume || !rest) return fail(XB_E_ARG, "xb_hirshfeld_sum: null argument");
    if (flags & ~XB_HIRSHFELD_FULL_SEARCH) return fail(XB_E_ARG, "xb_hirshfeld_sum: unknown flag bits 0x%x", flags & ~XB_HIRSHFELD_FULL_SEARCH);
    if (int rc = analysis_ready(c, "xb_hirshfeld_sum", "", NEED_RHO)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const HsGeom &G = c->hs_geom;
    const size_t n = (size_t)c->hs_n;
    double *acc = c->ptr<double>(BLK_HS) + c->hs_acc;
    unsigned long long *restn = reinterpret_cast<unsigned long long *>(acc + 2 * n + 1);
    unsigned int *dst = reinterpret_cast<unsigned int *>(acc + 2 * n + 2);
    const long long tiles = hirshfeld_tiles(G);
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    HIPCHK(hipMemsetAsync(acc, 0, (2 * n + 3) * sizeof(double), c->stream));
    k_hirshfeld<HS_SUM><<<hirshfeld_groups(c), 256, 0, c->stream>>>(G, c->rho, forced, (int)n, acc, restn, nullptr, dst);
    HIPCHK(hipGetLastError());
    std::vector<double> res(2 * n + 3);
    HIPCHK(hipMemcpyAsync(res.data(), acc, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t a = 0; a < n; a++) {
        charge[a] = res[a] * voxel_volume;
        volume[a] = res[n + a] * voxel_volume;
    }
    unsigned long long cn;
    unsigned int st[2];
    memcpy(&cn, &res[2 * n + 1], sizeof cn);
    memcpy(st, &res[2 * n + 2], sizeof st);
    rest[0] = res[2 * n] * voxel_volume;
    rest[1] = (double)cn * voxel_volume;
    tile_route_stats(stats, tiles, forced, st);
    return XB_OK;
}

int xb_hirshfeld_field(xb_ctx *c, int mode, int flags, double *out_host, void *out_dev) {
    if (int rc = hirshfeld_ready(c, "xb_hirshfeld_field")) return rc;
    if (c->hs_mbis) return fail(XB_E_STATE, "xb_hirshfeld_field: the setup of this grid is xb_mbis_setup's: its pro-atoms are no radial tables");
    if (mode != XB_HIRSHFELD_PROMOLECULE && mode != XB_HIRSHFELD_DEFORMATION) return fail(XB_E_ARG, "xb_hirshfeld_field: unknown mode %d", mode);
    if ((out_host != nullptr) == (out_dev != nullptr)) return fail(XB_E_ARG, "xb_hirshfeld_field: exactly one of out_host and out_dev is wanted");
    if (flags & ~XB_HIRSHFELD_FULL_SEARCH) return fail(XB_E_ARG, "xb_hirshfeld_field: unknown flag bits 0x%x", flags & ~XB_HIRSHFELD_FULL_SEARCH);
    if (mode == XB_HIRSHFELD_DEFORMATION && !c->have_rho) return fail(XB_E_STATE, "xb_hirshfeld_field: no density on this grid yet");
    HIPCHK(hipSetDevice(c->device));
    double *dst = (double *)out_dev;
    if (out_dev) {
        uintptr_t lo, hi;
        if (int rc = io_check_dense(c, "xb_hirshfeld_field", out_dev, sizeof(double), &lo, &hi)) return rc;
        if (io_overlaps(lo, hi, c->rho, (size_t)c->N * 8)) return fail(XB_E_ARG, "xb_hirshfeld_field: the destination overlaps the resident density");
        if (io_overlaps(lo, hi, c->ptr<void>(BLK_HS), c->bytes(BLK_HS))) return fail(XB_E_ARG, "xb_hirshfeld_field: the destination overlaps the setup");
    } else {
        if (c->stage_bytes < (size_t)c->N * sizeof(double)) return fail(XB_E_STATE, "xb_hirshfeld_field: the scratch buffer holds no whole grid");
        stage_clobbered(*c);
        dst = (double *)c->stage;
    }
    const HsGeom &G = c->hs_geom;
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    unsigned int *st = reinterpret_cast<unsigned int *>(c->ptr<double>(BLK_HS) + c->hs_acc + 2 * (size_t)c->hs_n + 2);
    if (mode == XB_HIRSHFELD_PROMOLECULE) k_hirshfeld<HS_PRO><<<(unsigned)hirshfeld_tiles(G), 256, 0, c->stream>>>(G, c->rho, forced, 0, nullptr, nullptr, dst, st);
    else k_hirshfeld<HS_DEF><<<(unsigned)hirshfeld_tiles(G), 256, 0, c->stream>>>(G, c->rho, forced, 0, nullptr, nullptr, dst, st);
    HIPCHK(hipGetLastError());
    if (out_host) return staged_d2h(c, out_host, dst, (size_t)c->N * sizeof(double));   // (waits)
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
