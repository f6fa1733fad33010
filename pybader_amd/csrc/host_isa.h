// host_isa.h -- host side, part 15b: iterative stockholder atoms (k_isa.h).  An ISA setup IS a Hirshfeld setup of the context
// (host_hirshfeld.h) with one table per atom, species[a] = a, whose pairs are (A[a][k], +0.0); hs_isa marks it.  xb_hirshfeld_sum,
// xb_hirshfeld_field and xb_hirshfeld_release serve it unchanged; an xb_hirshfeld_setup replaces it and the reverse.
//
// What the iteration needs lies in the same block (BLK_HS), behind the results, from the even double isa_x on:
//   the second table area, 2 n K doubles (the first is the setup's own; hs_geom.pairs points to the current one)
//   count[n][K], bin[n][K]  int64
//   qsum[XB_ISA_ITERS_MAX][n]  int64, a row per iteration of one call
//   one word: the voxels beyond rho_bound
// The two statistics words of the Hirshfeld results (tiles that overflowed, the longest list) serve the shell pass too.

static int isa_ceil_log2(double x) {   // x > 0 finite: the least c with x <= 2^c, by frexp
    int ex;
    const double m = std::frexp(x, &ex);   // x = m 2^ex, 0.5 <= m < 1
    return m == 0.5 ? ex - 1 : ex;
}
static int isa_ceil_log2(unsigned long long v) {   // v >= 1
    int c = 0;
    while (c < 64 && (1ull << c) < v) c++;
    return c;
}

struct IsaAreas { double2 *pairs[2]; long long *count, *bins; unsigned long long *qsum, *viol; unsigned int *stats; };
static IsaAreas isa_areas(const xb_ctx *c) {
    double *buf = c->ptr<double>(BLK_HS);
    const size_t n = (size_t)c->hs_n, nk = n * (size_t)c->hs_geom.K;
    IsaAreas a;
    a.pairs[0] = reinterpret_cast<double2 *>(buf + c->isa_pairs0);
    a.pairs[1] = reinterpret_cast<double2 *>(buf + c->isa_x);
    a.count = reinterpret_cast<long long *>(buf + c->isa_x + 2 * nk);
    a.bins = a.count + nk;
    a.qsum = reinterpret_cast<unsigned long long *>(a.bins + nk);
    a.viol = a.qsum + (size_t)XB_ISA_ITERS_MAX * n;
    a.stats = reinterpret_cast<unsigned int *>(buf + c->hs_acc + 2 * n + 2);
    return a;
}

int xb_isa_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, const double *r_cut, int64_t shells,
                 const double *initial, double rho_bound, int64_t out_info[4]) {
    if (!c) return fail(XB_E_ARG, "xb_isa_setup: null ctx");
    if (int rc = analysis_ready(c, "xb_isa_setup", "the weights need", NEED_WHOLE)) return rc;
    if (!out_info) return fail(XB_E_ARG, "xb_isa_setup: null argument");
    if (shells < 1) return fail(XB_E_ARG, "xb_isa_setup: %lld shells", (long long)shells);
    if (!std::isfinite(rho_bound) || !(rho_bound > 0.)) return fail(XB_E_ARG, "xb_isa_setup: rho_bound = %g is not a positive finite number", rho_bound);
    const int64_t K = shells;
    // (before anything is sized by n; an n below 1 passes here and is hs_ranges' to refuse)
    if (K > (1 << 26) || n > (1 << 26) / K) return fail(XB_E_LIMIT, "xb_isa_setup: %lld atoms of %lld shells exceed 2^26 table entries", (long long)n, (long long)K);
    std::vector<int32_t> species(n >= 1 ? (size_t)n : 1);   // (at most 2^26; hs_ranges refuses n < 1 before it reads them)
    for (size_t a = 0; a < species.size(); a++) species[a] = (int32_t)a;
    std::vector<int> lo, hi;
    int64_t count = 0;
    if (int rc = hs_ranges("xb_isa_setup", lattice, atoms_cart, species.data(), n, r_cut, n, lo, hi, &count)) return rc;
    if (initial)
        for (int64_t k = 0; k < n * K; k++)
            if (!std::isfinite(initial[k]) || initial[k] < 0.) return fail(XB_E_ARG, "xb_isa_setup: the initial table of atom %lld holds %g at shell %lld", (long long)(k / K), initial[k], (long long)(k % K));
    const size_t nk = (size_t)n * K;
    size_t x = 0;
    std::vector<double> pairs(2 * nk, 0.);
    for (size_t k = 0; k < nk; k++) pairs[2 * k] = initial ? initial[k] : 1.;
    if (int rc = hs_build(c, lattice, atoms_cart, species.data(), n, r_cut, n, K, lo, hi, count, 4 * nk + (size_t)XB_ISA_ITERS_MAX * n + 1, &x, pairs)) return rc;
    c->hs_have = false;   // (until the counts are in)
    c->isa_x = x;
    c->isa_pairs0 = (size_t)(reinterpret_cast<const double *>(c->hs_geom.pairs) - c->ptr<double>(BLK_HS));
    c->isa_cur = 0;
    const IsaAreas A = isa_areas(c);
    // the counting pass: phases 1 and 2 of the tile without a density, a 1 per pair
    HIPCHK(hipMemsetAsync(A.count, 0, (2 * nk + (size_t)XB_ISA_ITERS_MAX * n + 1) * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(A.stats, 0, 2 * sizeof(unsigned int), c->stream));
    IsaArgs args{reinterpret_cast<unsigned long long *>(A.count), A.viol, 0., 0, 0};
    k_isa<ISA_COUNT><<<hirshfeld_groups(c), 256, 0, c->stream>>>(c->hs_geom, nullptr, 0, args, A.stats);
    HIPCHK(hipGetLastError());
    std::vector<long long> cnt(nk);
    HIPCHK(hipMemcpyAsync(cnt.data(), A.count, nk * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long cmax = 0, total = 0, empty = 0;
    for (long long v : cnt) { cmax = std::max(cmax, v); total += v; empty += v == 0; }
    c->isa_e = 61 - isa_ceil_log2(rho_bound) - isa_ceil_log2((unsigned long long)cmax + 1ull);
    c->isa_bound = rho_bound;
    c->sm_cmax = 0; c->sm_pairs = total;   // (xb_stockholder_moments' exponents: the pairs per atom)
    for (int64_t a = 0; a < n; a++) c->sm_cmax = std::max(c->sm_cmax, std::accumulate(cnt.begin() + a * K, cnt.begin() + (a + 1) * K, 0ll));
    c->hs_isa = true;
    c->hs_have = true;
    out_info[0] = c->isa_e; out_info[1] = cmax; out_info[2] = total; out_info[3] = empty;
    return XB_OK;
}

// what the ISA calls check alike: hirshfeld_ready, and that the setup is an ISA one
static int isa_ready(xb_ctx *c, const char *who) {
    if (int rc = hirshfeld_ready(c, who)) return rc;
    if (!c->hs_isa) return fail(XB_E_STATE, "%s: the setup of this grid is %s, not xb_isa_setup's", who, c->hs_mbis ? "xb_mbis_setup's" : "xb_hirshfeld_setup's");
    return XB_OK;
}

int xb_isa_iterate(xb_ctx *c, int64_t iters, int flags, int64_t *qsum_out, int64_t stats[4]) {
    if (int rc = isa_ready(c, "xb_isa_iterate")) return rc;
    if (!qsum_out) return fail(XB_E_ARG, "xb_isa_iterate: null argument");
    if (iters < 1) return fail(XB_E_ARG, "xb_isa_iterate: %lld iterations", (long long)iters);
    if (iters > XB_ISA_ITERS_MAX) return fail(XB_E_LIMIT, "xb_isa_iterate: %lld iterations in one call exceed %d", (long long)iters, XB_ISA_ITERS_MAX);
    const int known = XB_HIRSHFELD_FULL_SEARCH | XB_ISA_DIRECT;
    if (flags & ~known) return fail(XB_E_ARG, "xb_isa_iterate: unknown flag bits 0x%x", flags & ~known);
    if (int rc = analysis_ready(c, "xb_isa_iterate", "", NEED_RHO)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->hs_n, nk = n * (size_t)c->hs_geom.K;
    const IsaAreas A = isa_areas(c);
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    c->hs_have = false;   // (a launch or copy that fails below leaves no setup behind: a table area may be half written, the bins not cleared)
    HIPCHK(hipMemsetAsync(A.qsum, 0, ((size_t)XB_ISA_ITERS_MAX * n + 1) * sizeof(long long), c->stream));   // (the rows and the counter)
    HIPCHK(hipMemsetAsync(A.stats, 0, 2 * sizeof(unsigned int), c->stream));
    HsGeom G = c->hs_geom;
    IsaArgs args{reinterpret_cast<unsigned long long *>(A.bins), A.viol, c->isa_bound, c->isa_e, (flags & XB_ISA_DIRECT) != 0};
    for (int64_t i = 0; i < iters; i++) {
        const int from = (c->isa_cur + (int)(i & 1)) & 1;
        G.pairs = A.pairs[from];
        k_isa<ISA_SHELL><<<hirshfeld_groups(c), 256, 0, c->stream>>>(G, c->rho, forced, args, A.stats);
        HIPCHK(hipGetLastError());
        k_isa_update<<<nblocks((long long)nk), TPB, 0, c->stream>>>(A.count, A.bins, A.pairs[from], A.pairs[from ^ 1], A.qsum + (size_t)i * n, A.viol,
                                                                     c->hs_geom.K, (long long)nk, c->isa_e);
        HIPCHK(hipGetLastError());
    }
    std::vector<unsigned long long> res((size_t)XB_ISA_ITERS_MAX * n + 1);
    unsigned int st[2];
    HIPCHK(hipMemcpyAsync(res.data(), A.qsum, (size_t)iters * n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&res.back(), A.viol, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(st, A.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the one wait of the call
    c->hs_have = true;
    const long long tiles = hirshfeld_tiles(c->hs_geom);
    st[0] = (unsigned int)(st[0] / (unsigned long long)iters);   // (every iteration counted the overflowing tiles)
    tile_route_stats(stats, tiles, forced, st);
    if (stats) stats[3] = (long long)(res.back() / (unsigned long long)iters);
    // with a voxel beyond the bound every update wrote the old tables again: both areas hold what the call found
    if (res.back())
        return fail(XB_E_ARG, "xb_isa_iterate: %llu voxels of the density lie beyond rho_bound = %g", res.back() / (unsigned long long)iters, c->isa_bound);
    memcpy(qsum_out, res.data(), (size_t)iters * n * sizeof(long long));
    c->isa_cur = (c->isa_cur + (int)(iters & 1)) & 1;
    c->hs_geom.pairs = A.pairs[c->isa_cur];
    return XB_OK;
}

int xb_isa_load(xb_ctx *c, const double *tables) {
    if (int rc = isa_ready(c, "xb_isa_load")) return rc;
    if (!tables) return fail(XB_E_ARG, "xb_isa_load: null argument");
    const size_t K = (size_t)c->hs_geom.K, nk = (size_t)c->hs_n * K;
    for (size_t k = 0; k < nk; k++)
        if (!std::isfinite(tables[k]) || tables[k] < 0.) return fail(XB_E_ARG, "xb_isa_load: the table of atom %lld holds %g at shell %lld", (long long)(k / K), tables[k], (long long)(k % K));
    HIPCHK(hipSetDevice(c->device));
    std::vector<double> pairs(2 * nk, 0.);
    for (size_t k = 0; k < nk; k++) pairs[2 * k] = tables[k];
    HIPCHK(hipMemcpyAsync(isa_areas(c).pairs[c->isa_cur], pairs.data(), 2 * nk * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (`pairs` goes)
    return XB_OK;
}

int xb_isa_tables(xb_ctx *c, double *A_out, int64_t *count_out) {
    if (int rc = isa_ready(c, "xb_isa_tables")) return rc;
    if (!A_out && !count_out) return fail(XB_E_ARG, "xb_isa_tables: null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t nk = (size_t)c->hs_n * (size_t)c->hs_geom.K;
    const IsaAreas A = isa_areas(c);
    std::vector<double> pairs(A_out ? 2 * nk : 0);
    if (A_out) HIPCHK(hipMemcpyAsync(pairs.data(), A.pairs[c->isa_cur], 2 * nk * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (count_out) HIPCHK(hipMemcpyAsync(count_out, A.count, nk * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < pairs.size() / 2; k++) A_out[k] = pairs[2 * k];
    return XB_OK;
}

int xb_isa_rho_bound(xb_ctx *c, double *out) {
    if (!c) return fail(XB_E_ARG, "xb_isa_rho_bound: null ctx");
    if (int rc = analysis_ready(c, "xb_isa_rho_bound", "the weights need", NEED_WHOLE | NEED_RHO)) return rc;
    if (!out) return fail(XB_E_ARG, "xb_isa_rho_bound: null argument");
    HIPCHK(hipSetDevice(c->device));
    // a word of the scratch buffer every grid has
    if (c->stage_bytes < sizeof(unsigned long long)) return fail(XB_E_STATE, "xb_isa_rho_bound: no scratch buffer");
    stage_clobbered(*c);
    unsigned long long *w = (unsigned long long *)c->stage, bits = 0;
    HIPCHK(hipMemsetAsync(w, 0, sizeof *w, c->stream));
    k_isa_absmax<<<(unsigned)std::min<long long>(nblocks(c->N), 4096), TPB, 0, c->stream>>>(c->rho, c->N, w);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&bits, w, sizeof bits, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    memcpy(out, &bits, sizeof bits);
    return XB_OK;
}
