// host_mbis.h -- host side, part 15c: minimal-basis iterative stockholder atoms (k_mbis.h).  An MBIS setup is the third kind of the
// context's Hirshfeld setup (host_hirshfeld.h; ISA's, host_isa.h, is the second): species[a] = a, K = 1 and one zero pair per atom,
// so the cell, the position table, the cutoffs and the image list are that setup's; hs_mbis marks it.  Its pro-atoms are not radial
// tables, so xb_hirshfeld_sum, xb_hirshfeld_field and the xb_isa_* calls refuse it (XB_E_STATE) and the xb_mbis_* calls refuse the
// other kinds; xb_hirshfeld_release frees it, every setup replaces every other.
//
// What the iteration needs lies in the same block (BLK_HS), behind the results, from the even double mbis_x on:
//   the table       KE pairs (E[k], E[k+1] - E[k])
//   two parameter areas of 4 n M doubles each: (c, 1/sigma)[n][M] as pairs, N[n][M], sigma[n][M]; mbis_cur is the current one
//   count[n]        int64
//   bins            [n][2 MS + 1] int64 (binN[MS], binS[MS], binV), then restq, restn
//   rows            [XB_MBIS_ITERS_MAX][2 n + 2] int64: qsum[n], vsum[n], restq, restn of every iteration of one call
//   one word        the voxels beyond rho_bound
//   shells[n]       int32
// The two statistics words of the Hirshfeld results (tiles that overflowed, the longest list) serve these passes too.

struct MbisAreas { double2 *E; double *par[2]; unsigned long long *count, *bins, *rows, *viol; int *shells; unsigned int *stats; };
static MbisAreas mbis_areas(const xb_ctx *c) {
    double *buf = c->ptr<double>(BLK_HS);
    const size_t n = (size_t)c->hs_n, nm = n * (size_t)c->mbis_M, nb = 2 * (size_t)c->mbis_MS + 1;
    MbisAreas a;
    a.E = reinterpret_cast<double2 *>(buf + c->mbis_x);
    a.par[0] = buf + c->mbis_x + 2 * (size_t)c->mbis_KE;
    a.par[1] = a.par[0] + 4 * nm;
    a.count = reinterpret_cast<unsigned long long *>(a.par[1] + 4 * nm);
    a.bins = a.count + n;
    a.rows = a.bins + n * nb + 2;
    a.viol = a.rows + (size_t)XB_MBIS_ITERS_MAX * (2 * n + 2);
    a.shells = reinterpret_cast<int *>(a.viol + 1);
    a.stats = reinterpret_cast<unsigned int *>(buf + c->hs_acc + 2 * n + 2);
    return a;
}
static size_t mbis_words(size_t n, size_t nb) { return n + (n * nb + 2) + (size_t)XB_MBIS_ITERS_MAX * (2 * n + 2) + 1; }   // count .. viol

static MbisArgs mbis_args(const xb_ctx *c, const MbisAreas &A, int from) {
    MbisArgs g{};
    g.E = A.E; g.cis = reinterpret_cast<const double2 *>(A.par[from]); g.shells = A.shells;
    g.bins = A.bins; g.viol = A.viol; g.out = nullptr;
    g.rho_bound = c->mbis_bound; g.Jd = (double)c->mbis_J; g.KEd = (double)c->mbis_KE;
    g.M = c->mbis_M; g.n_atoms = (int)c->hs_n;
    g.eN = c->mbis_e[0]; g.eS = c->mbis_e[1]; g.eV = c->mbis_e[2]; g.eR = c->mbis_e[3];
    return g;
}

// k_mbis<MODE, MS> for the setup's MS
#define MBIS_LAUNCH(MODE, ms, groups, ...)                                                              \
    do {                                                                                                \
        switch (ms) {                                                                                   \
        case 1: k_mbis<MODE, 1><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;                   \
        case 2: k_mbis<MODE, 2><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;                   \
        case 4: k_mbis<MODE, 4><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;                   \
        default: k_mbis<MODE, 8><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;                  \
        }                                                                                               \
    } while (0)

// N[n][M], sigma[n][M] of the caller -> one parameter area; shells beyond an atom's own become (N, sigma) = (0, 1)
static int mbis_pack(const char *who, const int32_t *shells, int64_t n, int M, const double *N, const double *sigma, std::vector<double> &par) {
    const size_t nm = (size_t)n * M;
    par.assign(4 * nm, 0.);
    for (int64_t a = 0; a < n; a++)
        for (int i = 0; i < M; i++) {
            const size_t at = (size_t)a * M + i;
            double Nv = 0., sv = 1.;
            if (i < shells[a]) {
                Nv = N[at]; sv = sigma[at];
                if (!std::isfinite(Nv) || Nv < 0.) return fail(XB_E_ARG, "%s: shell %d of atom %lld holds the population %g", who, i, (long long)a, Nv);
                if (!std::isfinite(sv) || !(sv > 0.)) return fail(XB_E_ARG, "%s: shell %d of atom %lld has the width %g, not a positive finite number", who, i, (long long)a, sv);
            }
            mbis_shell(Nv, sv, par[2 * at], par[2 * at + 1]);
            par[2 * nm + at] = Nv;
            par[3 * nm + at] = sv;
        }
    return XB_OK;
}

int xb_mbis_setup(xb_ctx *c, const double lattice[9], const double *atoms_cart, int64_t n, const double *r_cut, const int32_t *shells,
                  const double *etable, int64_t J, int64_t KE, const double *init_N, const double *init_sigma, double rho_bound,
                  double voxel_volume, int64_t out_info[6]) {
    if (!c) return fail(XB_E_ARG, "xb_mbis_setup: null ctx");
    if (int rc = analysis_ready(c, "xb_mbis_setup", "the weights need", NEED_WHOLE)) return rc;
    if (!out_info || !shells || !etable || !init_N || !init_sigma || !r_cut) return fail(XB_E_ARG, "xb_mbis_setup: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_mbis_setup: %lld atoms", (long long)n);
    if (n > (1 << 26) / XB_MBIS_SHELLS_MAX) return fail(XB_E_LIMIT, "xb_mbis_setup: %lld atoms of up to %d shells exceed 2^26 entries", (long long)n, XB_MBIS_SHELLS_MAX);
    if (!std::isfinite(rho_bound) || !(rho_bound > 0.)) return fail(XB_E_ARG, "xb_mbis_setup: rho_bound = %g is not a positive finite number", rho_bound);
    if (!std::isfinite(voxel_volume) || !(voxel_volume > 0.)) return fail(XB_E_ARG, "xb_mbis_setup: voxel_volume = %g is not a positive finite number", voxel_volume);
    int M = 0;
    for (int64_t a = 0; a < n; a++) {
        if (shells[a] < 1 || shells[a] > XB_MBIS_SHELLS_MAX) return fail(XB_E_ARG, "xb_mbis_setup: atom %lld has %d shells, outside 1 .. %d", (long long)a, shells[a], XB_MBIS_SHELLS_MAX);
        M = std::max(M, (int)shells[a]);
    }
    if (J < 1 || KE < 1) return fail(XB_E_ARG, "xb_mbis_setup: a table of %lld knots per unit and %lld knots", (long long)J, (long long)KE);
    if (KE > (1 << 26)) return fail(XB_E_LIMIT, "xb_mbis_setup: %lld knots exceed 2^26", (long long)KE);
    for (int64_t k = 0; k <= KE; k++)
        if (!std::isfinite(etable[k]) || etable[k] < 0.) return fail(XB_E_ARG, "xb_mbis_setup: the table holds %g at knot %lld", etable[k], (long long)k);
    if (etable[KE] != 0.) return fail(XB_E_ARG, "xb_mbis_setup: the table ends with %g, not with 0", etable[KE]);
    std::vector<double> par;
    if (int rc = mbis_pack("xb_mbis_setup", shells, n, M, init_N, init_sigma, par)) return rc;
    std::vector<int32_t> species((size_t)n);
    for (size_t a = 0; a < species.size(); a++) species[a] = (int32_t)a;
    std::vector<int> lo, hi;
    int64_t count = 0;
    if (int rc = hs_ranges("xb_mbis_setup", lattice, atoms_cart, species.data(), n, r_cut, n, lo, hi, &count)) return rc;
    const int MS = M <= 1 ? 1 : (M <= 2 ? 2 : (M <= 4 ? 4 : 8));
    const size_t nm = (size_t)n * M, nb = 2 * (size_t)MS + 1, words = mbis_words((size_t)n, nb);
    size_t x = 0;
    const std::vector<double> pairs(2 * (size_t)n, 0.);
    if (int rc = hs_build(c, lattice, atoms_cart, species.data(), n, r_cut, n, 1, lo, hi, count, 2 * (size_t)KE + 8 * nm + words + ((size_t)n + 1) / 2, &x, pairs)) return rc;
    c->hs_have = false;   // (until the counts are in)
    c->mbis_x = x; c->mbis_M = M; c->mbis_MS = MS; c->mbis_J = J; c->mbis_KE = KE; c->mbis_cur = 0;
    c->mbis_bound = rho_bound; c->mbis_vv = voxel_volume;
    c->mbis_shells.assign(shells, shells + n);
    const MbisAreas A = mbis_areas(c);
    std::vector<double> host(2 * (size_t)KE + 8 * nm, 0.);
    for (int64_t k = 0; k < KE; k++) { host[2 * k] = etable[k]; host[2 * k + 1] = etable[k + 1] - etable[k]; }
    std::copy(par.begin(), par.end(), host.begin() + 2 * (size_t)KE);
    std::copy(par.begin(), par.end(), host.begin() + 2 * (size_t)KE + 4 * nm);
    HIPCHK(hipMemcpyAsync(A.E, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(A.shells, shells, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(A.count, 0, words * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(A.stats, 0, 2 * sizeof(unsigned int), c->stream));
    // the counting pass: phase 1 and the pairs of the tile without a density, a 1 per pair
    MbisArgs args = mbis_args(c, A, 0);
    args.bins = A.count;
    k_mbis<MBIS_COUNT, 1><<<hirshfeld_groups(c), 256, 0, c->stream>>>(c->hs_geom, nullptr, 0, args, A.stats);
    HIPCHK(hipGetLastError());
    std::vector<long long> cnt((size_t)n);
    HIPCHK(hipMemcpyAsync(cnt.data(), A.count, (size_t)n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (`host` goes)
    long long cmax = 0, total = 0;
    double rmax = 0.;
    for (long long v : cnt) { cmax = std::max(cmax, v); total += v; }
    for (int64_t a = 0; a < n; a++) rmax = std::max(rmax, r_cut[a]);
    const int lc = isa_ceil_log2((unsigned long long)cmax + 1ull), lb = isa_ceil_log2(rho_bound);
    c->mbis_e[0] = 61 - lb - lc;
    c->mbis_e[1] = c->mbis_e[0] - std::max(0, isa_ceil_log2(rmax));
    c->mbis_e[2] = 61 - lc;
    c->mbis_e[3] = 61 - lb - isa_ceil_log2((unsigned long long)c->N + 1ull);
    c->sm_cmax = cmax; c->sm_pairs = total;   // (xb_stockholder_moments' exponents)
    c->hs_mbis = true;
    c->hs_have = true;
    for (int k = 0; k < 4; k++) out_info[k] = c->mbis_e[k];
    out_info[4] = cmax; out_info[5] = total;
    return XB_OK;
}

// what the MBIS calls check alike: hirshfeld_ready, and that the setup is an MBIS one
static int mbis_ready(xb_ctx *c, const char *who) {
    if (int rc = hirshfeld_ready(c, who)) return rc;
    if (!c->hs_mbis) return fail(XB_E_STATE, "%s: the setup of this grid is not xb_mbis_setup's", who);
    return XB_OK;
}

int xb_mbis_iterate(xb_ctx *c, int64_t iters, int flags, int64_t *qsum_out, int64_t *vsum_out, int64_t *rest_out, int64_t stats[4]) {
    if (int rc = mbis_ready(c, "xb_mbis_iterate")) return rc;
    if (!qsum_out || !vsum_out || !rest_out) return fail(XB_E_ARG, "xb_mbis_iterate: null argument");
    if (iters < 1) return fail(XB_E_ARG, "xb_mbis_iterate: %lld iterations", (long long)iters);
    if (iters > XB_MBIS_ITERS_MAX) return fail(XB_E_LIMIT, "xb_mbis_iterate: %lld iterations in one call exceed %d", (long long)iters, XB_MBIS_ITERS_MAX);
    const int known = XB_HIRSHFELD_FULL_SEARCH | XB_MBIS_DIRECT | XB_MBIS_KEEP;
    if (flags & ~known) return fail(XB_E_ARG, "xb_mbis_iterate: unknown flag bits 0x%x", flags & ~known);
    const int keep = (flags & XB_MBIS_KEEP) != 0;
    if (keep && iters != 1) return fail(XB_E_ARG, "xb_mbis_iterate: XB_MBIS_KEEP with %lld iterations, not 1", (long long)iters);
    if (int rc = analysis_ready(c, "xb_mbis_iterate", "", NEED_RHO)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->hs_n, nm = n * (size_t)c->mbis_M, rw = 2 * n + 2;
    const MbisAreas A = mbis_areas(c);
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    c->hs_have = false;   // (a launch or copy that fails below leaves no setup behind: an area may be half written, the bins not cleared)
    HIPCHK(hipMemsetAsync(A.rows, 0, ((size_t)XB_MBIS_ITERS_MAX * rw + 1) * sizeof(long long), c->stream));   // (the rows and the counter)
    HIPCHK(hipMemsetAsync(A.stats, 0, 2 * sizeof(unsigned int), c->stream));
    for (int64_t i = 0; i < iters; i++) {
        const int from = (c->mbis_cur + (int)(i & 1)) & 1;
        MbisArgs args = mbis_args(c, A, from);
        args.direct = (flags & XB_MBIS_DIRECT) != 0;
        MBIS_LAUNCH(MBIS_SHELL, c->mbis_MS, hirshfeld_groups(c), c->hs_geom, c->rho, forced, args, A.stats);
        HIPCHK(hipGetLastError());
        k_mbis_update<<<nblocks((long long)nm), TPB, 0, c->stream>>>(A.bins, A.par[from], A.par[from ^ 1], A.rows + (size_t)i * rw, A.viol, (int)n,
                                                                      c->mbis_M, c->mbis_MS, c->mbis_e[0], c->mbis_e[1], c->mbis_vv, keep);
        HIPCHK(hipGetLastError());
    }
    std::vector<long long> res((size_t)iters * rw + 1);
    unsigned int st[2];
    HIPCHK(hipMemcpyAsync(res.data(), A.rows, (size_t)iters * rw * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&res.back(), A.viol, sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(st, A.stats, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the one wait of the call
    c->hs_have = true;
    st[0] = (unsigned int)(st[0] / (unsigned long long)iters);   // (every iteration counted the overflowing tiles)
    tile_route_stats(stats, hirshfeld_tiles(c->hs_geom), forced, st);
    const unsigned long long beyond = (unsigned long long)res.back() / (unsigned long long)iters;
    if (stats) stats[3] = (long long)beyond;
    // with a voxel beyond the bound every update wrote the old parameters again: both areas hold what the call found
    if (res.back()) return fail(XB_E_ARG, "xb_mbis_iterate: %llu voxels of the density lie beyond rho_bound = %g", beyond, c->mbis_bound);
    for (int64_t i = 0; i < iters; i++) {
        const long long *row = res.data() + (size_t)i * rw;
        memcpy(qsum_out + (size_t)i * n, row, n * sizeof(long long));
        memcpy(vsum_out + (size_t)i * n, row + n, n * sizeof(long long));
        rest_out[2 * i] = row[2 * n]; rest_out[2 * i + 1] = row[2 * n + 1];
    }
    if (!keep) c->mbis_cur = (c->mbis_cur + (int)(iters & 1)) & 1;
    return XB_OK;
}

int xb_mbis_params(xb_ctx *c, double *N_out, double *sigma_out, int64_t *count_out) {
    if (int rc = mbis_ready(c, "xb_mbis_params")) return rc;
    if (!N_out && !sigma_out && !count_out) return fail(XB_E_ARG, "xb_mbis_params: null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->hs_n, nm = n * (size_t)c->mbis_M;
    const MbisAreas A = mbis_areas(c);
    const double *par = A.par[c->mbis_cur];
    if (N_out) HIPCHK(hipMemcpyAsync(N_out, par + 2 * nm, nm * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (sigma_out) HIPCHK(hipMemcpyAsync(sigma_out, par + 3 * nm, nm * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    if (count_out) HIPCHK(hipMemcpyAsync(count_out, A.count, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

int xb_mbis_load(xb_ctx *c, const double *N, const double *sigma) {
    if (int rc = mbis_ready(c, "xb_mbis_load")) return rc;
    if (!N || !sigma) return fail(XB_E_ARG, "xb_mbis_load: null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->hs_n;
    const MbisAreas A = mbis_areas(c);
    std::vector<double> par;
    if (int rc = mbis_pack("xb_mbis_load", c->mbis_shells.data(), (int64_t)n, c->mbis_M, N, sigma, par)) return rc;
    HIPCHK(hipMemcpyAsync(A.par[c->mbis_cur], par.data(), par.size() * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // (`par` goes)
    return XB_OK;
}

int xb_mbis_field(xb_ctx *c, int mode, int flags, double *out_host, void *out_dev) {
    if (int rc = mbis_ready(c, "xb_mbis_field")) return rc;
    if (mode != XB_HIRSHFELD_PROMOLECULE && mode != XB_HIRSHFELD_DEFORMATION) return fail(XB_E_ARG, "xb_mbis_field: unknown mode %d", mode);
    if ((out_host != nullptr) == (out_dev != nullptr)) return fail(XB_E_ARG, "xb_mbis_field: exactly one of out_host and out_dev is wanted");
    if (flags & ~XB_HIRSHFELD_FULL_SEARCH) return fail(XB_E_ARG, "xb_mbis_field: unknown flag bits 0x%x", flags & ~XB_HIRSHFELD_FULL_SEARCH);
    if (mode == XB_HIRSHFELD_DEFORMATION && !c->have_rho) return fail(XB_E_STATE, "xb_mbis_field: no density on this grid yet");
    HIPCHK(hipSetDevice(c->device));
    double *dst = (double *)out_dev;
    if (out_dev) {
        uintptr_t lo, hi;
        if (int rc = io_check_dense(c, "xb_mbis_field", out_dev, sizeof(double), &lo, &hi)) return rc;
        if (io_overlaps(lo, hi, c->rho, (size_t)c->N * 8)) return fail(XB_E_ARG, "xb_mbis_field: the destination overlaps the resident density");
        if (io_overlaps(lo, hi, c->ptr<void>(BLK_HS), c->bytes(BLK_HS))) return fail(XB_E_ARG, "xb_mbis_field: the destination overlaps the setup");
    } else {
        if (c->stage_bytes < (size_t)c->N * sizeof(double)) return fail(XB_E_STATE, "xb_mbis_field: the scratch buffer holds no whole grid");
        stage_clobbered(*c);
        dst = (double *)c->stage;
    }
    const MbisAreas A = mbis_areas(c);
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    MbisArgs args = mbis_args(c, A, c->mbis_cur);
    args.out = dst;
    args.deform = mode == XB_HIRSHFELD_DEFORMATION;
    MBIS_LAUNCH(MBIS_FIELD, c->mbis_MS, (unsigned)hirshfeld_tiles(c->hs_geom), c->hs_geom, c->rho, forced, args, A.stats);
    HIPCHK(hipGetLastError());
    if (out_host) return staged_d2h(c, out_host, dst, (size_t)c->N * sizeof(double));   // (waits)
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
