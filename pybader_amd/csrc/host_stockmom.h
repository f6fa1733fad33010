// host_stockmom.h -- host side, part 15d: the atomic multipoles and radial moments of a stockholder partition (k_stockmom.h).
// xb_stockholder_moments works on whichever setup of the context is current -- xb_hirshfeld_setup's, xb_isa_setup's or
// xb_mbis_setup's (host_hirshfeld.h, host_isa.h, host_mbis.h) -- reads the resident density and writes nothing resident: not the
// density, not the tables, not the parameters, not a word of the setup's block.
//
// What the exponents need of the setup is kept on the host with it: sm_rmax, the largest cutoff (hs_build), and sm_cmax, sm_pairs,
// the largest and the total pair count.  The ISA and MBIS setups count their pairs anyway and record the two; a plain Hirshfeld
// setup has sm_cmax < 0 until the first call here runs one counting pass (one more host wait, once per setup).
//
// The bins are per call and live in the block of the other moments (BLK_M, ctx_buffers.h; xb_moment_sum fills it anew on every call
// of its own), in 64-bit words:  bins[n][12], count[n] (the counting pass alone), the voxels beyond the bound, the two statistics words.

#define SM_LAUNCH(ms, groups, ...)                                                                                    \
    do {                                                                                                              \
        switch (ms) {                                                                                                 \
        case 0: k_stockmom<SM_MOMENTS, SM_TABLE, 1><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;             \
        case 1: k_stockmom<SM_MOMENTS, SM_SLATER, 1><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;            \
        case 2: k_stockmom<SM_MOMENTS, SM_SLATER, 2><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;            \
        case 4: k_stockmom<SM_MOMENTS, SM_SLATER, 4><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;            \
        default: k_stockmom<SM_MOMENTS, SM_SLATER, 8><<<(groups), 256, 0, c->stream>>>(__VA_ARGS__); break;           \
        }                                                                                                             \
    } while (0)

int xb_stockholder_moments(xb_ctx *c, double rho_bound, int flags, int64_t *bins_out, int64_t info[8], int64_t stats[3]) {
    if (int rc = hirshfeld_ready(c, "xb_stockholder_moments")) return rc;
    if (!bins_out || !info) return fail(XB_E_ARG, "xb_stockholder_moments: null argument");
    if (!std::isfinite(rho_bound) || !(rho_bound > 0.)) return fail(XB_E_ARG, "xb_stockholder_moments: rho_bound = %g is not a positive finite number", rho_bound);
    const int known = XB_HIRSHFELD_FULL_SEARCH | XB_STOCKMOM_DIRECT;
    if (flags & ~known) return fail(XB_E_ARG, "xb_stockholder_moments: unknown flag bits 0x%x", flags & ~known);
    if (int rc = analysis_ready(c, "xb_stockholder_moments", "", NEED_RHO)) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)c->hs_n, nb = SM_BINS * n;
    if (int rc = reserve(c, BLK_M, (nb + n + 2) * sizeof(long long))) return rc;
    unsigned long long *bins = c->ptr<unsigned long long>(BLK_M), *count = bins + nb, *viol = count + n;
    unsigned int *dst = reinterpret_cast<unsigned int *>(viol + 1);
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    SmArgs args{};
    args.viol = viol; args.rho_bound = rho_bound; args.n_atoms = (int)n; args.direct = (flags & XB_STOCKMOM_DIRECT) != 0;
    if (c->sm_cmax < 0) {
        // a plain Hirshfeld setup, for the first time: phase 1 and the pairs of the tile without a density, a 1 per pair
        HIPCHK(hipMemsetAsync(count, 0, (n + 2) * sizeof(long long), c->stream));
        args.bins = count;
        k_stockmom<SM_COUNT, SM_TABLE, 1><<<hirshfeld_groups(c), 256, 0, c->stream>>>(c->hs_geom, nullptr, 0, args, dst);
        HIPCHK(hipGetLastError());
        std::vector<long long> cnt(n);
        HIPCHK(hipMemcpyAsync(cnt.data(), count, n * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        long long cmax = 0, total = 0;
        for (long long v : cnt) { cmax = std::max(cmax, v); total += v; }
        c->sm_cmax = cmax; c->sm_pairs = total;
    }
    const int lb = isa_ceil_log2(rho_bound), lc = isa_ceil_log2((unsigned long long)c->sm_cmax + 1ull), L = std::max(0, isa_ceil_log2(c->sm_rmax));
    for (int k = 0; k < 5; k++) args.e[k] = 61 - lb - lc - k * L;
    args.bins = bins;
    int ms = 0;
    if (c->hs_mbis) {
        args.mb = mbis_args(c, mbis_areas(c), c->mbis_cur);
        ms = c->mbis_MS;
    }
    HIPCHK(hipMemsetAsync(bins, 0, (nb + n + 2) * sizeof(long long), c->stream));
    SM_LAUNCH(ms, hirshfeld_groups(c), c->hs_geom, c->rho, forced, args, dst);
    HIPCHK(hipGetLastError());
    std::vector<long long> res(nb);
    unsigned long long beyond = 0;
    unsigned int st[2];
    HIPCHK(hipMemcpyAsync(res.data(), bins, nb * sizeof(long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&beyond, viol, sizeof beyond, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(st, dst, sizeof st, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));   // the one wait of the call
    for (int k = 0; k < 5; k++) info[k] = args.e[k];
    info[5] = c->sm_cmax; info[6] = c->sm_pairs; info[7] = (long long)beyond;
    tile_route_stats(stats, hirshfeld_tiles(c->hs_geom), forced, st);
    if (beyond) return fail(XB_E_ARG, "xb_stockholder_moments: %llu voxels of the density lie beyond rho_bound = %g", beyond, rho_bound);
    memcpy(bins_out, res.data(), nb * sizeof(long long));
    return XB_OK;
}
