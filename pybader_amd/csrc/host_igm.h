// host_igm.h -- host side of IGM, the independent gradient model (k_igm.h).  xb_igm_field reads the table setup of
// host_hirshfeld.h / host_isa.h and the resident density; xb_igm_sum reads the resident density and labels and two device fields
// of the caller's.  Neither writes anything resident.
//
// Both use the NCI sums' block of the context (ctx_buffers.h), which every call that uses it fills anew:
//   xb_igm_field   BLK_NCI = the two statistics words of hs_candidates (one 8-byte word), then the fragment of every atom (int32)
//   xb_igm_sum     BLK_NCI = sum of rho [3 n], sum of val [3 n], counts [3 n] (64-bit integers)
// xb_igm_field writes its first host output into `stage` (N doubles on a whole grid: need_scratch) and a second one into a
// temporary buffer of N doubles, and copies from there.

#define IGM_LAUNCH(MODE, F) \
    k_igm<MODE, F><<<(unsigned)hirshfeld_tiles(G), 256, 0, c->stream>>>(G, c->rho, frag, K, p_min, forced, out[0], out[1], st)

int xb_igm_field(xb_ctx *c, const double lattice[9], const int32_t *fragment, int n_fragments, int mode, double p_min, int flags,
                 double *dg_host, double *dgi_host, void *dg_dev, void *dgi_dev, int64_t stats[3]) {
    if (int rc = hirshfeld_ready(c, "xb_igm_field")) return rc;
    if (c->hs_mbis) return fail(XB_E_STATE, "xb_igm_field: the setup of this grid is xb_mbis_setup's: its pro-atoms are no radial tables");
    if (!lattice || !fragment) return fail(XB_E_ARG, "xb_igm_field: null argument");
    if (n_fragments < 1 || n_fragments > XB_IGM_FRAGMENTS_MAX)
        return fail(XB_E_ARG, "xb_igm_field: %d fragments; 1 .. %d are wanted", n_fragments, XB_IGM_FRAGMENTS_MAX);
    if (mode != XB_IGM_PRO && mode != XB_IGM_STOCKHOLDER) return fail(XB_E_ARG, "xb_igm_field: unknown mode %d", mode);
    if (flags & ~XB_HIRSHFELD_FULL_SEARCH) return fail(XB_E_ARG, "xb_igm_field: unknown flag bits 0x%x", flags & ~XB_HIRSHFELD_FULL_SEARCH);
    if (!std::isfinite(p_min) || p_min < 0.) return fail(XB_E_ARG, "xb_igm_field: p_min (%g) must be finite and not negative", p_min);
    if ((dg_host && dg_dev) || (dgi_host && dgi_dev)) return fail(XB_E_ARG, "xb_igm_field: a field goes to the host or to the device, not to both");
    if (!dg_host && !dg_dev && !dgi_host && !dgi_dev) return fail(XB_E_ARG, "xb_igm_field: neither field is asked for");
    const size_t n = (size_t)c->hs_n;
    for (size_t a = 0; a < n; a++)
        if (fragment[a] < -1 || fragment[a] >= n_fragments)
            return fail(XB_E_ARG, "xb_igm_field: atom %zu has fragment %d, outside [-1, %d)", a, fragment[a], n_fragments);
    const HsGeom &G = c->hs_geom;
    for (int k = 0; k < 9; k++)
        if (!(lattice[k] == G.lat[k])) return fail(XB_E_ARG, "xb_igm_field: the lattice is not the setup's (entry %d: %g, the setup has %g)", k, lattice[k], G.lat[k]);
    if (int rc = analysis_ready(c, "xb_igm_field", "", NEED_RHO)) return rc;
    StCoeffs K;
    if (int rc = xb_stencil_coeffs(lattice, c->g.nx, c->g.ny, c->g.nz, reinterpret_cast<double *>(&K))) return rc;
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->N * sizeof(double), want = 8 + n * sizeof(int);
    if (int rc = reserve(c, BLK_NCI, want)) return rc;
    void *const dev[2] = {dg_dev, dgi_dev};
    uintptr_t lo[2] = {0, 0}, hi[2] = {0, 0};
    for (int k = 0; k < 2; k++) {
        if (!dev[k]) continue;
        if (int rc = io_check_dense(c, "xb_igm_field", dev[k], sizeof(double), &lo[k], &hi[k])) return rc;
        if (io_overlaps(lo[k], hi[k], c->rho, bytes)) return fail(XB_E_ARG, "xb_igm_field: a destination overlaps the resident density");
        if (io_overlaps(lo[k], hi[k], c->ptr<void>(BLK_HS), c->bytes(BLK_HS))) return fail(XB_E_ARG, "xb_igm_field: a destination overlaps the setup");
        if (io_overlaps(lo[k], hi[k], c->ptr<void>(BLK_NCI), c->bytes(BLK_NCI)))
            return fail(XB_E_ARG, "xb_igm_field: a destination overlaps the context's buffers");
    }
    if (dg_dev && dgi_dev && lo[0] < hi[1] && lo[1] < hi[0]) return fail(XB_E_ARG, "xb_igm_field: the two destinations overlap");
    double *out[2] = {(double *)dg_dev, (double *)dgi_dev};
    double *const host[2] = {dg_host, dgi_host};
    DevBuf<double> tmp;
    if (dg_host || dgi_host) {
        if (c->stage_bytes < bytes) return fail(XB_E_STATE, "xb_igm_field: the scratch buffer holds no whole grid");
        if (dg_host && dgi_host) HIPCHK(tmp.alloc((size_t)c->N));
        stage_clobbered(*c);
        out[dg_host ? 0 : 1] = (double *)c->stage;
        if (dg_host && dgi_host) out[1] = tmp.p;
    }
    unsigned int *st = c->ptr<unsigned int>(BLK_NCI);
    int *frag = reinterpret_cast<int *>(st + 2);
    HIPCHK(hipMemsetAsync(st, 0, 8, c->stream));
    HIPCHK(hipMemcpyAsync(frag, fragment, n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    const int forced = (flags & XB_HIRSHFELD_FULL_SEARCH) != 0;
    const bool four = n_fragments > 2;   // (1 -> 2 and 3 -> 4: an empty fragment adds +0.0 to gX)
    if (mode == XB_IGM_PRO) {
        if (four) IGM_LAUNCH(IGM_PRO, 4);
        else IGM_LAUNCH(IGM_PRO, 2);
    } else {
        if (four) IGM_LAUNCH(IGM_STOCKHOLDER, 4);
        else IGM_LAUNCH(IGM_STOCKHOLDER, 2);
    }
    HIPCHK(hipGetLastError());
    unsigned int sth[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(sth, st, sizeof sth, hipMemcpyDeviceToHost, c->stream));
    for (int k = 0; k < 2; k++)
        if (host[k])
            if (int rc = staged_d2h(c, host[k], out[k], bytes)) return rc;   // (waits)
    HIPCHK(hipStreamSynchronize(c->stream));
    tile_route_stats(stats, hirshfeld_tiles(G), forced, sth);
    return XB_OK;
}

int xb_igm_sum(xb_ctx *c, const void *val_dev, const void *x_dev, int64_t n, double voxel_volume, double cut, double rho_split,
               int64_t *count, double *charge, double *integral) {
    ANALYSIS_NEED_GRID("xb_igm_sum");
    if (!val_dev || !x_dev || !count || !charge || !integral) return fail(XB_E_ARG, "xb_igm_sum: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_igm_sum: %lld labels", (long long)n);
    if (!std::isfinite(rho_split) || rho_split < 0.) return fail(XB_E_ARG, "xb_igm_sum: rho_split (%g) must be finite and not negative", rho_split);
    if (!std::isfinite(cut) || !(cut > 0.)) return fail(XB_E_ARG, "xb_igm_sum: cut (%g) must be finite and above 0", cut);
    if (n > XB_INT_MAX / 3) return fail(XB_E_LIMIT, "xb_igm_sum: %lld labels exceed %d", (long long)n, XB_INT_MAX / 3);
    if (int rc = analysis_ready(c, "xb_igm_sum", "the sums need", NEED_WHOLE | NEED_RHO | NEED_LABELS)) return rc;
    HIPCHK(hipSetDevice(c->device));
    uintptr_t lo, hi;
    if (int rc = io_check_dense(c, "xb_igm_sum", val_dev, sizeof(double), &lo, &hi)) return rc;
    if (int rc = io_check_dense(c, "xb_igm_sum", x_dev, sizeof(double), &lo, &hi)) return rc;
    if (int rc = settle_labels(c)) return rc;
    const size_t keys = 3 * (size_t)n, want = 3 * keys;
    if (int rc = reserve(c, BLK_NCI, want * sizeof(double))) return rc;
    double *ds = c->ptr<double>(BLK_NCI), *dq = ds + keys;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(dq + keys);
    HIPCHK(hipMemsetAsync(ds, 0, want * sizeof(double), c->stream));
    const unsigned blocks = (unsigned)((c->N + (long long)IGM_SUM_STEPS * TPB - 1) / ((long long)IGM_SUM_STEPS * TPB));
    if (n <= NCI_LABELS_LDS)
        k_igm_sum<true><<<blocks, TPB, 0, c->stream>>>((long long)c->N, c->rho, c->labels, (const double *)val_dev, (const double *)x_dev, (int)n, cut, rho_split, ds, dq, dc);
    else
        k_igm_sum<false><<<blocks, TPB, 0, c->stream>>>((long long)c->N, c->rho, c->labels, (const double *)val_dev, (const double *)x_dev, (int)n, cut, rho_split, ds, dq, dc);
    HIPCHK(hipGetLastError());
    static_assert(sizeof(unsigned long long) == sizeof(int64_t), "the counts travel as they are");
    HIPCHK(hipMemcpyAsync(charge, ds, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(integral, dq, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(count, dc, keys * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < keys; i++) {
        charge[i] *= voxel_volume;
        integral[i] *= voxel_volume;
    }
    return XB_OK;
}
