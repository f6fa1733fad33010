// host_regions.h -- host side, part 19: connected components of a periodic voxel mask (k_regions.h).  The calls read the resident
// density, a caller's field and the resident labels of the whole grid and write nothing resident.
//
// Scratch: the roots' numbers (4 N bytes), the runs' counts (16 bytes per RG_BLOCK voxels) and the chunks' sums live in `stage`
// (N doubles on a whole grid: need_scratch), which is scratch between calls; the sums per component, the share table and the key
// list in temporary buffers.  With XB_DOMAINS_TIMES five events bracket the four stages (xb_regions_times).
// Kept (blocks of ctx_buffers.h, freed by xb_regions_release; the result is discarded by every writer of the density): BLK_RG_MAP,
// the component of every voxel (4 N bytes), and BLK_RG_SEED, the smallest index of every component (4 bytes each, at least one).

static void regions_forget(xb_ctx *c) {
    c->rg_m = 0; c->rg_members = 0; c->rg_have = false; c->rg_sh_have = false;
    std::vector<int32_t>().swap(c->rg_sh_comp); std::vector<int32_t>().swap(c->rg_sh_lab);
    std::vector<int64_t>().swap(c->rg_sh_cnt);
}

int xb_regions_label(xb_ctx *c, int mode, const void *field_dev, double level, const double lattice[9], double s_cut, double rho_cut,
                     int flags, int64_t *m_out) {
    ANALYSIS_NEED_GRID("xb_regions_label");
    if (!m_out) return fail(XB_E_ARG, "xb_regions_label: null argument");
    if (mode != XB_DOMAINS_ABOVE && mode != XB_DOMAINS_BELOW && mode != XB_DOMAINS_NCI) return fail(XB_E_ARG, "xb_regions_label: unknown mode %d", mode);
    const int known = XB_DOMAINS_GLOBAL | XB_DOMAINS_GATHER | XB_DOMAINS_TIMES;
    if (flags & ~known) return fail(XB_E_ARG, "xb_regions_label: unknown flag bits 0x%x", flags & ~known);
    const bool nci = mode == XB_DOMAINS_NCI;
    StCoeffs K{};
    NciCuts C{0., 0., 0.};
    if (nci) {
        if (!lattice) return fail(XB_E_ARG, "xb_regions_label: the NCI region needs a lattice");
        if (field_dev) return fail(XB_E_ARG, "xb_regions_label: the NCI region is that of the resident density; no field is taken");
        if (!std::isfinite(s_cut) || !std::isfinite(rho_cut) || s_cut < 0. || rho_cut < 0.)
            return fail(XB_E_ARG, "xb_regions_label: the thresholds (%g, %g) must be finite and not negative", s_cut, rho_cut);
        if (int rc = stencil_ready(c, "xb_regions_label", lattice, false, &K)) return rc;
        C = NciCuts{nci_threshold(s_cut), rho_cut, 0.};
    } else {
        if (level != level) return fail(XB_E_ARG, "xb_regions_label: the level is NaN");
        if (flags & XB_DOMAINS_GATHER) return fail(XB_E_ARG, "xb_regions_label: XB_DOMAINS_GATHER belongs to the NCI region's predicate");
        if (int rc = analysis_ready(c, "xb_regions_label", "the components need", NEED_WHOLE | NEED_RHO)) return rc;
    }
    if (c->N > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_regions_label: %lld voxels exceed %d", c->N, XB_INT_MAX);
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const long long N = c->N, nb = (N + RG_BLOCK - 1) / RG_BLOCK, np = (nb + ISO_CHUNK - 1) / ISO_CHUNK;
    const size_t off_tot = ((size_t)N * 4 + 15) / 16 * 16, off_part = off_tot + (size_t)nb * 16, off_grand = off_part + (size_t)np * 16;
    if (c->stage_bytes < off_grand + 16) return fail(XB_E_STATE, "xb_regions_label: the scratch buffer holds no whole grid");
    if (field_dev) {
        uintptr_t lo, hi;
        if (int rc = io_check_dense(c, "xb_regions_label", field_dev, sizeof(double), &lo, &hi)) return rc;
        if (io_overlaps(lo, hi, c->stage, c->stage_bytes)) return fail(XB_E_ARG, "xb_regions_label: the field overlaps the context's scratch");
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->rg_have = false; c->rg_sh_have = false;
    stage_clobbered(*c);
    if (int rc = reserve(c, BLK_RG_MAP, (size_t)N * sizeof(int))) return rc;
    int *const rg_map = c->ptr<int>(BLK_RG_MAP);
    const double *f = field_dev ? (const double *)field_dev : c->rho;
    int *num = reinterpret_cast<int *>(c->stage);
    unsigned long long *tot = reinterpret_cast<unsigned long long *>((char *)c->stage + off_tot);
    unsigned long long *part = reinterpret_cast<unsigned long long *>((char *)c->stage + off_part);
    unsigned long long *grand = reinterpret_cast<unsigned long long *>((char *)c->stage + off_grand);
    const unsigned tiles = stencil_tiles(g);
    const bool global = (flags & XB_DOMAINS_GLOBAL) != 0, gather = (flags & XB_DOMAINS_GATHER) != 0;
    const int below = mode == XB_DOMAINS_BELOW;
    // XB_DOMAINS_TIMES: an event before the first launch and one behind each of the four stages
    const bool timed = (flags & XB_DOMAINS_TIMES) != 0;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    struct EvGuard { hipEvent_t *e; ~EvGuard() { for (int k = 0; k < 5; k++) if (e[k]) hipEventDestroy(e[k]); } } guard{ev};
    c->rg_timed = false;
    if (timed) {
        for (int k = 0; k < 5; k++) HIPCHK(hipEventCreate(&ev[k]));
        HIPCHK(hipEventRecord(ev[0], c->stream));
    }
#define RG_TILE_LAUNCH(SRC, LOCAL) k_rg_tile<SRC, LOCAL><<<tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, below, K, C, rg_map)
    if (!nci) { if (global) RG_TILE_LAUNCH(RG_SRC_FIELD, false); else RG_TILE_LAUNCH(RG_SRC_FIELD, true); }
    else if (gather) { if (global) RG_TILE_LAUNCH(RG_SRC_NCI_GATHER, false); else RG_TILE_LAUNCH(RG_SRC_NCI_GATHER, true); }
    else { if (global) RG_TILE_LAUNCH(RG_SRC_NCI_TILE, false); else RG_TILE_LAUNCH(RG_SRC_NCI_TILE, true); }
#undef RG_TILE_LAUNCH
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(ev[1], c->stream));
    if (global) k_rg_link<true><<<nblocks(N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, rg_map);
    else k_rg_link<false><<<nblocks(N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, rg_map);
    if (timed) HIPCHK(hipEventRecord(ev[2], c->stream));
    k_rg_flatten<<<nblocks(N), TPB, 0, c->stream>>>(N, rg_map);
    if (timed) HIPCHK(hipEventRecord(ev[3], c->stream));
    k_rg_count<<<(unsigned)nb, TPB, 0, c->stream>>>(N, rg_map, tot);
    k_iso_scan_sums<<<(unsigned)np, TPB, 0, c->stream>>>(tot, nb, part);
    k_iso_scan_top<<<1, XB_WAVE, 0, c->stream>>>(part, np, grand);
    k_iso_scan_apply<<<(unsigned)np, TPB, 0, c->stream>>>(tot, nb, part);
    HIPCHK(hipGetLastError());
    unsigned long long want[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(want, grand, sizeof want, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (want[0] > want[1] || want[1] > (unsigned long long)N)
        return fail(XB_E_STATE, "xb_regions_label: the count pass reports %llu roots and %llu members on %lld voxels", want[0], want[1], N);
    const size_t m = (size_t)want[0];
    release(c, BLK_RG_SEED, BLK_RG_SEED);   // (exactly the last labelling's seeds are kept and counted)
    if (int rc = reserve(c, BLK_RG_SEED, std::max<size_t>(m, 1) * sizeof(int))) return rc;
    k_rg_emit<<<(unsigned)nb, TPB, 0, c->stream>>>(N, rg_map, tot, c->ptr<int>(BLK_RG_SEED), num);
    k_rg_number<<<nblocks(N), TPB, 0, c->stream>>>(N, rg_map, num);
    HIPCHK(hipGetLastError());
    if (timed) HIPCHK(hipEventRecord(ev[4], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (timed) {
        for (int k = 0; k < 4; k++) {
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, ev[k], ev[k + 1]));
            c->rg_ms[k] = ms;
        }
        c->rg_timed = true;
    }
    c->rg_m = m; c->rg_members = (size_t)want[1];
    c->rg_nci = nci; c->rg_K = K;
    c->rg_have = true;
    *m_out = (int64_t)m;
    return XB_OK;
}

int xb_regions_sums(xb_ctx *c, double voxel_volume, double rho_split, int64_t *seed, int64_t *count, int64_t *top, double *sum1, double *sum2,
                    int64_t *count3, double *sum1_3, double *sum2_3, int64_t capacity) {
    if (!c || !c->rg_have) return fail(XB_E_STATE, "xb_regions_sums: no result (call xb_regions_label first)");
    const bool classes = rho_split == rho_split;
    if (!seed || !count || !top || !sum1 || !sum2 || (classes && (!count3 || !sum1_3 || !sum2_3))) return fail(XB_E_ARG, "xb_regions_sums: null argument");
    if (classes && (!std::isfinite(rho_split) || rho_split < 0.)) return fail(XB_E_ARG, "xb_regions_sums: rho_split (%g) must be finite and not negative, or NaN for no classes", rho_split);
    if (classes && !c->rg_nci) return fail(XB_E_STATE, "xb_regions_sums: classes need components of the NCI region");
    const size_t m = c->rg_m;
    if (capacity < (int64_t)m) return fail(XB_E_ARG, "xb_regions_sums: capacity %lld below %lld components", (long long)capacity, (long long)m);
    if (m > (size_t)XB_INT_MAX / 3) return fail(XB_E_LIMIT, "xb_regions_sums: %lld components exceed %d", (long long)m, XB_INT_MAX / 3);
    if (!m) return XB_OK;
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const size_t keys = classes ? 3 * m : m, words = 3 * keys + 2 * m;
    DevBuf<double> buf;
    HIPCHK(buf.alloc(words));
    double *ds = buf.p, *dq = ds + keys;
    unsigned long long *dc = reinterpret_cast<unsigned long long *>(dq + keys), *dk = dc + keys, *dl = dk + m;
    HIPCHK(hipMemsetAsync(buf.p, 0, words * sizeof(double), c->stream));
    if (classes) k_rg_sums<true><<<nblocks((c->N + RG_STEPS - 1) / RG_STEPS), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->ptr<int>(BLK_RG_MAP), c->rg_K, rho_split, ds, dq, dc, dk);
    else k_rg_sums<false><<<nblocks((c->N + RG_STEPS - 1) / RG_STEPS), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->ptr<int>(BLK_RG_MAP), c->rg_K, rho_split, ds, dq, dc, dk);
    k_rg_top<<<nblocks(c->N), TPB, 0, c->stream>>>(c->N, c->rho, c->ptr<int>(BLK_RG_MAP), dk, dl);
    HIPCHK(hipGetLastError());
    std::vector<double> hs(keys), hq(keys);
    std::vector<unsigned long long> hc(keys), hl(m);
    std::vector<int32_t> hseed(m);
    HIPCHK(hipMemcpyAsync(hs.data(), ds, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hq.data(), dq, keys * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hc.data(), dc, keys * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hl.data(), dl, m * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(hseed.data(), c->ptr<int>(BLK_RG_SEED), m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < m; i++) {
        seed[i] = hseed[i];
        top[i] = (int64_t)hl[i];
        if (classes) {
            // the totals from the classes: the three partial sums added before the one multiplication
            count[i] = (int64_t)(hc[3 * i] + hc[3 * i + 1] + hc[3 * i + 2]);
            sum1[i] = ((hs[3 * i] + hs[3 * i + 1]) + hs[3 * i + 2]) * voxel_volume;
            sum2[i] = ((hq[3 * i] + hq[3 * i + 1]) + hq[3 * i + 2]) * voxel_volume;
            for (int k = 0; k < 3; k++) {
                count3[3 * i + k] = (int64_t)hc[3 * i + k];
                sum1_3[3 * i + k] = hs[3 * i + k] * voxel_volume;
                sum2_3[3 * i + k] = hq[3 * i + k] * voxel_volume;
            }
        } else {
            count[i] = (int64_t)hc[i];
            sum1[i] = hs[i] * voxel_volume;
            sum2[i] = hq[i] * voxel_volume;
        }
    }
    return XB_OK;
}

int xb_regions_shares(xb_ctx *c, int64_t n, int flags, int64_t *n_triplets) {
    if (!c || !c->rg_have) return fail(XB_E_STATE, "xb_regions_shares: no result (call xb_regions_label first)");
    if (!n_triplets) return fail(XB_E_ARG, "xb_regions_shares: null argument");
    if (flags & ~XB_DOMAINS_SHARES_LIST) return fail(XB_E_ARG, "xb_regions_shares: unknown flag bits 0x%x", flags & ~XB_DOMAINS_SHARES_LIST);
    if (n < 1) return fail(XB_E_ARG, "xb_regions_shares: %lld labels", (long long)n);
    if (n > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_regions_shares: %lld labels exceed %d", (long long)n, XB_INT_MAX);
    if (!c->have_labels) return fail(XB_E_STATE, "xb_regions_shares: no labels on this grid yet");
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    c->rg_sh_have = false;
    c->rg_sh_comp.clear(); c->rg_sh_lab.clear(); c->rg_sh_cnt.clear();
    const size_t m = c->rg_m;
    const unsigned long long un = (unsigned long long)n;
    if (m && !(flags & XB_DOMAINS_SHARES_LIST) && (unsigned long long)m * un <= (unsigned long long)XB_DOMAINS_SHARE_CELLS) {
        // the dense table; its non-empty cells are compacted on the device into (cell, count) pairs and put in order here
        const size_t cells = m * (size_t)n, cap = std::min(cells, c->rg_members);
        DevBuf<unsigned long long> tab, pairs;
        HIPCHK(tab.alloc(cells));
        HIPCHK(pairs.alloc(2 * cap));
        unsigned long long *used = c->counters64 + 8, got = 0;
        HIPCHK(hipMemsetAsync(tab.p, 0, cells * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(used, 0, sizeof(unsigned long long), c->stream));
        const unsigned grid = nblocks((c->N + RG_STEPS - 1) / RG_STEPS);
        if (cells <= RG_SHARE_LDS) k_rg_share_dense<true><<<grid, TPB, 0, c->stream>>>(c->N, c->ptr<int>(BLK_RG_MAP), c->labels, (int)n, (int)cells, tab.p);
        else k_rg_share_dense<false><<<grid, TPB, 0, c->stream>>>(c->N, c->ptr<int>(BLK_RG_MAP), c->labels, (int)n, (int)cells, tab.p);
        k_rg_share_compact<<<nblocks((long long)cells), TPB, 0, c->stream>>>((long long)cells, tab.p, pairs.p, (unsigned long long)cap, used);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&got, used, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (got > cap) return fail(XB_E_STATE, "xb_regions_shares: %llu non-empty cells among %llu members", got, (unsigned long long)cap);
        std::vector<std::pair<unsigned long long, unsigned long long>> h((size_t)got);
        static_assert(sizeof(std::pair<unsigned long long, unsigned long long>) == 16, "the pairs travel as they are");
        if (got)
            if (int rc = staged_d2h(c, h.data(), pairs.p, (size_t)got * 16)) return rc;   // (waits)
        std::sort(h.begin(), h.end());
        for (const auto &e : h) {
            c->rg_sh_comp.push_back((int32_t)(e.first / un));
            c->rg_sh_lab.push_back((int32_t)(e.first % un));
            c->rg_sh_cnt.push_back((int64_t)e.second);
        }
    } else if (m) {
        // the keys of the labelled member voxels, sorted and counted here (as host_critical.h sorts its list)
        const size_t cap = c->rg_members;
        DevBuf<unsigned long long> keys;
        HIPCHK(keys.alloc(cap));
        unsigned long long *used = c->counters64 + 8, got = 0;
        HIPCHK(hipMemsetAsync(used, 0, sizeof(unsigned long long), c->stream));
        k_rg_share_list<<<nblocks(c->N), TPB, 0, c->stream>>>(c->N, c->ptr<int>(BLK_RG_MAP), c->labels, (int)n, keys.p, (unsigned long long)cap, used);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&got, used, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (got > cap) return fail(XB_E_STATE, "xb_regions_shares: %llu labelled voxels among %llu members", got, (unsigned long long)cap);
        std::vector<unsigned long long> h((size_t)got);
        if (got)
            if (int rc = staged_d2h(c, h.data(), keys.p, (size_t)got * sizeof(unsigned long long))) return rc;
        std::sort(h.begin(), h.end());
        for (size_t i = 0; i < h.size();) {
            size_t j = i;
            while (j < h.size() && h[j] == h[i]) j++;
            c->rg_sh_comp.push_back((int32_t)(h[i] / un));
            c->rg_sh_lab.push_back((int32_t)(h[i] % un));
            c->rg_sh_cnt.push_back((int64_t)(j - i));
            i = j;
        }
    }
    c->rg_sh_have = true;
    *n_triplets = (int64_t)c->rg_sh_comp.size();
    return XB_OK;
}

int xb_regions_shares_fetch(xb_ctx *c, int32_t *component, int32_t *label, int64_t *count, int64_t capacity) {
    if (!c || !c->rg_have || !c->rg_sh_have) return fail(XB_E_STATE, "xb_regions_shares_fetch: no result (call xb_regions_shares first)");
    if (!component || !label || !count) return fail(XB_E_ARG, "xb_regions_shares_fetch: null argument");
    const size_t nt = c->rg_sh_comp.size();
    if (capacity < (int64_t)nt) return fail(XB_E_ARG, "xb_regions_shares_fetch: capacity %lld below %lld triplets", (long long)capacity, (long long)nt);
    if (nt) {
        std::memcpy(component, c->rg_sh_comp.data(), nt * sizeof(int32_t));
        std::memcpy(label, c->rg_sh_lab.data(), nt * sizeof(int32_t));
        std::memcpy(count, c->rg_sh_cnt.data(), nt * sizeof(int64_t));
    }
    return XB_OK;
}

int xb_regions_fetch_map(xb_ctx *c, int on_device, void *map) {
    if (!c || !c->rg_have) return fail(XB_E_STATE, "xb_regions_fetch_map: no result (call xb_regions_label first)");
    if (!map) return fail(XB_E_ARG, "xb_regions_fetch_map: null argument");
    HIPCHK(hipSetDevice(c->device));
    const size_t bytes = (size_t)c->N * sizeof(int32_t);
    if (on_device) {
        uintptr_t lo, hi;
        if (int rc = io_check_dense(c, "xb_regions_fetch_map", map, sizeof(int32_t), &lo, &hi)) return rc;
        if (io_overlaps(lo, hi, c->ptr<int>(BLK_RG_MAP), bytes)) return fail(XB_E_ARG, "xb_regions_fetch_map: the destination overlaps the kept map");
        HIPCHK(hipMemcpyAsync(map, c->ptr<int>(BLK_RG_MAP), bytes, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return XB_OK;
    }
    return staged_d2h(c, map, c->ptr<int>(BLK_RG_MAP), bytes);   // (waits)
}

int xb_regions_times(xb_ctx *c, double ms[4]) {
    if (!c || !c->rg_have || !c->rg_timed) return fail(XB_E_STATE, "xb_regions_times: no timed result (call xb_regions_label with XB_DOMAINS_TIMES first)");
    if (!ms) return fail(XB_E_ARG, "xb_regions_times: null argument");
    for (int k = 0; k < 4; k++) ms[k] = c->rg_ms[k];
    return XB_OK;
}
