// host_critical.h -- host side, part 13: the critical points of the density and the bond graph (k_critical.h).  Both calls read the
// resident density (xb_critical_bonds the resident labels too) of the whole grid and write neither.
//
// Two blocks of the context (ctx_buffers.h; xb_critical_release frees them):
//   BLK_CP_LUT    the 16 384 bytes of xb_critical_lut, uploaded on the first call that uses the table
//   BLK_CP_LIST   the records of the last xb_critical_points call, in the order the workgroups claimed their slots.  It starts at
//             N / 64 + 4096 records; a call that finds more learns the exact number from its own counter, grows the list to it and
//             runs the pass once more: the list is sized from a count and never cut short.
// The records are sorted HERE (lin is their high word), as host_adjacency.h sorts its pairs; xb_critical_bonds reduces the bond
// rows per pair here as well: a count, a maximum of keys and a minimum of indices.

static void critical_forget(xb_ctx *c) {
    c->cp_n = 0;
    c->cp_have = false; c->cb_have = false; c->cp_bond_voxels = 0;
    std::vector<unsigned long long>().swap(c->cp_rec);
    std::vector<int32_t>().swap(c->cb_a); std::vector<int32_t>().swap(c->cb_b);
    std::vector<int64_t>().swap(c->cb_saddles); std::vector<int64_t>().swap(c->cb_voxel);
    std::vector<double>().swap(c->cb_rho);
}

static const uint8_t *critical_table() {
    static uint8_t tab[XB_CRITICAL_LUT_SIZE];
    static bool made = false;
    static std::mutex mu;
    std::lock_guard<std::mutex> lock(mu);
    if (!made) {
        for (unsigned L = 0; L < XB_CRITICAL_LUT_SIZE; L++) tab[L] = (uint8_t)cp_classify(L);
        made = true;
    }
    return tab;
}

int xb_critical_lut(uint8_t *out) {
    if (!out) return fail(XB_E_ARG, "xb_critical_lut: null argument");
    std::memcpy(out, critical_table(), XB_CRITICAL_LUT_SIZE);
    return XB_OK;
}

int xb_critical_points(xb_ctx *c, double vac_tol, int flags, int64_t counts[6], int64_t *n_list) {
    ANALYSIS_NEED_GRID("xb_critical_points");
    if (!counts || !n_list) return fail(XB_E_ARG, "xb_critical_points: null argument");
    if (flags & ~XB_CRITICAL_FLOOD) return fail(XB_E_ARG, "xb_critical_points: unknown flag bits 0x%x", flags & ~XB_CRITICAL_FLOOD);
    if (int rc = analysis_ready(c, "xb_critical_points", "the critical points need", NEED_WHOLE | NEED_RHO)) return rc;
    const Grid &g = c->g;
    HIPCHK(hipSetDevice(c->device));
    c->cp_have = false; c->cb_have = false;
    const bool flood = (flags & XB_CRITICAL_FLOOD) != 0;
    if (!flood && !c->bytes(BLK_CP_LUT)) {
        if (int rc = reserve(c, BLK_CP_LUT, XB_CRITICAL_LUT_SIZE)) return rc;
        HIPCHK(hipMemcpyAsync(c->ptr<void>(BLK_CP_LUT), critical_table(), XB_CRITICAL_LUT_SIZE, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));   // (the table is static, but pageable: the copy is staged before this returns anyway)
    }
    const long long tiles = (long long)((g.nx + CP_TX - 1) / CP_TX) * ((g.ny + CP_TY - 1) / CP_TY) * ((g.nz + CP_TZ - 1) / CP_TZ);   // (at most N)
    unsigned long long cnt[7] = {0, 0, 0, 0, 0, 0, 0}, cp_cap = 0;
    for (int pass = 0; pass < 2; pass++) {
        const size_t want = pass == 0 ? (size_t)(c->N / 64 + 4096) : (size_t)cnt[6];
        if (int rc = reserve(c, BLK_CP_LIST, want * sizeof(unsigned long long))) return rc;
        cp_cap = c->bytes(BLK_CP_LIST) / sizeof(unsigned long long);
        HIPCHK(hipMemsetAsync(c->counters64, 0, sizeof cnt, c->stream));
        k_critical<<<(unsigned)tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, flood ? nullptr : c->ptr<unsigned char>(BLK_CP_LUT), vac_tol == vac_tol ? 1 : 0,
                                                          vac_tol, c->ptr<unsigned long long>(BLK_CP_LIST), cp_cap, c->counters64);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(cnt, c->counters64, sizeof cnt, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (cnt[6] <= cp_cap) break;
        if (pass == 1) return fail(XB_E_STATE, "xb_critical_points: %llu records after %llu were counted", cnt[6], cp_cap);
    }
    c->cp_n = (size_t)cnt[6];
    c->cp_rec.resize(c->cp_n);
    if (c->cp_n) {
        if (int rc = staged_d2h(c, c->cp_rec.data(), c->ptr<unsigned long long>(BLK_CP_LIST), c->cp_n * sizeof(unsigned long long))) return rc;
        std::sort(c->cp_rec.begin(), c->cp_rec.end());
    }
    for (int k = 0; k < XB_CRITICAL_COUNTS; k++) counts[k] = (int64_t)cnt[k];
    c->cp_bond_voxels = (size_t)cnt[XB_CRITICAL_BOND_VOXELS];
    c->cp_have = true;
    *n_list = (int64_t)c->cp_n;
    return XB_OK;
}

int xb_critical_fetch(xb_ctx *c, int64_t *lin, uint16_t *lower_mask, uint8_t *ring, uint8_t *bond, int64_t capacity) {
    if (!c || !c->cp_have) return fail(XB_E_STATE, "xb_critical_fetch: no result (call xb_critical_points first)");
    if (!lin || !lower_mask || !ring || !bond) return fail(XB_E_ARG, "xb_critical_fetch: null argument");
    const size_t n = c->cp_rec.size();
    if (capacity < (int64_t)n) return fail(XB_E_ARG, "xb_critical_fetch: capacity %lld below %lld records", (long long)capacity, (long long)n);
    for (size_t i = 0; i < n; i++) {
        const unsigned long long r = c->cp_rec[i];
        lin[i] = (int64_t)(r >> 32);
        lower_mask[i] = (uint16_t)((r >> 8) & XB_CRITICAL_FULL);
        ring[i] = (uint8_t)(r & 15ull);
        bond[i] = (uint8_t)((r >> 4) & 15ull);
    }
    return XB_OK;
}

int xb_critical_bonds(xb_ctx *c, int64_t n, int64_t *n_pairs, int64_t *same_basin) {
    ANALYSIS_NEED_GRID("xb_critical_bonds");
    if (!n_pairs || !same_basin) return fail(XB_E_ARG, "xb_critical_bonds: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_critical_bonds: %lld labels", (long long)n);
    if (int rc = analysis_ready(c, "xb_critical_bonds", "the bond graph needs", NEED_WHOLE | NEED_RHO | NEED_LABELS)) return rc;
    const Grid &g = c->g;
    if (!c->cp_have) return fail(XB_E_STATE, "xb_critical_bonds: no critical points of the resident density (call xb_critical_points first)");
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    c->cb_have = false;
    c->cb_a.clear(); c->cb_b.clear(); c->cb_saddles.clear(); c->cb_voxel.clear(); c->cb_rho.clear();
    const size_t nb = c->cp_bond_voxels;
    std::vector<unsigned long long> rows(nb * CP_BOND_ROW);
    if (nb) {
        DevBuf<unsigned long long> out;
        unsigned long long *count = c->counters64 + 8, got = 0;
        HIPCHK(out.alloc(nb * CP_BOND_ROW));
        HIPCHK(hipMemsetAsync(count, 0, sizeof(unsigned long long), c->stream));
        k_critical_bonds<<<nblocks((long long)c->cp_n), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, c->rho, c->labels, c->ptr<unsigned long long>(BLK_CP_LIST), (unsigned long long)c->cp_n,
                                                                         out.p, (unsigned long long)nb, count);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&got, count, sizeof got, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(rows.data(), out.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (got != nb) return fail(XB_E_STATE, "xb_critical_bonds: %llu bond voxels in the list, %llu were counted", got, (unsigned long long)nb);
    }
    // per bond voxel: the distinct basins in [0, n) among its tops; every pair of them gains a saddle
    struct Saddle { unsigned long long pair, key; long long lin; };
    std::vector<Saddle> sad;
    long long same = 0;
    for (size_t i = 0; i < nb; i++) {
        const unsigned long long *r = rows.data() + i * CP_BOND_ROW;
        int32_t lab[6], d[6];
        std::memcpy(lab, r + 2, sizeof lab);
        int nd = 0;
        for (int k = 0; k < 6; k++) {
            if (lab[k] < 0 || (int64_t)lab[k] >= n) continue;   // (CP_NONE is negative)
            bool seen = false;
            for (int j = 0; j < nd; j++) seen = seen || d[j] == lab[k];
            if (!seen) d[nd++] = lab[k];
        }
        if (nd == 1) same++;
        for (int p = 0; p < nd; p++)
            for (int q = p + 1; q < nd; q++) {
                const unsigned long long lo = (unsigned long long)std::min(d[p], d[q]), hi = (unsigned long long)std::max(d[p], d[q]);
                sad.push_back({(lo << 32) | hi, r[0], (long long)r[1]});
            }
    }
    // ascending pair; inside a pair the greatest key first, and the smallest index among equal keys
    std::sort(sad.begin(), sad.end(), [](const Saddle &x, const Saddle &y) {
        if (x.pair != y.pair) return x.pair < y.pair;
        if (x.key != y.key) return x.key > y.key;
        return x.lin < y.lin;
    });
    for (size_t i = 0; i < sad.size();) {
        size_t j = i;
        while (j < sad.size() && sad[j].pair == sad[i].pair) j++;
        const unsigned long long key = sad[i].key, bits = (key >> 63) ? (key ^ (1ull << 63)) : ~key;   // aj_key, inverted
        double rho_b;
        std::memcpy(&rho_b, &bits, sizeof bits);
        c->cb_a.push_back((int32_t)(sad[i].pair >> 32));
        c->cb_b.push_back((int32_t)(sad[i].pair & 0xffffffffull));
        c->cb_saddles.push_back((int64_t)(j - i));
        c->cb_rho.push_back(rho_b);
        c->cb_voxel.push_back((int64_t)sad[i].lin);
        i = j;
    }
    c->cb_have = true;
    *n_pairs = (int64_t)c->cb_a.size();
    *same_basin = (int64_t)same;
    return XB_OK;
}

int xb_critical_bonds_fetch(xb_ctx *c, int32_t *a, int32_t *b, int64_t *saddles, double *rho_b, int64_t *voxel, int64_t capacity) {
    if (!c || !c->cb_have) return fail(XB_E_STATE, "xb_critical_bonds_fetch: no result (call xb_critical_bonds first)");
    if (!a || !b || !saddles || !rho_b || !voxel) return fail(XB_E_ARG, "xb_critical_bonds_fetch: null argument");
    const size_t np = c->cb_a.size();
    if (capacity < (int64_t)np) return fail(XB_E_ARG, "xb_critical_bonds_fetch: capacity %lld below %lld pairs", (long long)capacity, (long long)np);
    if (np) {
        std::memcpy(a, c->cb_a.data(), np * sizeof(int32_t));
        std::memcpy(b, c->cb_b.data(), np * sizeof(int32_t));
        std::memcpy(saddles, c->cb_saddles.data(), np * sizeof(int64_t));
        std::memcpy(rho_b, c->cb_rho.data(), np * sizeof(double));
        std::memcpy(voxel, c->cb_voxel.data(), np * sizeof(int64_t));
    }
    return XB_OK;
}
