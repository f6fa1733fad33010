// host_adjacency.h -- host side, part 10: which labels share a surface (k_adjacency.h).  xb_adjacency reads the resident density and
// labels of the whole grid and writes neither.
//
// One block of the context (BLK_AJ, ctx_buffers.h; xb_adjacency_release frees it), in 64-bit words:
//   dense route  the n (n - 1) / 2 entries of AJ_HEAD + n_dirs words
//   hash route   the slots' keys, then the slots' entries
// The occupied entries are compacted on the device in any order into a temporary array of n_pairs rows and sorted by key HERE:
// n_pairs is small next to the grid in every intended use, and a host sort of rows that are downloaded anyway adds no launch.

static void adjacency_forget(xb_ctx *c) {
    c->aj_have = false; c->aj_dirs = 0;
    std::vector<int32_t>().swap(c->aj_a); std::vector<int32_t>().swap(c->aj_b);
    std::vector<int64_t>().swap(c->aj_facets); std::vector<int64_t>().swap(c->aj_sfacet);
    std::vector<double>().swap(c->aj_saddle);
}

extern "C++" {
template <class Route>
static int adjacency_run(xb_ctx *c, const Route &R, const AjDirs &D, int n, size_t n_slots, size_t n_cand,
                         std::vector<unsigned long long> &rows) {
    const Grid &g = c->g;
    const unsigned blocks = nblocks((c->N + AJ_PER_THREAD - 1) / AJ_PER_THREAD);
    const unsigned cand_blocks = (unsigned)std::min<size_t>((n_cand + TPB - 1) / TPB, (size_t)1 << 18);
    unsigned long long *cnt = c->counters64;
    unsigned long long n_pairs = 0;
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
    {
        ScopedTimer timer(c, XB_TIMER_ADJACENCY);
        k_aj_init<<<(unsigned)std::min<size_t>((n_slots * R.stride + TPB - 1) / TPB, (size_t)1 << 18), TPB, 0, c->stream>>>(R.ent, n_slots, R.stride);
        k_aj_pass1<Route><<<blocks, TPB, 0, c->stream>>>(R, g, D, c->rho, c->labels, n, c->N);
        k_aj_pass2<Route><<<blocks, TPB, 0, c->stream>>>(R, g, D, c->rho, c->labels, n, c->N);
        k_aj_occupied<Route><<<cand_blocks, TPB, 0, c->stream>>>(R, n_cand, cnt);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&n_pairs, cnt, sizeof n_pairs, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t width = (size_t)R.stride + 1;
    rows.assign((size_t)n_pairs * width, 0ull);
    if (!n_pairs) return XB_OK;
    DevBuf<unsigned long long> out;
    HIPCHK(out.alloc((size_t)n_pairs * width));
    HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
    {
        ScopedTimer timer(c, XB_TIMER_ADJACENCY);
        k_aj_compact<Route><<<cand_blocks, TPB, 0, c->stream>>>(R, n_cand, cnt, n_pairs, out.p);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(rows.data(), out.p, rows.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}
}  // extern "C++"

// the active directions of a call, checked: each in {-1,0,1}^3 \ {0}, none twice or together with its negative (xb_merge_basins
// takes the same list under the same rules)
static int adjacency_dirs(const char *who, const int32_t *dirs, int n_dirs, AjDirs &D) {
    if (n_dirs < 1 || n_dirs > AJ_MAX_DIRS) return fail(XB_E_ARG, "%s: %d directions (1 .. %d)", who, n_dirs, AJ_MAX_DIRS);
    D.n = n_dirs;
    bool seen[27] = {false};
    for (int k = 0; k < n_dirs; k++) {
        int code = 0, neg = 0;
        for (int j = 0; j < 3; j++) {
            const int d = dirs[3 * k + j];
            if (d < -1 || d > 1) return fail(XB_E_ARG, "%s: direction %d has a step of %d", who, k, d);
            D.d[k][j] = d;
            code = code * 3 + (d + 1);
            neg = neg * 3 + (1 - d);
        }
        if (code == 13) return fail(XB_E_ARG, "%s: direction %d is (0, 0, 0)", who, k);
        if (seen[code] || seen[neg]) return fail(XB_E_ARG, "%s: direction %d is given twice or together with its negative", who, k);
        seen[code] = true;
    }
    for (int k = n_dirs; k < AJ_MAX_DIRS; k++) D.d[k][0] = D.d[k][1] = D.d[k][2] = 0;
    return XB_OK;
}

int xb_adjacency(xb_ctx *c, const int32_t *dirs, int n_dirs, int64_t n, int64_t *n_pairs) {
    ANALYSIS_NEED_GRID("xb_adjacency");
    if (!dirs || !n_pairs) return fail(XB_E_ARG, "xb_adjacency: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_adjacency: %lld labels", (long long)n);
    if (n > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_adjacency: %lld labels exceed %d", (long long)n, XB_INT_MAX);
    AjDirs D;
    if (int rc = adjacency_dirs("xb_adjacency", dirs, n_dirs, D)) return rc;
    if (int rc = analysis_ready(c, "xb_adjacency", "the adjacency needs", NEED_WHOLE | NEED_RHO | NEED_LABELS)) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    const int stride = AJ_HEAD + n_dirs;
    const bool dense = n <= AJ_DENSE;
    size_t n_slots = 0, words = 0;
    if (dense) {
        n_slots = (size_t)n * (size_t)(n - 1) / 2;
        words = n_slots * stride;
    } else {
        unsigned long long facets = 0;
        HIPCHK(hipMemsetAsync(c->counters64, 0, sizeof(unsigned long long), c->stream));
        {
            ScopedTimer timer(c, XB_TIMER_ADJACENCY);
            k_aj_count<<<nblocks((c->N + AJ_PER_THREAD - 1) / AJ_PER_THREAD), TPB, 0, c->stream>>>(c->g, D, c->labels, (int)n, c->N, c->counters64);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&facets, c->counters64, sizeof facets, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        if (facets) {
            n_slots = 1024;
            while (n_slots < 2 * (size_t)facets) n_slots <<= 1;
            words = n_slots * (size_t)(stride + 1);
        }
    }
    c->aj_have = false;
    c->aj_a.clear(); c->aj_b.clear(); c->aj_facets.clear(); c->aj_sfacet.clear(); c->aj_saddle.clear();
    std::vector<unsigned long long> rows;
    if (n_slots) {
        if (int rc = reserve(c, BLK_AJ, words * sizeof(unsigned long long))) return rc;
        unsigned long long *const aj_buf = c->ptr<unsigned long long>(BLK_AJ);
        int rc;
        if (dense) {
            const AjDense R{aj_buf, stride, (int)n};
            rc = adjacency_run(c, R, D, (int)n, n_slots, (size_t)n * (size_t)n, rows);
        } else {
            HIPCHK(hipMemsetAsync(aj_buf, 0xff, n_slots * sizeof(unsigned long long), c->stream));   // every key AJ_EMPTY
            const AjHash R{aj_buf, aj_buf + n_slots, (unsigned long long)(n_slots - 1), stride};
            rc = adjacency_run(c, R, D, (int)n, n_slots, n_slots, rows);
        }
        if (rc) return rc;
    }
    const size_t width = (size_t)stride + 1, np = rows.size() / width;
    std::vector<size_t> order(np);
    for (size_t i = 0; i < np; i++) order[i] = i;
    std::sort(order.begin(), order.end(), [&](size_t x, size_t y) { return rows[x * width] < rows[y * width]; });
    c->aj_a.resize(np); c->aj_b.resize(np); c->aj_saddle.resize(np); c->aj_sfacet.resize(np);
    c->aj_facets.resize(np * (size_t)n_dirs);
    for (size_t i = 0; i < np; i++) {
        const unsigned long long *r = rows.data() + order[i] * width;
        c->aj_a[i] = (int32_t)(r[0] >> 32);
        c->aj_b[i] = (int32_t)(r[0] & 0xffffffffull);
        const unsigned long long key = r[1], bits = (key >> 63) ? (key ^ (1ull << 63)) : ~key;   // aj_key, inverted
        std::memcpy(&c->aj_saddle[i], &bits, sizeof bits);
        c->aj_sfacet[i] = (int64_t)r[2];
        for (int k = 0; k < n_dirs; k++) c->aj_facets[i * (size_t)n_dirs + k] = (int64_t)r[1 + AJ_HEAD + k];
    }
    c->aj_have = true;
    c->aj_dirs = n_dirs;
    *n_pairs = (int64_t)np;
    return XB_OK;
}

int xb_adjacency_fetch(xb_ctx *c, int32_t *a, int32_t *b, int64_t *facets, double *saddle, int64_t *saddle_facet, int64_t capacity) {
    if (!c || !c->aj_have) return fail(XB_E_STATE, "xb_adjacency_fetch: no result (call xb_adjacency first)");
    if (!a || !b || !facets || !saddle || !saddle_facet) return fail(XB_E_ARG, "xb_adjacency_fetch: null argument");
    const size_t np = c->aj_a.size();
    if (capacity < (int64_t)np) return fail(XB_E_ARG, "xb_adjacency_fetch: capacity %lld below %lld pairs", (long long)capacity, (long long)np);
    if (np) {
        std::memcpy(a, c->aj_a.data(), np * sizeof(int32_t));
        std::memcpy(b, c->aj_b.data(), np * sizeof(int32_t));
        std::memcpy(facets, c->aj_facets.data(), np * (size_t)c->aj_dirs * sizeof(int64_t));
        std::memcpy(saddle, c->aj_saddle.data(), np * sizeof(double));
        std::memcpy(saddle_facet, c->aj_sfacet.data(), np * sizeof(int64_t));
    }
    return XB_OK;
}
