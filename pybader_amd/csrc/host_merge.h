// host_merge.h -- host side, part 11: merge Bader volumes below a persistence threshold (k_merge.h).  xb_merge_basins reads the
// resident density and labels of the whole grid and writes neither.
//
// One block of the context (BLK_MG, ctx_buffers.h; xb_merge_release frees it), MG_BYTES = 44 bytes per label:
//   ent 16   best 8   merge_persistence 8   target 4   parent 4   merge_round 4
// One host wait per round, for the number of merges: it ends the loop and sizes the pointer doubling.
#define MG_BYTES 44

static void merge_forget(xb_ctx *c) {
    c->mg_have = false;
    std::vector<int32_t>().swap(c->mg_root); std::vector<int32_t>().swap(c->mg_round);
    std::vector<double>().swap(c->mg_pers);
}

int xb_merge_basins(xb_ctx *c, const int32_t *dirs, int n_dirs, int64_t n, const int64_t *max_idx, double tol, int64_t max_rounds,
                    int64_t *rounds, int64_t *n_survivors, int *converged) {
    ANALYSIS_NEED_GRID("xb_merge_basins");
    if (!dirs || !max_idx || !rounds || !n_survivors || !converged) return fail(XB_E_ARG, "xb_merge_basins: null argument");
    if (n < 1) return fail(XB_E_ARG, "xb_merge_basins: %lld labels", (long long)n);
    if (n > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_merge_basins: %lld labels exceed %d", (long long)n, XB_INT_MAX);
    AjDirs D;
    if (int rc = adjacency_dirs("xb_merge_basins", dirs, n_dirs, D)) return rc;
    if (max_rounds < 1) return fail(XB_E_ARG, "xb_merge_basins: %lld rounds", (long long)max_rounds);
    if (!(tol >= 0.)) return fail(XB_E_ARG, "xb_merge_basins: the threshold %g is negative or not a number", tol);
    if (int rc = analysis_ready(c, "xb_merge_basins", "the merge needs", NEED_WHOLE | NEED_RHO | NEED_LABELS)) return rc;
    std::vector<int> idx((size_t)n);
    for (int64_t m = 0; m < n; m++) {
        if (max_idx[m] < 0 || max_idx[m] >= c->N)
            return fail(XB_E_ARG, "xb_merge_basins: the maximum of label %lld is voxel %lld of %lld", (long long)m, (long long)max_idx[m], c->N);
        idx[(size_t)m] = (int)max_idx[m];
    }
    HIPCHK(hipSetDevice(c->device));
    if (int rc = settle_labels(c)) return rc;
    c->mg_have = false;
    if (int rc = reserve(c, BLK_MG, (size_t)n * MG_BYTES)) return rc;
    // carved by the capacity, widest first: every array stays aligned to its element
    const size_t cap = c->bytes(BLK_MG) / MG_BYTES;
    MgEnt *ent = c->ptr<MgEnt>(BLK_MG);
    unsigned long long *best = reinterpret_cast<unsigned long long *>(ent + cap);
    double *mpers = reinterpret_cast<double *>(best + cap);
    int *target = reinterpret_cast<int *>(mpers + cap);
    int *parent = target + cap, *mround = parent + cap;
    const int nl = (int)n;
    const unsigned lblocks = nblocks(n), vblocks = nblocks((c->N + AJ_PER_THREAD - 1) / AJ_PER_THREAD);
    unsigned long long *cnt = c->counters64;
    HIPCHK(hipMemcpyAsync(parent, idx.data(), (size_t)n * sizeof(int), hipMemcpyHostToDevice, c->stream));
    {
        ScopedTimer timer(c, XB_TIMER_MERGE);
        k_mg_init<<<lblocks, TPB, 0, c->stream>>>(c->rho, ent, best, target, parent, mround, mpers, nl);
    }
    HIPCHK(hipGetLastError());
    int64_t done = 0, merged_total = 0;
    bool settled = false;
    while (done < max_rounds) {
        unsigned long long merged = 0;
        HIPCHK(hipMemsetAsync(cnt, 0, sizeof(unsigned long long), c->stream));
        {
            ScopedTimer timer(c, XB_TIMER_MERGE);
            k_mg_pass<1><<<vblocks, TPB, 0, c->stream>>>(c->g, D, c->rho, c->labels, nl, c->N, ent, best, target);
            k_mg_pass<2><<<vblocks, TPB, 0, c->stream>>>(c->g, D, c->rho, c->labels, nl, c->N, ent, best, target);
            k_mg_decide<<<lblocks, TPB, 0, c->stream>>>(ent, best, target, parent, mround, mpers, nl, tol, (int)done, cnt);
        }
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(&merged, cnt, sizeof merged, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        done++;
        settled = merged == 0;
        if (settled) break;
        merged_total += (int64_t)merged;
        {
            // the longest chain of this round's links has at most `merged` of them
            ScopedTimer timer(c, XB_TIMER_MERGE);
            k_mg_hook<<<lblocks, TPB, 0, c->stream>>>(ent, parent, nl);
            for (unsigned long long reach = 1; reach < merged; reach <<= 1) k_mg_jump<<<lblocks, TPB, 0, c->stream>>>(ent, nl);
            k_mg_keys<<<lblocks, TPB, 0, c->stream>>>(ent, nl);
        }
        HIPCHK(hipGetLastError());
    }
    // the roots go out through `parent`, which no later call reads (the next one starts over)
    c->mg_root.resize((size_t)n); c->mg_round.resize((size_t)n); c->mg_pers.resize((size_t)n);
    {
        ScopedTimer timer(c, XB_TIMER_MERGE);
        k_mg_roots<<<lblocks, TPB, 0, c->stream>>>(ent, parent, nl);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(c->mg_root.data(), parent, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->mg_round.data(), mround, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->mg_pers.data(), mpers, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->mg_have = true;
    *rounds = done;
    *n_survivors = n - merged_total;
    *converged = settled ? 1 : 0;
    return XB_OK;
}

int xb_merge_fetch(xb_ctx *c, int32_t *root, int32_t *merge_round, double *merge_persistence, int64_t capacity) {
    if (!c || !c->mg_have) return fail(XB_E_STATE, "xb_merge_fetch: no result (call xb_merge_basins first)");
    if (!root || !merge_round || !merge_persistence) return fail(XB_E_ARG, "xb_merge_fetch: null argument");
    const size_t n = c->mg_root.size();
    if (capacity < (int64_t)n) return fail(XB_E_ARG, "xb_merge_fetch: capacity %lld below %lld labels", (long long)capacity, (long long)n);
    std::memcpy(root, c->mg_root.data(), n * sizeof(int32_t));
    std::memcpy(merge_round, c->mg_round.data(), n * sizeof(int32_t));
    std::memcpy(merge_persistence, c->mg_pers.data(), n * sizeof(double));
    return XB_OK;
}
