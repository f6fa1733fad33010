// k_merge.h -- device kernels of libbader_hip.so: merge Bader volumes whose persistence lies below a threshold, round by round
// (xb_merge_basins, host_merge.h; the definition is in include/bader_hip.h and DESIGN.md section 15).  Included by bader_hip.hip
// (one translation unit) after k_adjacency.h, whose facets, key order and direction list it shares.
#pragma once

// Per round two streaming passes over the density and the labels, shaped as k_aj_pass1 / k_aj_pass2 (12 B per voxel each, the
// neighbours from lines the wave or its neighbours fetch anyway), then one thread per label:
//   pass 1  per counting facet: atomic max of the saddle key sk into best[lower]
//   pass 2  per counting facet whose sk is best[lower]: atomic min of `upper` into target[lower]
//   decide  per root: pers = peak - unkey(best), parent = pers < tol ? target : itself; counts the merges; clears best / target
//   hook, jump, keys   the new root of every label by pointer doubling over the parents
// The atomic targets are the n per-label words: no pair table, no hash, no counting pass, no compaction.  Every number is an
// integer, a maximum / minimum of existing bits or one float64 subtraction: integer atomics in any order give the same result.
//
// The current root of a label reaches the passes by a gather through the n-entry table `ent`: 16 bytes per label, the root and
// the key of the root's peak, so that one load per facet side gives both what decides `counts` and what decides `lower`.  Only
// lanes on a boundary of the ORIGINAL labels gather: a wave whose voxels and their active neighbours carry one original label has
// no counting facet whatever the roots are -- one ballot, as in k_aj_pass1, before anything else is read.
#define MG_NONE 0x7fffffff   // target[m] of a root that was `lower` on no counting facet (no label: n <= 2^31 - 1)

struct __attribute__((aligned(16))) MgEnt { unsigned long long pk; int root; int pad; };   // per original label: key(peak[root]), root

// unkey(aj_key(x)) == x, bit for bit
__device__ __forceinline__ double mg_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ (1ull << 63)) : ~k));
}

// max_idx arrives in `parent` (the voxel of each label's maximum); every label starts as its own root
__global__ __launch_bounds__(TPB) void k_mg_init(const double *__restrict__ rho, MgEnt *ent, unsigned long long *best, int *target,
                                                 int *parent, int *mround, double *mpers, int n) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    if (m >= n) return;
    MgEnt e;
    e.pk = aj_key(rho[parent[m]]);
    e.root = (int)m;
    e.pad = 0;
    ent[m] = e;
    best[m] = 0ull;
    target[m] = MG_NONE;
    parent[m] = (int)m;
    mround[m] = -1;
    mpers[m] = __longlong_as_double(0x7ff0000000000000ll);
}

// PASS 1: best[lower] = max sk.  PASS 2 (another launch: best is final): target[lower] = min upper over the facets with sk == best.
// best only rises and target only falls within a launch, so a plain (possibly stale) load can rule a facet out but never in: the
// atomic settles it.  The lanes of a step that still have something to say are peeled by `lower`: a group of AJ_GROUP lanes or
// more reduces with shuffles and its leader issues one atomic, a smaller group issues per lane.
template <int PASS>
__global__ __launch_bounds__(TPB) void k_mg_pass(Grid g, AjDirs D, const double *__restrict__ rho, const int *__restrict__ labels,
                                                 int n, long long N, const MgEnt *__restrict__ ent, unsigned long long *best,
                                                 int *target) {
    long long v = (long long)blockIdx.x * TPB * AJ_PER_THREAD + threadIdx.x;
    const int lane = (int)(threadIdx.x % XB_WAVE);
    for (int it = 0; it < AJ_PER_THREAD; it++, v += TPB) {
        int a = -1;
        AjVoxel p{0, 0, 0};
        bool any = false;
        if (v < N) {
            a = labels[v];
            if ((unsigned)a < (unsigned)n) { p = aj_split(g, v); any = aj_any(g, D, labels, n, p, a); }
        }
        if (!__ballot(any)) continue;                 // the whole wave sees one original label (or none that counts)
        MgEnt ea{0ull, -1, 0};
        unsigned long long ka = 0ull;
        if (any) { ea = ent[a]; ka = aj_key(rho[v]); }
        for (int k = 0; k < D.n; k++) {
            bool cnt = false;
            int lo = -1, up = MG_NONE;
            unsigned long long sk = 0ull;
            if (any) {
                const long long u = aj_neighbour(g, D, k, p);
                const int b = labels[u];
                if (aj_counts(a, b, n)) {
                    const MgEnt eb = ent[b];
                    if (eb.root != ea.root) {
                        const bool b_above = eb.pk > ea.pk || (eb.pk == ea.pk && eb.root < ea.root);
                        lo = b_above ? ea.root : eb.root;
                        up = b_above ? eb.root : ea.root;
                        const unsigned long long kb = aj_key(rho[u]);
                        sk = ka < kb ? ka : kb;
                        cnt = PASS == 1 ? sk > best[lo] : (sk == best[lo] && up < target[lo]);
                    }
                }
            }
            unsigned long long todo = __ballot(cnt);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const int ll = __shfl(lo, leader);
                const bool mine = cnt && lo == ll;
                const unsigned long long grp = __ballot(mine);
                if (__popcll(grp) >= AJ_GROUP) {
                    if (PASS == 1) {
                        unsigned long long m = mine ? sk : 0ull;
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) {
                            const unsigned long long w = __shfl_xor(m, o);
                            m = w > m ? w : m;
                        }
                        if (lane == leader) atomicMax(&best[ll], m);
                    } else {
                        int m = mine ? up : MG_NONE;
#pragma unroll
                        for (int o = 32; o > 0; o >>= 1) m = min(m, __shfl_xor(m, o));
                        if (lane == leader) atomicMin(&target[ll], m);
                    }
                } else if (mine) {
                    if (PASS == 1) atomicMax(&best[lo], sk);
                    else atomicMin(&target[lo], up);
                }
                todo &= ~grp;
            }
        }
    }
}

// one thread per label; only roots act (a label that merged keeps the round and the persistence of its merge)
__global__ __launch_bounds__(TPB) void k_mg_decide(const MgEnt *__restrict__ ent, unsigned long long *best, int *target, int *parent,
                                                   int *mround, double *mpers, int n, double tol, int round,
                                                   unsigned long long *merged) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    bool merges = false;
    if (m < n && ent[m].root == (int)m) {
        const int t = target[m];
        double pers = __longlong_as_double(0x7ff0000000000000ll);
        if (t != MG_NONE) {
            pers = mg_unkey(ent[m].pk) - mg_unkey(best[m]);
            merges = pers < tol;                      // false for a NaN
            best[m] = 0ull;
            target[m] = MG_NONE;
        }
        mpers[m] = pers;
        if (merges) { parent[m] = t; mround[m] = round; }
    }
    const unsigned long long w = __ballot(merges);
    if (w && threadIdx.x % XB_WAVE == 0) atomicAdd(merged, (unsigned long long)__popcll(w));
}

// The new roots.  Before a round ent[m].root is a root r; after it the root of m is the end of the parent chain from r, and every
// link of that chain was made in this round.  hook: root := parent[root].  jump, in place: root := ent[root].root -- whatever a
// racing thread has or has not yet written there is an ancestor, and after i launches the root lies min(2^i, what is left) links
// further up at least: ceil(log2(links)) launches end every chain, of any length.  keys: pk := the new root's.
__global__ __launch_bounds__(TPB) void k_mg_hook(MgEnt *ent, const int *__restrict__ parent, int n) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    if (m < n) ent[m].root = parent[ent[m].root];
}
__global__ __launch_bounds__(TPB) void k_mg_jump(MgEnt *ent, int n) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    if (m >= n) return;
    const int r = ent[m].root, rr = ent[r].root;
    if (rr != r) ent[m].root = rr;
}
__global__ __launch_bounds__(TPB) void k_mg_keys(MgEnt *ent, int n) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    if (m >= n) return;
    const int r = ent[m].root;
    if (r != (int)m) ent[m].pk = ent[r].pk;           // (a root's own key never changes)
}
__global__ __launch_bounds__(TPB) void k_mg_roots(const MgEnt *__restrict__ ent, int *root, int n) {
    const long long m = (long long)blockIdx.x * TPB + threadIdx.x;
    if (m < n) root[m] = ent[m].root;
}
