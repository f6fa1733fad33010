// k_adjacency.h -- device kernels of libbader_hip.so: which labels share a surface, how many voxel facets of each active
// direction lie on it, and the highest point of the density on it (xb_adjacency, host_adjacency.h; the definition is in
// include/bader_hip.h and DESIGN.md section 14).  Included by bader_hip.hip (one translation unit).
#pragma once

// Two streaming passes over the density and the labels (12 B per voxel each; the neighbours' labels and densities are read from
// lines the wave or its neighbours fetch anyway).  Every number is an integer or a maximum / minimum of existing bits: integer
// atomics in any order give the same result.
//   pass 1  per counting facet: find or create the pair's entry, add to facets[k], atomic max of the saddle key
//   pass 2  per counting facet whose key is the entry's maximum: atomic min of the facet id
//
// A wave whose voxels and their active neighbours carry one label has no counting facet: one ballot, and the step is over.  On a
// boundary the lanes of a step are peeled by (pair, direction): a group of AJ_GROUP lanes or more reduces its maximum with
// shuffles and its leader adds the group's count once, a smaller group adds per lane (as k_moments.h peels labels).
//
// Two routes by the label count n:
//   n <= AJ_DENSE  a triangular table in global memory, entry hi * (hi - 1) / 2 + lo of the pair lo < hi
//   any n          an open-addressing hash table: the key lo << 32 | hi claimed by a 64-bit compare-and-swap, linear probing;
//                  a counting pass sizes it (a power of two >= twice the counting facets, which bound the distinct pairs)
// AJ_DENSE = 256: 32 640 entries of (2 + n_dirs) * 8 bytes -- 1.3 MB with the 3 directions of an orthogonal cell, 2.3 MB with the 7
// of a triclinic one, 3.9 MB with all 13 -- stay below the 4 MiB L2 of one XCD next to the streamed lines.
#define AJ_DENSE 256
#define AJ_MAX_DIRS 13
#define AJ_PER_THREAD 16   // voxels per thread: a block covers TPB * AJ_PER_THREAD consecutive voxels
#define AJ_GROUP 8         // lanes of one (pair, direction) in a step from which a shuffle reduction replaces per-lane atomics
#define AJ_EMPTY (~0ull)                    // a free slot of the hash table (no pair key: lo < 2^31)
#define AJ_NO_FACET 0x7fffffffffffffffull   // the facet id of an entry before pass 2
#define AJ_MISSING (~(size_t)0)

// an entry is AJ_HEAD + n_dirs words: the saddle key, the smallest facet id with that key, facets[k]
#define AJ_HEAD 2

struct AjDirs { int n; int d[AJ_MAX_DIRS][3]; };   // passed by value (uniform reads)

// the total order of the definition: as unsigned integers the keys of doubles compare as the doubles do, -0.0 below +0.0,
// NaNs beyond the infinities of their sign
__device__ __forceinline__ unsigned long long aj_key(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    return b ^ ((b >> 63) ? ~0ull : (1ull << 63));
}

struct AjDense {
    unsigned long long *ent;
    int stride, n;
    __device__ __forceinline__ size_t slot(unsigned long long pk) const {
        const size_t lo = (size_t)(pk >> 32), hi = (size_t)(pk & 0xffffffffull);
        return hi * (hi - 1) / 2 + lo;
    }
    __device__ __forceinline__ size_t find(unsigned long long pk) const { return slot(pk); }
    // the i-th candidate of n * n: its pair key and slot, false when it is none or holds nothing
    __device__ __forceinline__ bool at(size_t i, unsigned long long &pk, size_t &s) const {
        const size_t hi = i / (size_t)n, lo = i - hi * (size_t)n;
        if (lo >= hi) return false;
        pk = ((unsigned long long)lo << 32) | (unsigned long long)hi;
        s = hi * (hi - 1) / 2 + lo;
        bool any = false;
        for (int k = AJ_HEAD; k < stride; k++) any = any || ent[s * stride + k] != 0;
        return any;
    }
};

struct AjHash {
    unsigned long long *hkey;
    unsigned long long *ent;
    unsigned long long mask;   // slots - 1
    int stride;
    __device__ __forceinline__ size_t home(unsigned long long pk) const {
        unsigned long long h = pk;
        h ^= h >> 33; h *= 0xff51afd7ed558ccdull; h ^= h >> 33; h *= 0xc4ceb9fe1a85ec53ull; h ^= h >> 33;
        return (size_t)(h & mask);
    }
    // A slot never changes once it is claimed, so a plain load that shows a key is right; one that shows AJ_EMPTY may be stale and
    // is settled by the compare-and-swap.  At most half the slots are ever claimed: the probe ends.
    __device__ __forceinline__ size_t slot(unsigned long long pk) const {
        size_t i = home(pk);
        for (;;) {
            unsigned long long cur = hkey[i];
            if (cur == AJ_EMPTY) cur = atomicCAS(&hkey[i], AJ_EMPTY, pk);
            if (cur == AJ_EMPTY || cur == pk) return i;
            i = (i + 1) & (size_t)mask;
        }
    }
    __device__ __forceinline__ size_t find(unsigned long long pk) const {   // after pass 1 (another launch): the key is there
        size_t i = home(pk);
        for (;;) {
            const unsigned long long cur = hkey[i];
            if (cur == pk) return i;
            if (cur == AJ_EMPTY) return AJ_MISSING;
            i = (i + 1) & (size_t)mask;
        }
    }
    __device__ __forceinline__ bool at(size_t i, unsigned long long &pk, size_t &s) const {
        pk = hkey[i];
        s = i;
        return pk != AJ_EMPTY;
    }
};

struct AjVoxel { int p0, p1, p2; };

__device__ __forceinline__ AjVoxel aj_split(const Grid &g, long long v) {
    AjVoxel p;
    p.p0 = (int)(v / g.nyz);
    const int r = (int)(v - (long long)p.p0 * g.nyz);
    p.p1 = r / g.nz;
    p.p2 = r - p.p1 * g.nz;
    return p;
}
// the neighbour of p in direction k, wrapped on every axis (steps are -1, 0, 1)
__device__ __forceinline__ long long aj_neighbour(const Grid &g, const AjDirs &D, int k, const AjVoxel &p) {
    int q0 = p.p0 + D.d[k][0], q1 = p.p1 + D.d[k][1], q2 = p.p2 + D.d[k][2];
    q0 += q0 < 0 ? g.nx : 0; q0 -= q0 >= g.nx ? g.nx : 0;
    q1 += q1 < 0 ? g.ny : 0; q1 -= q1 >= g.ny ? g.ny : 0;
    q2 += q2 < 0 ? g.nz : 0; q2 -= q2 >= g.nz ? g.nz : 0;
    return ((long long)q0 * g.ny + q1) * g.nz + q2;
}
__device__ __forceinline__ bool aj_counts(int a, int b, int n) { return (unsigned)b < (unsigned)n && b != a; }

// does any facet of voxel v count?  (a is its label, already known to lie in [0, n))
__device__ __forceinline__ bool aj_any(const Grid &g, const AjDirs &D, const int *__restrict__ labels, int n, const AjVoxel &p, int a) {
    bool any = false;
    for (int k = 0; k < D.n; k++) any = any || aj_counts(a, labels[aj_neighbour(g, D, k, p)], n);
    return any;
}

// the counting pass of the hash route: the number of counting facets
__global__ __launch_bounds__(TPB) void k_aj_count(Grid g, AjDirs D, const int *__restrict__ labels, int n, long long N,
                                                  unsigned long long *total) {
    long long v = (long long)blockIdx.x * TPB * AJ_PER_THREAD + threadIdx.x;
    unsigned int mine = 0;
    for (int it = 0; it < AJ_PER_THREAD; it++, v += TPB) {
        if (v >= N) break;
        const int a = labels[v];
        if ((unsigned)a >= (unsigned)n) continue;
        const AjVoxel p = aj_split(g, v);
        for (int k = 0; k < D.n; k++) mine += aj_counts(a, labels[aj_neighbour(g, D, k, p)], n) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if (threadIdx.x % XB_WAVE == 0 && mine) atomicAdd(total, (unsigned long long)mine);
}

__global__ __launch_bounds__(TPB) void k_aj_init(unsigned long long *ent, size_t n_slots, int stride) {
    const size_t total = n_slots * (size_t)stride;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += (size_t)gridDim.x * TPB)
        ent[i] = (i % (size_t)stride) == 1 ? AJ_NO_FACET : 0ull;
}

template <class Route>
__device__ __forceinline__ void aj_add(const Route &R, unsigned long long pk, int k, unsigned int c, unsigned long long m) {
    unsigned long long *e = R.ent + R.slot(pk) * (size_t)R.stride;
    atomicAdd(&e[AJ_HEAD + k], (unsigned long long)c);
    atomicMax(&e[0], m);
}

template <class Route>
__global__ __launch_bounds__(TPB) void k_aj_pass1(Route R, Grid g, AjDirs D, const double *__restrict__ rho,
                                                  const int *__restrict__ labels, int n, long long N) {
    long long v = (long long)blockIdx.x * TPB * AJ_PER_THREAD + threadIdx.x;
    const int lane = (int)(threadIdx.x % XB_WAVE);
    for (int it = 0; it < AJ_PER_THREAD; it++, v += TPB) {
        int a = -1;
        AjVoxel p{0, 0, 0};
        bool any = false;
        if (v < N) {
            a = labels[v];
            if ((unsigned)a < (unsigned)n) { p = aj_split(g, v); any = aj_any(g, D, labels, n, p, a); }
            else a = -1;
        }
        if (!__ballot(any)) continue;                 // the whole wave sees one label (or none that counts)
        const unsigned long long ka = any ? aj_key(rho[v]) : 0ull;
        for (int k = 0; k < D.n; k++) {
            bool cnt = false;
            unsigned long long pk = AJ_EMPTY, sk = 0ull;
            if (any) {
                const long long u = aj_neighbour(g, D, k, p);
                const int b = labels[u];
                if (aj_counts(a, b, n)) {
                    cnt = true;
                    const unsigned int lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
                    pk = ((unsigned long long)lo << 32) | (unsigned long long)hi;
                    const unsigned long long kb = aj_key(rho[u]);
                    sk = ka < kb ? ka : kb;
                }
            }
            unsigned long long todo = __ballot(cnt);
            while (todo) {
                const int leader = __ffsll((long long)todo) - 1;
                const unsigned long long lk = __shfl(pk, leader);
                const bool mine = cnt && pk == lk;
                const unsigned long long grp = __ballot(mine);
                const unsigned int c = (unsigned int)__popcll(grp);
                if (c >= AJ_GROUP) {
                    unsigned long long m = mine ? sk : 0ull;
#pragma unroll
                    for (int o = 32; o > 0; o >>= 1) {
                        const unsigned long long w = __shfl_xor(m, o);
                        m = w > m ? w : m;
                    }
                    if (lane == leader) aj_add(R, lk, k, c, m);
                } else if (mine)
                    aj_add(R, pk, k, 1u, sk);
                todo &= ~grp;
            }
        }
    }
}

// pass 2: the entries hold their final keys.  A facet id can lower the entry only if it is below what a (possibly stale) load
// of the entry shows: the entry only ever falls.
template <class Route>
__global__ __launch_bounds__(TPB) void k_aj_pass2(Route R, Grid g, AjDirs D, const double *__restrict__ rho,
                                                  const int *__restrict__ labels, int n, long long N) {
    long long v = (long long)blockIdx.x * TPB * AJ_PER_THREAD + threadIdx.x;
    for (int it = 0; it < AJ_PER_THREAD; it++, v += TPB) {
        int a = -1;
        AjVoxel p{0, 0, 0};
        bool any = false;
        if (v < N) {
            a = labels[v];
            if ((unsigned)a < (unsigned)n) { p = aj_split(g, v); any = aj_any(g, D, labels, n, p, a); }
        }
        if (!__ballot(any)) continue;
        if (!any) continue;
        const unsigned long long ka = aj_key(rho[v]);
        for (int k = 0; k < D.n; k++) {
            const long long u = aj_neighbour(g, D, k, p);
            const int b = labels[u];
            if (!aj_counts(a, b, n)) continue;
            const unsigned int lo = (unsigned)min(a, b), hi = (unsigned)max(a, b);
            const unsigned long long pk = ((unsigned long long)lo << 32) | (unsigned long long)hi;
            const unsigned long long kb = aj_key(rho[u]);
            const unsigned long long sk = ka < kb ? ka : kb;
            const size_t s = R.find(pk);
            if (s == AJ_MISSING) continue;
            unsigned long long *e = R.ent + s * (size_t)R.stride;
            const unsigned long long f = (unsigned long long)v * 8ull + (unsigned long long)k;
            if (e[0] == sk && f < e[1]) atomicMin(&e[1], f);
        }
    }
}

// the occupied entries, counted and then copied out in any order (the host sorts them by key): a row of `out` is the pair key and
// the entry's words
template <class Route>
__global__ __launch_bounds__(TPB) void k_aj_occupied(Route R, size_t n_cand, unsigned long long *count) {
    unsigned long long pk;
    size_t s;
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_cand; i += (size_t)gridDim.x * TPB) mine += R.at(i, pk, s) ? 1u : 0u;
    if (mine) atomicAdd(count, (unsigned long long)mine);
}
template <class Route>
__global__ __launch_bounds__(TPB) void k_aj_compact(Route R, size_t n_cand, unsigned long long *count, unsigned long long capacity,
                                                    unsigned long long *__restrict__ out) {
    unsigned long long pk;
    size_t s;
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_cand; i += (size_t)gridDim.x * TPB) {
        if (!R.at(i, pk, s)) continue;
        const unsigned long long row = atomicAdd(count, 1ull);
        if (row >= capacity) continue;
        unsigned long long *o = out + row * (size_t)(R.stride + 1);
        o[0] = pk;
        for (int k = 0; k < R.stride; k++) o[1 + k] = R.ent[s * (size_t)R.stride + k];
    }
}
