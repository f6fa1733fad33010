// k_regions.h -- device kernels of libbader_hip.so: connected components of a periodic voxel mask under the Freudenthal adjacency
// -- the islands of a level set, the pockets below it, the domains of the NCI region (xb_regions_label / xb_regions_sums /
// xb_regions_shares, host_regions.h; the definition is in include/bader_hip.h and DESIGN.md section 22).  Included by bader_hip.hip
// (one translation unit) behind k_nci.h and k_isosurface.h, whose voxel routine, tile, wave sums and scan kernels it uses.
#pragma once

// The map holds a forest over the linear C-order indices: parent[v] <= v for a member, -1 outside; a root is its own parent and
// the smallest index of its set.  Two routes build it, both to the same final map (the root of a set is its smallest member
// whatever the order of the unions):
//   tiles    k_rg_tile<., true>: a workgroup takes an ST_TX x ST_TY x ST_TZ tile, forms its membership bits (a row mask along x
//            per thread), runs a union-find over the tile's 2048 voxels in LDS along the seven forward offsets that stay inside the
//            tile, and writes parent[v] = lin(root).  k_rg_link<false> then unions across every tile face, the grid's periodic wrap
//            and the ragged last tiles included, in global memory.
//   global   (XB_DOMAINS_GLOBAL) k_rg_tile<., false> writes parent[v] = v; k_rg_link<true> unions every member with its seven
//            forward neighbours in global memory.
// k_rg_flatten points every member at its root.  The numbering is a count of the roots per run of RG_BLOCK consecutive indices,
// the scan of k_isosurface.h (three launches), an emit pass and a pass that rewrites the map: no kernel waits for another
// workgroup.
//
// The union (rg_union) is lock-free and never waits: find both roots, stop if they are equal, atomicMin(&parent[hi], lo); when the
// returned value was hi the link is made, otherwise hi had a parent already -- the returned value -- and the loop goes on with
// that value and lo.  Parents only ever decrease, so a stale read of parent[] is still an ancestor in the same set: plain loads
// decide nothing, only the return value of atomicMin says that a link was made.
//
// LDS per workgroup: the tile's parents, 2048 x 4 B = 8 192 B; in NCI mode through tiles the staged density as well (27 200 B):
// 35 392 B, four workgroups per compute unit.
#define RG_BLOCK ISO_BLOCK
#define RG_TILE (ST_TX * ST_TY * ST_TZ)
#define RG_STEPS 16           // runs of TPB voxels a workgroup of the sums and the shares walks
#define RG_SHARE_LDS 1024     // cells of the share table up to which a workgroup counts in LDS (4 096 B)
#define RG_SRC_FIELD 0        // membership: field >= level, or field < level
#define RG_SRC_NCI_TILE 1     // ... the NCI region, the 19 values from the staged tile
#define RG_SRC_NCI_GATHER 2   // ... the NCI region, the 19 values from global memory
static_assert(RG_BLOCK == TPB, "one voxel of a run per thread");
static_assert((ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2) * 8 + RG_TILE * 4 <= 160 * 1024 / 4, "four workgroups per compute unit");

__device__ __forceinline__ int rg_load(const int *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }
__device__ __forceinline__ void rg_store(int *p, int v) { __atomic_store_n(p, v, __ATOMIC_RELAXED); }
__device__ __forceinline__ int rg_find(const int *parent, int a) {
    for (int q = rg_load(parent + a); q != a; q = rg_load(parent + a)) a = q;
    return a;
}
// a and b are members (parent >= 0); `parent` is the map in global memory or a tile's parents in LDS
__device__ __forceinline__ void rg_union(int *parent, int a, int b) {
    for (;;) {
        a = rg_find(parent, a);
        b = rg_find(parent, b);
        if (a == b) return;
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = atomicMin(parent + hi, lo);
        if (old == hi) return;   // hi was a root and hangs below lo now
        a = old;                 // hi had the parent `old` (it points at min(old, lo) now): old and lo are still to be joined
        b = lo;
    }
}
// the NCI region's predicate: the first three comparisons of nci_key
__device__ __forceinline__ bool rg_nci_inside(const NciVoxel &v, const NciCuts &C) {
    return (v.rho > 0.) && (v.q < C.t_cut * v.r8) && (v.rho < C.rho_cut);
}
__device__ __forceinline__ bool rg_field_inside(double f, double level, int below) { return below ? f < level : f >= level; }   // (a NaN: neither)

// SRC: where the membership comes from (RG_SRC_*); f: the field, or the resident density for the NCI region.
// LOCAL: the union-find of the tile in LDS, parent[v] = lin(root of v in the tile); otherwise parent[v] = v.  -1 outside.
template <int SRC, bool LOCAL>
__global__ __launch_bounds__(TPB) void k_rg_tile(int nx, int ny, int nz, const double *__restrict__ f, double level, int below, StCoeffs K,
                                                 NciCuts C, int *__restrict__ parent) {
    __shared__ StTile s_rho[SRC == RG_SRC_NCI_TILE ? ST_TX + 2 : 1];   // (one plane nobody uses otherwise)
    __shared__ int s_par[LOCAL ? RG_TILE : 1];
    int x0, y0, z0;
    if (SRC == RG_SRC_NCI_TILE)
        st_stage(s_rho, nx, ny, nz, f, x0, y0, z0);
    else {
        const int tiles_z = (nz + ST_TZ - 1) / ST_TZ, tiles_y = (ny + ST_TY - 1) / ST_TY;
        x0 = (int)(blockIdx.x / (tiles_z * tiles_y)) * ST_TX;
        y0 = (int)((blockIdx.x / tiles_z) % tiles_y) * ST_TY;
        z0 = (int)(blockIdx.x % tiles_z) * ST_TZ;
    }
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool column = y < ny && z < nz;
    unsigned int bits = 0;   // bit tx: the voxel (tx, ty, tz) of the tile is a member
#pragma unroll 2
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        if (!column || x >= nx) break;
        bool in;
        if (SRC == RG_SRC_NCI_TILE) {
            const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
            in = rg_nci_inside(nci_voxel(r, K), C);
        } else if (SRC == RG_SRC_NCI_GATHER) {
            const StGatherReader r(f, x, y, z, nx, ny, nz);
            in = rg_nci_inside(nci_voxel(r, K), C);
        } else
            in = rg_field_inside(f[((long long)x * ny + y) * nz + z], level, below);
        bits |= (in ? 1u : 0u) << tx;
    }
    if (!LOCAL) {
        for (int tx = 0; tx < ST_TX && column && x0 + tx < nx; tx++) {
            const int lin = ((x0 + tx) * ny + y) * nz + z;   // (N <= 2^31 - 1: the host checks)
            parent[lin] = ((bits >> tx) & 1u) ? lin : -1;
        }
        return;
    }
    const int l0 = ty * ST_TZ + tz;   // the local index of (tx, ty, tz) is tx * TPB + l0: in the order of lin
#pragma unroll
    for (int tx = 0; tx < ST_TX; tx++) s_par[tx * TPB + l0] = ((bits >> tx) & 1u) ? tx * TPB + l0 : -1;
    const bool wave_has = __ballot(bits != 0u) != 0ull;   // a wave without members has nothing to join
    __syncthreads();
    if (wave_has) {
        for (int tx = 0; tx < ST_TX; tx++) {
            if (!((bits >> tx) & 1u)) continue;
#pragma unroll
            for (int k = 1; k <= 7; k++) {   // d = (k >> 2, (k >> 1) & 1, k & 1): d_0 .. d_6 of the definition
                const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
                if (tx + dx >= ST_TX || x0 + tx + dx >= nx || ty + dy >= ST_TY || y + dy >= ny || tz + dz >= ST_TZ || z + dz >= nz) continue;
                const int u = (tx + dx) * TPB + (ty + dy) * ST_TZ + (tz + dz);
                if (rg_load(s_par + u) >= 0) rg_union(s_par, tx * TPB + l0, u);
            }
        }
    }
    __syncthreads();
    for (int tx = 0; tx < ST_TX && column && x0 + tx < nx; tx++) {
        const int lin = ((x0 + tx) * ny + y) * nz + z;
        int out = -1;
        if ((bits >> tx) & 1u) {
            const int r = rg_find(s_par, tx * TPB + l0);
            out = ((x0 + r / TPB) * ny + (y0 + (r / ST_TZ) % ST_TY)) * nz + (z0 + r % ST_TZ);
        }
        parent[lin] = out;
    }
}

// ALL: every member joins its seven forward neighbours; otherwise only along the offsets that leave its tile (or the grid)
template <bool ALL>
__global__ __launch_bounds__(TPB) void k_rg_link(int nx, int ny, int nz, int *parent) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    if (v >= nx * nyz) return;
    const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
    const bool ex = ALL || x % ST_TX == ST_TX - 1 || x == nx - 1, ey = ALL || y % ST_TY == ST_TY - 1 || y == ny - 1,
               ez = ALL || z % ST_TZ == ST_TZ - 1 || z == nz - 1;
    if (!(ex || ey || ez)) return;
    if (rg_load(parent + v) < 0) return;
#pragma unroll
    for (int k = 1; k <= 7; k++) {
        const int dx = k >> 2, dy = (k >> 1) & 1, dz = k & 1;
        if (!((dx && ex) || (dy && ey) || (dz && ez))) continue;
        const int ux = x + dx < nx ? x + dx : 0, uy = y + dy < ny ? y + dy : 0, uz = z + dz < nz ? z + dz : 0;
        const int u = (ux * ny + uy) * nz + uz;
        if (u == (int)v) continue;   // (the offset wraps onto the voxel itself: axes of length 1)
        if (rg_load(parent + u) >= 0) rg_union(parent, (int)v, u);
    }
}

__global__ __launch_bounds__(TPB) void k_rg_flatten(long long N, int *parent) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= N || rg_load(parent + v) < 0) return;
    rg_store(parent + v, rg_find(parent, (int)v));   // (whoever reads the old value meanwhile reads an ancestor)
}

// ---- the numbering ----------------------------------------------------------------------------------------------------------------
// tot[2 b], tot[2 b + 1]: the roots and the members of run b (the flattened map: a root is its own parent)
__global__ __launch_bounds__(TPB) void k_rg_count(long long N, const int *__restrict__ parent, unsigned long long *__restrict__ tot) {
    __shared__ unsigned int s_wave[2][TPB / XB_WAVE];
    const long long v = (long long)blockIdx.x * RG_BLOCK + threadIdx.x;
    const int p = v < N ? parent[v] : -1;
    const unsigned long long roots = __ballot(p >= 0 && p == (int)v), members = __ballot(p >= 0);
    if (threadIdx.x % XB_WAVE == 0) {
        s_wave[0][threadIdx.x / XB_WAVE] = (unsigned int)__popcll(roots);
        s_wave[1][threadIdx.x / XB_WAVE] = (unsigned int)__popcll(members);
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0;
        for (int k = 0; k < TPB / XB_WAVE; k++) s += s_wave[threadIdx.x][k];
        tot[2 * (long long)blockIdx.x + threadIdx.x] = s;
    }
}
// tot[2 b]: the roots before run b.  seed[i]: the i-th root in ascending order; num[root]: its number
__global__ __launch_bounds__(TPB) void k_rg_emit(long long N, const int *__restrict__ parent, const unsigned long long *__restrict__ tot,
                                                 int *__restrict__ seed, int *__restrict__ num) {
    __shared__ unsigned int s_wave[TPB / XB_WAVE];
    const long long v = (long long)blockIdx.x * RG_BLOCK + threadIdx.x;
    const bool root = v < N && parent[v] == (int)v;
    const unsigned long long roots = __ballot(root);
    const int lane = threadIdx.x % XB_WAVE, wave = threadIdx.x / XB_WAVE;
    if (lane == 0) s_wave[wave] = (unsigned int)__popcll(roots);
    __syncthreads();
    if (!root) return;
    unsigned long long at = tot[2 * (long long)blockIdx.x] + (unsigned long long)__popcll(roots & ((1ull << lane) - 1ull));
    for (int k = 0; k < wave; k++) at += s_wave[k];
    seed[at] = (int)v;
    num[v] = (int)at;
}
__global__ __launch_bounds__(TPB) void k_rg_number(long long N, int *__restrict__ map, const int *__restrict__ num) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= N) return;
    const int p = map[v];
    if (p >= 0) map[v] = num[p];
}

// ---- the sums per component -------------------------------------------------------------------------------------------------------
// all lanes call it (comp = -1 for nothing): dst[comp] = max(dst[comp], val); a wave that holds one component adds once
__device__ __forceinline__ void rg_wave_max(unsigned long long *dst, int comp, unsigned long long val) {
    const unsigned long long act = __ballot(comp >= 0);
    if (!act) return;
    const int first = __ffsll((long long)act) - 1, lc = __shfl(comp, first);
    if (__ballot(comp == lc) == act) {
        unsigned long long m = comp >= 0 ? val : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(m, o);
            m = other > m ? other : m;
        }
        if ((int)(threadIdx.x % XB_WAVE) == first && m > __atomic_load_n(dst + lc, __ATOMIC_RELAXED)) atomicMax(dst + lc, m);
    } else if (comp >= 0 && val > __atomic_load_n(dst + comp, __ATOMIC_RELAXED))   // (the cell only grows: a stale read asks once too often)
        atomicMax(dst + comp, val);
}
// one lane on its own (comp = -1 for nothing)
__device__ __forceinline__ void rg_wave_max_lane(unsigned long long *dst, int comp, unsigned long long val) {
    if (comp >= 0 && val > __atomic_load_n(dst + comp, __ATOMIC_RELAXED)) atomicMax(dst + comp, val);
}
// the cells of one class: key 3 component + k
struct RgSinkClass {
    double *sum, *mag;
    unsigned long long *cnt;
    int k;
    __device__ __forceinline__ void add(int a, double s, double m, unsigned int c) const {
        atomicAdd(&sum[3 * a + k], s); atomicAdd(&mag[3 * a + k], m); atomicAdd(&cnt[3 * a + k], (unsigned long long)c);
    }
};
// CLASSES: the key is 3 component + class (the class of nci_key, the 19 values from global memory), else the component; every
// class then has a carry of its own, so a wave inside one component whose voxels fall into several classes still adds once per
// class at its end and not once per run.
// A workgroup takes RG_STEPS runs of TPB consecutive voxels, so a wave walks RG_STEPS runs of 64 and carries its sums in registers
// while the component stays (k_moments.h's rule): inside a large component it adds once at its end, not once per run.
// sum (rho), sq (rho^2), cnt: one per key, zero on entry; topkey[component]: the greatest key(rho), zero on entry
template <bool CLASSES>
__global__ __launch_bounds__(TPB) void k_rg_sums(int nx, int ny, int nz, const double *__restrict__ rho, const int *__restrict__ map, StCoeffs K,
                                                 double rho_split, double *sum, double *sq, unsigned long long *cnt, unsigned long long *topkey) {
    const long long nyz = (long long)ny * nz, N = nx * nyz, first = (long long)blockIdx.x * (TPB * RG_STEPS) + threadIdx.x;
    StAcc A, A3[3];
    const StSinkGlb S{sum, sq, cnt};
    int held = -1;                   // the component this lane's running maximum belongs to
    unsigned long long best = 0ull;
    for (int i = 0; i < RG_STEPS; i++) {
        const long long v = first + (long long)i * TPB;
        if (v - threadIdx.x >= N) break;   // (uniform over the workgroup)
        int comp = -1, cls = -1;
        double s = 0., m = 0.;
        if (v < N) comp = map[v];
        if (comp >= 0) {
            s = rho[v];
            m = s * s;
            if (CLASSES) {
                const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
                const StGatherReader r(rho, x, y, z, nx, ny, nz);
                const NciVoxel w = nci_voxel(r, K);
                const double sx = (double)w.sig * w.rho;
                cls = sx < -rho_split ? 0 : (sx > rho_split ? 2 : 1);
            }
            const unsigned long long kr = aj_key(s);
            if (comp != held) {      // (this lane moves on to another component: what it held goes out)
                rg_wave_max_lane(topkey, held, best);
                held = comp;
                best = kr;
            } else if (kr > best)
                best = kr;
        }
        if (CLASSES) {
#pragma unroll
            for (int k = 0; k < 3; k++) st_step2(RgSinkClass{sum, sq, cnt, k}, A3[k], cls == k ? comp : -1, cls == k ? s : 0., cls == k ? m : 0.);
        } else
            st_step2(S, A, comp, s, m);
    }
    if (CLASSES) {
#pragma unroll
        for (int k = 0; k < 3; k++) st_finish(RgSinkClass{sum, sq, cnt, k}, A3[k]);
    } else
        st_finish(S, A);
    rg_wave_max(topkey, held, best);
}
// toplin[component]: the greatest index among the voxels whose key is topkey[component]; zero on entry
__global__ __launch_bounds__(TPB) void k_rg_top(long long N, const double *__restrict__ rho, const int *__restrict__ map,
                                                const unsigned long long *__restrict__ topkey, unsigned long long *toplin) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    int comp = v < N ? map[v] : -1;
    if (comp >= 0 && aj_key(rho[v]) != topkey[comp]) comp = -1;
    rg_wave_max(toplin, comp, (unsigned long long)v);
}

// ---- the shares: voxels per (component, label) ---------------------------------------------------------------------------------------
// tab[component * n + label], zero on entry (m n <= XB_DOMAINS_SHARE_CELLS: an int holds the cell).  A wave whose voxels of a run
// share one cell carries their number to the next run and adds when the cell changes; a mixed run adds per distinct cell.
// LDS: m n <= RG_SHARE_LDS and a workgroup counts in LDS, its non-empty cells going to the table at its end -- few labels would
// otherwise queue every wave of the grid up on a handful of addresses.
template <bool LDS>
__global__ __launch_bounds__(TPB) void k_rg_share_dense(long long N, const int *__restrict__ map, const int *__restrict__ labels, int n,
                                                        int cells, unsigned long long *tab) {
    __shared__ unsigned int s_cnt[LDS ? RG_SHARE_LDS : 1];   // (one counter nobody uses without LDS; a workgroup holds 4096 voxels)
    if (LDS) {
        for (int i = threadIdx.x; i < cells; i += TPB) s_cnt[i] = 0u;
        __syncthreads();
    }
    const long long first = (long long)blockIdx.x * (TPB * RG_STEPS) + threadIdx.x;
    const bool lead = threadIdx.x % XB_WAVE == 0;
    int cur = -1;                    // (uniform over the wave)
    unsigned long long held = 0ull;
    for (int i = 0; i < RG_STEPS; i++) {
        const long long v = first + (long long)i * TPB;
        if (v - threadIdx.x >= N) break;   // (uniform over the workgroup)
        int cell = -1;
        if (v < N) {
            const int comp = map[v], a = comp >= 0 ? labels[v] : -1;
            if (a >= 0 && a < n) cell = comp * n + a;
        }
        const unsigned long long act = __ballot(cell >= 0);
        if (!act) continue;
        const int lc = __shfl(cell, __ffsll((long long)act) - 1);
        if (__ballot(cell == lc) == act) {
            if (lc != cur) {
                if (lead && cur >= 0) {
                    if (LDS) atomicAdd(&s_cnt[cur], (unsigned int)held);
                    else atomicAdd(&tab[cur], held);
                }
                cur = lc;
                held = 0ull;
            }
            held += (unsigned long long)__popcll(act);
        } else if (LDS) {
            if (cell >= 0) atomicAdd(&s_cnt[cell], 1u);
        } else
            nci_count_wave(tab, cell);
    }
    if (lead && cur >= 0) {
        if (LDS) atomicAdd(&s_cnt[cur], (unsigned int)held);
        else atomicAdd(&tab[cur], held);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < cells; i += TPB)
            if (s_cnt[i]) atomicAdd(&tab[i], (unsigned long long)s_cnt[i]);
    }
}
// the non-empty cells of the table as pairs (cell, count), in the order the waves claimed their slots: out[2 i], out[2 i + 1]
__global__ __launch_bounds__(TPB) void k_rg_share_compact(long long cells, const unsigned long long *__restrict__ tab,
                                                          unsigned long long *__restrict__ out, unsigned long long cap, unsigned long long *used) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    const unsigned long long c = i < cells ? tab[i] : 0ull;
    const unsigned long long act = __ballot(c != 0ull);
    if (!act) return;
    const int lane = threadIdx.x % XB_WAVE, first = __ffsll((long long)act) - 1;
    unsigned long long base = 0ull;
    if (lane == first) base = atomicAdd(used, (unsigned long long)__popcll(act));
    base = __shfl(base, first);
    const unsigned long long at = base + (unsigned long long)__popcll(act & ((1ull << lane) - 1ull));
    if (c != 0ull && at < cap) { out[2 * at] = (unsigned long long)i; out[2 * at + 1] = c; }
}
// out[0 .. *used): the keys component * n + label of the labelled member voxels, in the order the waves claimed their slots
__global__ __launch_bounds__(TPB) void k_rg_share_list(long long N, const int *__restrict__ map, const int *__restrict__ labels, int n,
                                                       unsigned long long *__restrict__ out, unsigned long long cap, unsigned long long *used) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    bool have = false;
    unsigned long long key = 0ull;
    if (v < N) {
        const int comp = map[v], a = comp >= 0 ? labels[v] : -1;
        if (a >= 0 && a < n) { have = true; key = (unsigned long long)comp * (unsigned long long)n + (unsigned long long)a; }
    }
    const unsigned long long act = __ballot(have);
    if (!act) return;
    const int lane = threadIdx.x % XB_WAVE, first = __ffsll((long long)act) - 1;
    unsigned long long base = 0ull;
    if (lane == first) base = atomicAdd(used, (unsigned long long)__popcll(act));
    base = __shfl(base, first);
    const unsigned long long at = base + (unsigned long long)__popcll(act & ((1ull << lane) - 1ull));
    if (have && at < cap) out[at] = key;
}
