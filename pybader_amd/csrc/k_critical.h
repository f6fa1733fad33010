// k_critical.h -- device kernels of libbader_hip.so: the piecewise-linear critical points of the density on the Freudenthal
// triangulation of the periodic voxel lattice, and the basins the bond points join (xb_critical_points / xb_critical_bonds,
// host_critical.h; the definition is in include/bader_hip.h and DESIGN.md section 17).  Included by bader_hip.hip (one
// translation unit).
#pragma once
#include <utility>

// One streaming pass over the density (8 B per voxel).  A workgroup stages the keys of a CP_TX x CP_TY x CP_TZ tile and its
// one-voxel halo in LDS (27 200 B: six workgroups per compute unit); a thread owns the column (ty, tz) of the tile and walks
// its CP_TX voxels: 14 ordered comparisons give the lower mask L, one byte of the 16 384-entry table (global memory: 16 KB that
// stay in every L1 / L2 next to the streamed lines, and cost no LDS, so the occupancy is the tile's) or, with
// XB_CRITICAL_FLOOD, a flood fill in registers gives ring | bond << 4.  Non-regular voxels are rare on smooth data: a wave
// without one leaves after one ballot; the others claim slots in LDS, the workgroup claims its share of the list with ONE global
// atomic and adds its six counts.  Every number is an integer: atomics in any order give the same result, and the host sorts
// the records (lin in the high word) as it sorts the pairs of xb_adjacency.
#define CP_TX 8
#define CP_TY 8
#define CP_TZ 32
#define CP_FULL 0x3fffu
#define CP_NONE (-2147483647 - 1)   // "no component" among the six labels of a bond row
#define CP_BOND_ROW 5               // words of a bond row: key(rho[v]), lin(v), six int32 labels
static_assert(CP_TY * CP_TZ == TPB, "one column of the tile per thread");
static_assert(CP_FULL == XB_CRITICAL_FULL && (1 << 14) == XB_CRITICAL_LUT_SIZE, "14 neighbours");

// component j (0 x, 1 y, 2 z) of offset k: d_k = the bits of k + 1 for k < 7, d_{7 + k} = -d_k
constexpr __host__ __device__ int cp_d(int k, int j) {
    return k < 7 ? (((k + 1) >> (2 - j)) & 1) : -((((k - 7) + 1) >> (2 - j)) & 1);
}
// bits a and b of a mask are adjacent iff d_b - d_a (no wrapping) is one of the 14 offsets: not zero, and all of its components
// in {0, 1} or all in {0, -1}
constexpr __host__ __device__ bool cp_adjacent(int a, int b) {
    int lo = 0, hi = 0;
    for (int j = 0; j < 3; j++) {
        const int e = cp_d(b, j) - cp_d(a, j);
        lo = e < lo ? e : lo;
        hi = e > hi ? e : hi;
    }
    return (lo != 0 || hi != 0) && lo >= -1 && hi <= 1 && !(lo < 0 && hi > 0);
}
constexpr __host__ __device__ unsigned cp_adj_mask(int a) {
    unsigned m = 0;
    for (int b = 0; b < 14; b++)
        if (cp_adjacent(a, b)) m |= 1u << b;
    return m;
}
template <int K> struct CpAdj { static constexpr unsigned value = cp_adj_mask(K); };
namespace cp_check {
constexpr int edges2() {
    int n = 0;
    for (int a = 0; a < 14; a++)
        for (int b = 0; b < 14; b++) n += cp_adjacent(a, b) ? 1 : 0;
    return n;
}
constexpr int triangles6() {
    int n = 0;
    for (int a = 0; a < 14; a++)
        for (int b = 0; b < 14; b++)
            for (int c = 0; c < 14; c++) n += (cp_adjacent(a, b) && cp_adjacent(b, c) && cp_adjacent(a, c)) ? 1 : 0;
    return n;
}
static_assert(edges2() == 2 * 36 && triangles6() == 6 * 24, "the link is a triangulated sphere: 14 - 36 + 24 = 2");
static_assert(cp_d(0, 2) == 1 && cp_d(2, 1) == 1 && cp_d(2, 2) == 1 && cp_d(3, 0) == 1 && cp_d(6, 0) + cp_d(6, 1) + cp_d(6, 2) == 3 &&
              cp_d(9, 1) == -1 && cp_d(9, 2) == -1 && cp_d(9, 0) == 0, "the offsets of the definition");
}

// the set bits of s and their neighbours in the link graph
template <int... K>
__host__ __device__ __forceinline__ unsigned cp_expand_seq(unsigned s, std::integer_sequence<int, K...>) {
    return (s | ... | ((0u - ((s >> K) & 1u)) & CpAdj<K>::value));
}
__host__ __device__ __forceinline__ unsigned cp_expand(unsigned s) { return cp_expand_seq(s, std::make_integer_sequence<int, 14>()); }
// the component of the lowest set bit of rem inside the mask m (rem a union of components of m)
__host__ __device__ __forceinline__ unsigned cp_component(unsigned rem, unsigned m) {
    unsigned s = rem & (0u - rem);
    for (;;) {
        const unsigned t = cp_expand(s) & m;
        if (t == s) return s;
        s = t;
    }
}
__host__ __device__ __forceinline__ int cp_components(unsigned m) {
    int n = 0;
    while (m) { m &= ~cp_component(m, m); n++; }
    return n;
}
// ring | bond << 4 of the lower mask L; 0 for a regular voxel and for the two extrema (which the mask itself tells)
__host__ __device__ __forceinline__ unsigned cp_classify(unsigned L) {
    if (L == 0u || L == CP_FULL) return 0u;
    return (unsigned)(cp_components(L) - 1) | ((unsigned)(cp_components(~L & CP_FULL) - 1) << 4);
}

__device__ __forceinline__ double cp_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ (1ull << 63)) : ~k));
}
// v in [-1, 2 n + ...): into [0, n); the division only on an axis shorter than the tile
__device__ __forceinline__ int cp_wrap(int v, int n) {
    if (v < 0) v += n;
    if (v >= n) { v -= n; if (v >= n) v %= n; }
    return v;
}
// sign of (coordinate of the wrapped neighbour) - (own coordinate) for a step of +1 / -1 on an axis of n voxels
__device__ __forceinline__ int cp_sign_p(int p, int n) { return p + 1 < n ? 1 : (n == 1 ? 0 : -1); }
__device__ __forceinline__ int cp_sign_m(int p, int n) { return p > 0 ? -1 : (n == 1 ? 0 : 1); }
// bit k: lin(u_k) < lin(v), u_k the wrapped neighbour -- C order is the lexicographic order of the coordinates
__device__ __forceinline__ unsigned cp_tie_mask(int x, int y, int z, int nx, int ny, int nz) {
    const int xp = 9 * cp_sign_p(x, nx), xm = 9 * cp_sign_m(x, nx), yp = 3 * cp_sign_p(y, ny), ym = 3 * cp_sign_m(y, ny);
    const int zp = cp_sign_p(z, nz), zm = cp_sign_m(z, nz);
    unsigned t = 0;
#pragma unroll
    for (int k = 0; k < 14; k++) {
        const int dx = cp_d(k, 0), dy = cp_d(k, 1), dz = cp_d(k, 2);
        const int s = (dx > 0 ? xp : (dx < 0 ? xm : 0)) + (dy > 0 ? yp : (dy < 0 ? ym : 0)) + (dz > 0 ? zp : (dz < 0 ? zm : 0));
        t |= (s < 0 ? 1u : 0u) << k;
    }
    return t;
}

// cnt[0..5]: the six counts; cnt[6]: records wanted (it may exceed `cap`: the host grows the list and runs the pass again).
// A record is lin << 32 | L << 8 | ring | bond << 4.
__global__ __launch_bounds__(TPB) void k_critical(int nx, int ny, int nz, const double *__restrict__ rho,
                                                 const unsigned char *__restrict__ lut /* null: flood fill */, int use_vac, double vac_tol,
                                                 unsigned long long *__restrict__ list, unsigned long long cap, unsigned long long *cnt) {
    __shared__ unsigned long long s_key[CP_TX + 2][CP_TY + 2][CP_TZ + 2];
    __shared__ unsigned int s_cnt[8];
    __shared__ unsigned long long s_base;
    const int tiles_z = (nz + CP_TZ - 1) / CP_TZ, tiles_y = (ny + CP_TY - 1) / CP_TY;
    const int bz = blockIdx.x % tiles_z, by = (blockIdx.x / tiles_z) % tiles_y, bx = blockIdx.x / (tiles_z * tiles_y);
    const int x0 = bx * CP_TX, y0 = by * CP_TY, z0 = bz * CP_TZ;
    const int tid = threadIdx.x;
    if (tid < 8) s_cnt[tid] = 0u;
    // the tile and its one-voxel halo, z fastest; every coordinate wraps (an axis shorter than the tile meets itself)
    for (int e = tid; e < (CP_TX + 2) * (CP_TY + 2) * (CP_TZ + 2); e += TPB) {
        const int hz = e % (CP_TZ + 2), hy = (e / (CP_TZ + 2)) % (CP_TY + 2), hx = e / ((CP_TZ + 2) * (CP_TY + 2));
        const int x = cp_wrap(x0 - 1 + hx, nx), y = cp_wrap(y0 - 1 + hy, ny), z = cp_wrap(z0 - 1 + hz, nz);
        s_key[hx][hy][hz] = aj_key(rho[((long long)x * ny + y) * nz + z]);
    }
    __syncthreads();
    const int tz = tid % CP_TZ, ty = tid / CP_TZ;
    const int y = y0 + ty, z = z0 + tz;
    unsigned int info[CP_TX];
    unsigned int mine = 0, c_max = 0, c_bv = 0, c_bs = 0, c_rv = 0, c_rs = 0, c_min = 0;
#pragma unroll
    for (int tx = 0; tx < CP_TX; tx++) {
        info[tx] = 0u;
        const int x = x0 + tx;
        if (x < nx && y < ny && z < nz) {
            const unsigned long long kv = s_key[tx + 1][ty + 1][tz + 1];
            unsigned int lt = 0, eq = 0;
#pragma unroll
            for (int k = 0; k < 14; k++) {
                const unsigned long long ku = s_key[tx + 1 + cp_d(k, 0)][ty + 1 + cp_d(k, 1)][tz + 1 + cp_d(k, 2)];
                lt |= (ku < kv ? 1u : 0u) << k;
                eq |= (ku == kv ? 1u : 0u) << k;
            }
            unsigned int L = lt;
            if (eq) L |= eq & cp_tie_mask(x, y, z, nx, ny, nz);
            const unsigned int code = lut ? (unsigned int)lut[L] : cp_classify(L);
            bool crit = L == 0u || L == CP_FULL || code != 0u;
            if (use_vac && cp_unkey(kv) <= vac_tol) crit = false;
            if (crit) {
                info[tx] = 0x80000000u | (L << 8) | code;
                mine++;
                c_max += L == CP_FULL ? 1u : 0u;
                c_min += L == 0u ? 1u : 0u;
                c_rv += (code & 15u) ? 1u : 0u;
                c_rs += code & 15u;
                c_bv += (code >> 4) ? 1u : 0u;
                c_bs += code >> 4;
            }
        }
    }
    unsigned int slot = 0;
    if (__ballot(mine != 0u)) {   // (else: a wave of regular voxels -- nothing to count, nothing to list)
        if (mine) {
            slot = atomicAdd(&s_cnt[6], mine);
            if (c_max) atomicAdd(&s_cnt[XB_CRITICAL_MAXIMA], c_max);
            if (c_bv) atomicAdd(&s_cnt[XB_CRITICAL_BOND_VOXELS], c_bv);
            if (c_bs) atomicAdd(&s_cnt[XB_CRITICAL_BOND_SUM], c_bs);
            if (c_rv) atomicAdd(&s_cnt[XB_CRITICAL_RING_VOXELS], c_rv);
            if (c_rs) atomicAdd(&s_cnt[XB_CRITICAL_RING_SUM], c_rs);
            if (c_min) atomicAdd(&s_cnt[XB_CRITICAL_MINIMA], c_min);
        }
    }
    __syncthreads();
    if (tid < 7 && s_cnt[tid]) {
        const unsigned long long old = atomicAdd(&cnt[tid], (unsigned long long)s_cnt[tid]);
        if (tid == 6) s_base = old;
    }
    __syncthreads();
    if (mine) {
        unsigned long long at = s_base + slot;
#pragma unroll
        for (int tx = 0; tx < CP_TX; tx++) {
            if (!info[tx]) continue;
            const unsigned long long lin = ((unsigned long long)(x0 + tx) * ny + y) * nz + z;
            if (at < cap) list[at] = (lin << 32) | (unsigned long long)(info[tx] & 0x7fffffffu);
            at++;
        }
    }
}

// One thread per listed voxel; the bond voxels (bond > 0) claim a row of `out` each: key(rho[v]), lin(v) and, per component of the
// upper mask, the label of its top -- the greatest neighbour of the component in the order of the definition.  Rows in any order:
// the host's reduction per pair is a count, a maximum and a minimum.
__global__ __launch_bounds__(TPB) void k_critical_bonds(int nx, int ny, int nz, const double *__restrict__ rho, const int *__restrict__ labels,
                                                       const unsigned long long *__restrict__ list, unsigned long long n_list,
                                                       unsigned long long *__restrict__ out, unsigned long long cap, unsigned long long *count) {
    const unsigned long long i = (unsigned long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n_list) return;
    const unsigned long long rec = list[i];
    if (((rec >> 4) & 15ull) == 0ull) return;
    const unsigned long long row = atomicAdd(count, 1ull);
    if (row >= cap) return;
    const unsigned int U = ~(unsigned int)(rec >> 8) & CP_FULL;
    const long long lin = (long long)(rec >> 32);
    const int x = (int)(lin / ((long long)ny * nz)), r = (int)(lin - (long long)x * ny * nz), y = r / nz, z = r - y * nz;
    unsigned long long *o = out + row * CP_BOND_ROW;
    int *lab = reinterpret_cast<int *>(o + 2);
    o[0] = aj_key(rho[lin]);
    o[1] = (unsigned long long)lin;
    for (int k = 0; k < 6; k++) lab[k] = CP_NONE;
    unsigned int rem = U;
    for (int n = 0; rem && n < 6; n++) {
        const unsigned int comp = cp_component(rem, U);
        rem &= ~comp;
        unsigned long long best_k = 0ull;
        long long best_l = -1;
#pragma unroll
        for (int k = 0; k < 14; k++) {
            if (!((comp >> k) & 1u)) continue;
            const int ux = cp_wrap(x + cp_d(k, 0), nx), uy = cp_wrap(y + cp_d(k, 1), ny), uz = cp_wrap(z + cp_d(k, 2), nz);
            const long long lu = ((long long)ux * ny + uy) * nz + uz;
            const unsigned long long ku = aj_key(rho[lu]);
            if (best_l < 0 || ku > best_k || (ku == best_k && lu > best_l)) { best_k = ku; best_l = lu; }
        }
        lab[n] = labels[best_l];
    }
}
