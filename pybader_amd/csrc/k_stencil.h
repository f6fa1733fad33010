// k_stencil.h -- device kernels of libbader_hip.so: the compact second-order stencil over the resident density -- the Laplacian as
// a field and summed per label, and rho, its gradient and its Hessian at listed voxels (xb_laplacian_field / xb_laplacian_sum /
// xb_stencil_points, host_stencil.h; the definition is in include/bader_hip.h and DESIGN.md section 18).  Included by
// bader_hip.hip (one translation unit) behind k_critical.h, whose tile and wrap it uses.
#pragma once

// Two routes for the field and for the sums.
//   tile     a workgroup stages the ST_TX x ST_TY x ST_TZ tile and its one-voxel halo of rho in LDS (10 x 10 x 34 doubles, 27 200 B:
//            six workgroups per compute unit), periodic wraps resolved at staging time as k_critical stages its keys; a thread owns
//            the column (ty, tz) and walks its ST_TX voxels, 19 LDS reads each.  8 B read and 8 B written per voxel for the field,
//            8 + 4 B read for the sums.
//   gather   (XB_STENCIL_GATHER) one thread per voxel reads its 19 values from global memory with the wraps computed per lane:
//            the second implementation, and the one for grids where tiles do not pay.
// Both form the same expressions in the same order (st_second, st_dot6): no contraction, so the values are the same bits.
//
// The sums follow k_moments.h: a wave whose voxels of a step carry ONE label adds into registers and reduces with shuffles when
// the label changes or the wave ends; a mixed step is peeled label by label, ST_GROUP lanes or more reduced with shuffles, fewer
// adding per lane.  What the lanes add to is
//   n <= ST_BINS  bins in LDS (sum, sum of magnitudes, count: 20 B per label), a block's non-empty bins to global memory at its end
//   any n         global memory
// ST_BINS = 256: 5 120 B.  The tile alone fills a compute unit's 160 KiB with six workgroups (6 * 27 200 = 163 200 of 163 840 B) and
// leaves 106 B for each, so no bin count keeps six; with the bins a workgroup takes 32 320 B and five fit (32 768 B each: up to
// 278 bins would), 20 waves per compute unit.  The gather route has no tile: its 5 120 B let eight workgroups -- every wave slot --
// share a compute unit.
#define ST_TX CP_TX
#define ST_TY CP_TY
#define ST_TZ CP_TZ
#define ST_BINS 256
#define ST_GROUP 8   // lanes of one label in a mixed step from which a shuffle reduction replaces per-lane adds
static_assert(ST_TY * ST_TZ == TPB, "one column of the tile per thread");
static_assert((ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2) * 8 + ST_BINS * 20 <= 160 * 1024 / 5, "five workgroups per compute unit");

// what xb_stencil_coeffs computes, passed by value (scalar loads)
struct StCoeffs {
    double t[9];    // gradient: t[3 * alpha + i]
    double w[6];    // Laplacian, terms 00 11 22 01 02 12
    double h[36];   // Hessian: h[6 * c + k], c in xx xy xz yy yz zz
};
static_assert(sizeof(StCoeffs) == XB_STENCIL_COEFFS * sizeof(double), "the layout of xb_stencil_coeffs");

// the six second differences of the definition, terms 00 11 22 01 02 12; r(dx, dy, dz) reads the wrapped neighbour, c = r(0, 0, 0)
template <class R>
__device__ __forceinline__ void st_second(const R &r, double c, double d[6]) {
    d[0] = (r(1, 0, 0) - c) + (r(-1, 0, 0) - c);
    d[1] = (r(0, 1, 0) - c) + (r(0, -1, 0) - c);
    d[2] = (r(0, 0, 1) - c) + (r(0, 0, -1) - c);
    d[3] = (r(1, 1, 0) - r(1, -1, 0)) - (r(-1, 1, 0) - r(-1, -1, 0));
    d[4] = (r(1, 0, 1) - r(1, 0, -1)) - (r(-1, 0, 1) - r(-1, 0, -1));
    d[5] = (r(0, 1, 1) - r(0, 1, -1)) - (r(0, -1, 1) - r(0, -1, -1));
}
// the left-associated sum of six products, every coefficient taking part
__device__ __forceinline__ double st_dot6(const double *k, const double d[6]) {
    return ((((k[0] * d[0] + k[1] * d[1]) + k[2] * d[2]) + k[3] * d[3]) + k[4] * d[4]) + k[5] * d[5];
}

typedef double StTile[ST_TY + 2][ST_TZ + 2];
struct StTileReader {
    const StTile *s;   // the staged tile, [ST_TX + 2] of them
    int hx, hy, hz;    // the voxel's place in it (halo included)
    __device__ __forceinline__ double operator()(int dx, int dy, int dz) const { return s[hx + dx][hy + dy][hz + dz]; }
};
struct StGatherReader {
    const double *rho;
    long long xo[3];   // the row offsets of x - 1, x, x + 1 (wrapped), and likewise
    int yo[3], zo[3];
    __device__ __forceinline__ StGatherReader(const double *rho_, int x, int y, int z, int nx, int ny, int nz) : rho(rho_) {
        const long long nyz = (long long)ny * nz;
        xo[0] = (x > 0 ? x - 1 : nx - 1) * nyz; xo[1] = x * nyz; xo[2] = (x + 1 < nx ? x + 1 : 0) * nyz;
        yo[0] = (y > 0 ? y - 1 : ny - 1) * nz; yo[1] = y * nz; yo[2] = (y + 1 < ny ? y + 1 : 0) * nz;
        zo[0] = z > 0 ? z - 1 : nz - 1; zo[1] = z; zo[2] = z + 1 < nz ? z + 1 : 0;
    }
    __device__ __forceinline__ double operator()(int dx, int dy, int dz) const { return rho[xo[dx + 1] + yo[dy + 1] + zo[dz + 1]]; }
};

// the tile of workgroup blockIdx.x and its halo, z fastest; every coordinate wraps (an axis shorter than the tile meets itself)
__device__ __forceinline__ void st_stage(StTile *s, int nx, int ny, int nz, const double *__restrict__ rho, int &x0, int &y0, int &z0) {
    const int tiles_z = (nz + ST_TZ - 1) / ST_TZ, tiles_y = (ny + ST_TY - 1) / ST_TY;
    const int bz = blockIdx.x % tiles_z, by = (blockIdx.x / tiles_z) % tiles_y, bx = blockIdx.x / (tiles_z * tiles_y);
    x0 = bx * ST_TX; y0 = by * ST_TY; z0 = bz * ST_TZ;
    for (int e = threadIdx.x; e < (ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2); e += TPB) {
        const int hz = e % (ST_TZ + 2), hy = (e / (ST_TZ + 2)) % (ST_TY + 2), hx = e / ((ST_TZ + 2) * (ST_TY + 2));
        const int x = cp_wrap(x0 - 1 + hx, nx), y = cp_wrap(y0 - 1 + hy, ny), z = cp_wrap(z0 - 1 + hz, nz);
        s[hx][hy][hz] = rho[((long long)x * ny + y) * nz + z];
    }
    __syncthreads();
}

// ---- the field ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_laplacian_field(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                         double *__restrict__ out) {
    __shared__ StTile s_rho[ST_TX + 2];
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    if (y >= ny || z >= nz) return;
#pragma unroll
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        if (x >= nx) break;
        const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
        double d[6];
        st_second(r, r(0, 0, 0), d);
        out[((long long)x * ny + y) * nz + z] = st_dot6(K.w, d);
    }
}

__global__ __launch_bounds__(TPB) void k_laplacian_field_gather(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                                double *__restrict__ out) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    if (v >= nx * nyz) return;
    const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
    const StGatherReader r(rho, x, y, z, nx, ny, nz);
    double d[6];
    st_second(r, r(0, 0, 0), d);
    out[v] = st_dot6(K.w, d);
}

// ---- the sums per label -----------------------------------------------------------------------------------------------------------
struct StSinkLds {
    double *sum, *mag;    // [n] each
    unsigned int *cnt;    // [n]
    __device__ __forceinline__ void add(int a, double s, double m, unsigned int c) const {
        atomicAdd(&sum[a], s); atomicAdd(&mag[a], m); atomicAdd(&cnt[a], c);
    }
};
struct StSinkGlb {
    double *sum, *mag;
    unsigned long long *cnt;
    __device__ __forceinline__ void add(int a, double s, double m, unsigned int c) const {
        atomicAdd(&sum[a], s); atomicAdd(&mag[a], m); atomicAdd(&cnt[a], (unsigned long long)c);
    }
};
// what a wave carries from step to step while its voxels share one label (cur, n: uniform; s, m: per lane)
struct StAcc {
    double s = 0., m = 0.;
    unsigned int n = 0;
    int cur = -1;
};

// all lanes call it; s and m of the lanes outside the group must be zero; lane `leader` adds the wave's sums for label a
template <class Sink>
__device__ __forceinline__ void st_wave_add(const Sink &S, int a, double s, double m, unsigned int c, int leader) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o); m += __shfl_xor(m, o); }
    if ((int)(threadIdx.x % XB_WAVE) == leader) S.add(a, s, m, c);
}
// one step of a wave (all lanes call it): this lane's voxel has the key a >= 0, or a = -1 for nothing, and adds s to the first sum
// of its key and m to the second; both must be zero where a = -1
template <class Sink>
__device__ __forceinline__ void st_step2(const Sink &S, StAcc &A, int a, double s, double m) {
    const unsigned long long act = __ballot(a >= 0);
    if (!act) return;
    const int la = __shfl(a, __ffsll((long long)act) - 1);
    if (__ballot(a == la) == act) {   // one label in this step
        if (la != A.cur && A.cur >= 0) {
            st_wave_add(S, A.cur, A.s, A.m, A.n, 0);
            A.s = 0.; A.m = 0.; A.n = 0;
        }
        A.cur = la;
        A.s += s; A.m += m;
        A.n += (unsigned int)__popcll(act);
        return;
    }
    // several labels: peel them off one by one
    unsigned long long todo = act;
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lb = __shfl(a, leader);
        const bool mine = a == lb;
        const unsigned long long grp = __ballot(mine);
        const unsigned int c = (unsigned int)__popcll(grp);
        if (c >= ST_GROUP) st_wave_add(S, lb, mine ? s : 0., mine ? m : 0., c, leader);
        else if (mine) S.add(a, s, m, 1u);
        todo &= ~grp;
    }
}
// the Laplacian's step: label a in [0, n) or -1, the sums of v and of its magnitude
template <class Sink>
__device__ __forceinline__ void st_step(const Sink &S, StAcc &A, int a, double v) {
    st_step2(S, A, a, a >= 0 ? v : 0., a >= 0 ? fabs(v) : 0.);
}
template <class Sink>
__device__ __forceinline__ void st_finish(const Sink &S, StAcc &A) {
    if (A.cur >= 0) st_wave_add(S, A.cur, A.s, A.m, A.n, 0);
}

template <int B>
struct StBins {
    double sum[B], mag[B];
    unsigned int cnt[B];
    __device__ __forceinline__ StSinkLds sink() { return StSinkLds{sum, mag, cnt}; }
};
template <int B>
__device__ __forceinline__ void st_bins_clear(StBins<B> &b, int n) {
    for (int i = threadIdx.x; i < n; i += TPB) { b.sum[i] = 0.; b.mag[i] = 0.; b.cnt[i] = 0u; }
}
// the block's non-empty bins to the result (between two __syncthreads of the caller's)
template <int B>
__device__ __forceinline__ void st_bins_flush(const StBins<B> &b, int n, double *sum, double *mag, unsigned long long *cnt) {
    for (int i = threadIdx.x; i < n; i += TPB)
        if (b.cnt[i]) {
            atomicAdd(&sum[i], b.sum[i]); atomicAdd(&mag[i], b.mag[i]); atomicAdd(&cnt[i], (unsigned long long)b.cnt[i]);
        }
}

// BINS: n <= ST_BINS and the adds go to LDS.  sum, mag, cnt: [n] each, zero on entry
template <bool BINS>
__global__ __launch_bounds__(TPB) void k_laplacian_sum(int nx, int ny, int nz, const double *__restrict__ rho, const int *__restrict__ labels,
                                                       int n, StCoeffs K, double *sum, double *mag, unsigned long long *cnt) {
    __shared__ StTile s_rho[ST_TX + 2];
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;   // (one bin nobody uses without BINS)
    if (BINS) st_bins_clear(s_bins, n);   // (st_stage's barrier covers it)
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool inside = y < ny && z < nz;
    StAcc A;
#pragma unroll
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        int a = -1;
        double v = 0.;
        if (inside && x < nx) {
            a = labels[((long long)x * ny + y) * nz + z];
            if (a >= 0 && a < n) {
                const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
                double d[6];
                st_second(r, r(0, 0, 0), d);
                v = st_dot6(K.w, d);
            } else
                a = -1;
        }
        if (BINS) st_step(s_bins.sink(), A, a, v);
        else st_step(StSinkGlb{sum, mag, cnt}, A, a, v);
    }
    if (BINS) {
        st_finish(s_bins.sink(), A);
        __syncthreads();
        st_bins_flush(s_bins, n, sum, mag, cnt);
    } else
        st_finish(StSinkGlb{sum, mag, cnt}, A);
}

template <bool BINS>
__global__ __launch_bounds__(TPB) void k_laplacian_sum_gather(int nx, int ny, int nz, const double *__restrict__ rho,
                                                              const int *__restrict__ labels, int n, StCoeffs K, double *sum, double *mag,
                                                              unsigned long long *cnt) {
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;   // (one bin nobody uses without BINS)
    if (BINS) {
        st_bins_clear(s_bins, n);
        __syncthreads();
    }
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    int a = -1;
    double lap = 0.;
    if (v < nx * nyz) {
        a = labels[v];
        if (a >= 0 && a < n) {
            const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
            const StGatherReader r(rho, x, y, z, nx, ny, nz);
            double d[6];
            st_second(r, r(0, 0, 0), d);
            lap = st_dot6(K.w, d);
        } else
            a = -1;
    }
    StAcc A;
    if (BINS) {
        const StSinkLds S = s_bins.sink();
        st_step(S, A, a, lap);
        st_finish(S, A);
        __syncthreads();
        st_bins_flush(s_bins, n, sum, mag, cnt);
    } else {
        const StSinkGlb S{sum, mag, cnt};
        st_step(S, A, a, lap);
        st_finish(S, A);
    }
}

// ---- listed voxels ----------------------------------------------------------------------------------------------------------------
// One thread per listed voxel (lin checked by the host): rho, the three gradient components, the six Hessian components.
__global__ __launch_bounds__(TPB) void k_stencil_points(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                        const long long *__restrict__ lin, long long m, double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= m) return;
    const long long v = lin[i], nyz = (long long)ny * nz;
    const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
    const StGatherReader r(rho, x, y, z, nx, ny, nz);
    const double c = r(0, 0, 0);
    double d[6];
    st_second(r, c, d);
    const double g0 = r(1, 0, 0) - r(-1, 0, 0), g1 = r(0, 1, 0) - r(0, -1, 0), g2 = r(0, 0, 1) - r(0, 0, -1);
    double *o = out + i * XB_STENCIL_POINT_VALUES;
    o[0] = c;
#pragma unroll
    for (int al = 0; al < 3; al++) o[1 + al] = ((K.t[3 * al] * g0) + K.t[3 * al + 1] * g1) + K.t[3 * al + 2] * g2;
#pragma unroll
    for (int k = 0; k < 6; k++) o[4 + k] = st_dot6(K.h + 6 * k, d);
}
