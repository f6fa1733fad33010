// k_nci.h -- device kernels of libbader_hip.so: the NCI index over the resident density -- the reduced density gradient s and
// sign(lambda2) rho as fields, the region's sums per label and class, and the s against sign(lambda2) rho histogram (xb_nci_field /
// xb_nci_sum / xb_nci_hist, host_nci.h; the definition is in include/bader_hip.h and DESIGN.md section 20).  Included by
// bader_hip.hip (one translation unit) behind k_stencil.h, whose tile, readers, staging and wave sums it uses.
#pragma once

// One function, nci_voxel, forms (rho, g2, sigma, q, r8) of a voxel from a reader; the tile route hands it an StTileReader, the
// gather route (XB_STENCIL_GATHER) an StGatherReader, so both run the same expressions in the same order: the same bits.
// Everything that DECIDES something -- the region, the class, the bin -- is multiplications and comparisons of those five; the
// square root and the cube root enter the field s alone.
//
// LDS per workgroup and workgroups per compute unit (160 KiB = 163 840 B, the arithmetic of k_stencil.h's header):
//   k_nci_field          the tile, 10 x 10 x 34 doubles = 27 200 B: six (163 200 B)
//   k_nci_sum<true>      the tile + StBins<ST_BINS> (256 keys x 20 B = 5 120 B) = 32 320 B: five, as k_laplacian_sum<true>;
//                        3 n <= ST_BINS keys, n <= NCI_LABELS_LDS = 85
//   k_nci_sum<false>     the tile (the unused bin is dropped by the compiler): six
//   k_nci_hist<true>     the tile + NCI_HIST_LDS = 1024 counters x 4 B = 4 096 B = 31 296 B: five (32 768 B each would hold
//                        1 392 counters; 1024 keeps the power of two)
//   k_nci_hist<false>    the tile (the unused counter is dropped by the compiler): six; a wave adds once per distinct bin
//   the gather kernels   no tile: 5 120 B (sums) and 4 096 B (histogram), eight workgroups -- every wave slot -- per compute unit
// The edge tables of the histogram (n_s + 1 thresholds, n_x + 1 edges) stay in global memory: a binary search reads at most
// log2(n) + 1 entries of each, the first steps of every lane's search read the same entries (one line for the wave), and the
// whole table of a typical call (some hundred doubles) sits in the compute unit's 32 KiB vector L1 after the first wave.  In LDS
// the tables would take up to 16 KiB of a workgroup whose tile already leaves 5 568 B of its fifth of the compute unit.
#define NCI_HIST_LDS XB_NCI_HIST_LDS_BINS
#define NCI_LABELS_LDS (ST_BINS / 3)
static_assert((ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2) * 8 + NCI_HIST_LDS * 4 <= 160 * 1024 / 5, "five workgroups per compute unit");
static_assert(NCI_LABELS_LDS == 85, "the label count up to which the sums use LDS bins, as include/bader_hip.h states it");

struct NciVoxel {
    double rho, g2, q, r8;   // the density, |grad rho|^2, (g2 g2) g2, ((rho rho)^2)^2
    double r2;               // rho rho
    int sig;                 // the sign of the Hessian's middle eigenvalue: -1, 0, +1
};

// Descartes' rule on (1, -I1, I2, -I3): p sign changes (zeros skipped), z trailing zeros, 3 - p - z negative roots.  A NaN counts
// as a zero: it is neither below nor above 0.
__host__ __device__ __forceinline__ int nci_sign(double I1, double I2, double I3) {
    const int s1 = (I1 < 0.) - (I1 > 0.), s2 = (I2 > 0.) - (I2 < 0.), s3 = (I3 < 0.) - (I3 > 0.);
    int p = 0, last = 1;
    if (s1) { p += s1 != last; last = s1; }
    if (s2) { p += s2 != last; last = s2; }
    if (s3) { p += s3 != last; }
    const int z = s3 ? 0 : (s2 ? 1 : (s1 ? 2 : 3));
    return p >= 2 ? 1 : (3 - p - z >= 2 ? -1 : 0);
}

template <class R>
__device__ __forceinline__ NciVoxel nci_voxel(const R &r, const StCoeffs &K) {
    const double c = r(0, 0, 0);
    double d[6], g[3], H[6];
    st_second(r, c, d);
    const double g0 = r(1, 0, 0) - r(-1, 0, 0), g1 = r(0, 1, 0) - r(0, -1, 0), g2 = r(0, 0, 1) - r(0, 0, -1);
#pragma unroll
    for (int al = 0; al < 3; al++) g[al] = ((K.t[3 * al] * g0) + K.t[3 * al + 1] * g1) + K.t[3 * al + 2] * g2;
#pragma unroll
    for (int k = 0; k < 6; k++) H[k] = st_dot6(K.h + 6 * k, d);
    const double xx = H[0], xy = H[1], xz = H[2], yy = H[3], yz = H[4], zz = H[5];
    const double I1 = (xx + yy) + zz;
    const double I2 = ((xx * yy - xy * xy) + (xx * zz - xz * xz)) + (yy * zz - yz * yz);
    const double I3 = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz);
    NciVoxel v;
    v.rho = c;
    v.g2 = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    v.sig = nci_sign(I1, I2, I3);
    v.r2 = c * c;
    const double r4 = v.r2 * v.r2;
    v.r8 = r4 * r4;
    v.q = (v.g2 * v.g2) * v.g2;
    return v;
}

// ---- the fields -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void nci_store(const NciVoxel &v, double *__restrict__ s, double *__restrict__ x, long long at) {
    if (v.rho > 0.) {
        s[at] = sqrt(v.g2) / (XB_NCI_C * (v.rho * cbrt(v.rho)));
        x[at] = (double)v.sig * v.rho;
    } else {
        s[at] = __builtin_huge_val();
        x[at] = 0.;
    }
}

__global__ __launch_bounds__(TPB) void k_nci_field(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                   double *__restrict__ s_out, double *__restrict__ x_out) {
    __shared__ StTile s_rho[ST_TX + 2];
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    if (y >= ny || z >= nz) return;
#pragma unroll 2
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        if (x >= nx) break;
        const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
        nci_store(nci_voxel(r, K), s_out, x_out, ((long long)x * ny + y) * nz + z);
    }
}

__global__ __launch_bounds__(TPB) void k_nci_field_gather(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                          double *__restrict__ s_out, double *__restrict__ x_out) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    if (v >= nx * nyz) return;
    const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
    const StGatherReader r(rho, x, y, z, nx, ny, nz);
    nci_store(nci_voxel(r, K), s_out, x_out, v);
}

// ---- the region's sums per label and class ------------------------------------------------------------------------------------
// what the host forms once: T(s_cut) and the two density thresholds
struct NciCuts {
    double t_cut, rho_cut, rho_split;
};
// the key 3 a + class of a voxel with label a in [0, n) inside the region, else -1
__device__ __forceinline__ int nci_key(const NciVoxel &v, int a, const NciCuts &C) {
    if (!(v.rho > 0.) || !(v.q < C.t_cut * v.r8) || !(v.rho < C.rho_cut)) return -1;
    const double x = (double)v.sig * v.rho;
    return 3 * a + (x < -C.rho_split ? 0 : (x > C.rho_split ? 2 : 1));
}

// BINS: 3 n <= ST_BINS and the adds go to LDS.  sum (rho), sq (rho^2), cnt: [3 n] each, zero on entry
template <bool BINS>
__global__ __launch_bounds__(TPB) void k_nci_sum(int nx, int ny, int nz, const double *__restrict__ rho, const int *__restrict__ labels,
                                                 int n, StCoeffs K, NciCuts C, double *sum, double *sq, unsigned long long *cnt) {
    __shared__ StTile s_rho[ST_TX + 2];
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;   // (one bin nobody uses without BINS)
    if (BINS) st_bins_clear(s_bins, 3 * n);   // (st_stage's barrier covers it)
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool inside = y < ny && z < nz;
    StAcc A;
#pragma unroll 2
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        int key = -1;
        double s = 0., m = 0.;
        if (inside && x < nx) {
            const int a = labels[((long long)x * ny + y) * nz + z];
            if (a >= 0 && a < n) {
                const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
                const NciVoxel v = nci_voxel(r, K);
                key = nci_key(v, a, C);
                if (key >= 0) { s = v.rho; m = v.r2; }
            }
        }
        if (BINS) st_step2(s_bins.sink(), A, key, s, m);
        else st_step2(StSinkGlb{sum, sq, cnt}, A, key, s, m);
    }
    if (BINS) {
        st_finish(s_bins.sink(), A);
        __syncthreads();
        st_bins_flush(s_bins, 3 * n, sum, sq, cnt);
    } else
        st_finish(StSinkGlb{sum, sq, cnt}, A);
}

template <bool BINS>
__global__ __launch_bounds__(TPB) void k_nci_sum_gather(int nx, int ny, int nz, const double *__restrict__ rho,
                                                        const int *__restrict__ labels, int n, StCoeffs K, NciCuts C, double *sum,
                                                        double *sq, unsigned long long *cnt) {
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;   // (one bin nobody uses without BINS)
    if (BINS) {
        st_bins_clear(s_bins, 3 * n);
        __syncthreads();
    }
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    int key = -1;
    double s = 0., m = 0.;
    if (v < nx * nyz) {
        const int a = labels[v];
        if (a >= 0 && a < n) {
            const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
            const StGatherReader r(rho, x, y, z, nx, ny, nz);
            const NciVoxel w = nci_voxel(r, K);
            key = nci_key(w, a, C);
            if (key >= 0) { s = w.rho; m = w.r2; }
        }
    }
    StAcc A;
    if (BINS) {
        const StSinkLds S = s_bins.sink();
        st_step2(S, A, key, s, m);
        st_finish(S, A);
        __syncthreads();
        st_bins_flush(s_bins, 3 * n, sum, sq, cnt);
    } else {
        const StSinkGlb S{sum, sq, cnt};
        st_step2(S, A, key, s, m);
        st_finish(S, A);
    }
}

// ---- the histogram ----------------------------------------------------------------------------------------------------------------
// (the number of j in [0, m) with e[j] * scale <= v) - 1, by binary search: the products are monotone in e
__device__ __forceinline__ int nci_bin(const double *__restrict__ e, int m, double scale, double v) {
    int lo = 0, hi = m;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] * scale <= v) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}
// the bin n_x ks + kx of a voxel, or -1; ts: the n_s + 1 thresholds T(e_j), xe: the n_x + 1 edges of x
__device__ __forceinline__ int nci_cell(const NciVoxel &v, const double *__restrict__ ts, int n_s, const double *__restrict__ xe, int n_x) {
    if (!(v.rho > 0.)) return -1;
    const int ks = nci_bin(ts, n_s + 1, v.r8, v.q);
    if (ks < 0 || ks >= n_s) return -1;
    const int kx = nci_bin(xe, n_x + 1, 1., (double)v.sig * v.rho);
    if (kx < 0 || kx >= n_x) return -1;
    return ks * n_x + kx;
}

// one step of a wave towards global memory (all lanes call it; cell = -1 for nothing): the lanes that share a bin are peeled off
// together and their first lane adds their number -- neighbouring voxels mostly share bins, and 64 single adds to one address
// would queue up behind each other in the L2
__device__ __forceinline__ void nci_count_wave(unsigned long long *counts, int cell) {
    unsigned long long todo = __ballot(cell >= 0);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __shfl(cell, leader);
        const unsigned long long grp = __ballot(cell == lc);
        if ((int)(threadIdx.x % XB_WAVE) == leader) atomicAdd(&counts[lc], (unsigned long long)__popcll(grp));
        todo &= ~grp;
    }
}

// LDS: n_s n_x <= NCI_HIST_LDS and a block counts in LDS.  counts: [n_s n_x], zero on entry
template <bool LDS>
__global__ __launch_bounds__(TPB) void k_nci_hist(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                  const double *__restrict__ ts, int n_s, const double *__restrict__ xe, int n_x,
                                                  unsigned long long *counts) {
    __shared__ StTile s_rho[ST_TX + 2];
    __shared__ unsigned int s_cnt[LDS ? NCI_HIST_LDS : 1];   // (one counter nobody uses without LDS)
    if (LDS)
        for (int i = threadIdx.x; i < n_s * n_x; i += TPB) s_cnt[i] = 0u;   // (st_stage's barrier covers it)
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool inside = y < ny && z < nz;
#pragma unroll 2
    for (int tx = 0; tx < ST_TX; tx++) {
        int cell = -1;
        if (inside && x0 + tx < nx) {
            const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
            cell = nci_cell(nci_voxel(r, K), ts, n_s, xe, n_x);
        }
        if (LDS) {
            if (cell >= 0) atomicAdd(&s_cnt[cell], 1u);
        } else
            nci_count_wave(counts, cell);
    }
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_s * n_x; i += TPB)
            if (s_cnt[i]) atomicAdd(&counts[i], (unsigned long long)s_cnt[i]);
    }
}

template <bool LDS>
__global__ __launch_bounds__(TPB) void k_nci_hist_gather(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                         const double *__restrict__ ts, int n_s, const double *__restrict__ xe, int n_x,
                                                         unsigned long long *counts) {
    __shared__ unsigned int s_cnt[LDS ? NCI_HIST_LDS : 1];   // (one counter nobody uses without LDS)
    if (LDS) {
        for (int i = threadIdx.x; i < n_s * n_x; i += TPB) s_cnt[i] = 0u;
        __syncthreads();
    }
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    int cell = -1;
    if (v < nx * nyz) {
        const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
        const StGatherReader r(rho, x, y, z, nx, ny, nz);
        cell = nci_cell(nci_voxel(r, K), ts, n_s, xe, n_x);
    }
    if (LDS) {
        if (cell >= 0) atomicAdd(&s_cnt[cell], 1u);
    } else
        nci_count_wave(counts, cell);
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_s * n_x; i += TPB)
            if (s_cnt[i]) atomicAdd(&counts[i], (unsigned long long)s_cnt[i]);
    }
}
