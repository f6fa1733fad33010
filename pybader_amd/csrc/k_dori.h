// k_dori.h -- device kernels of libbader_hip.so: DORI, the density overlap regions indicator, over the resident density -- gamma
// and sign(lambda2) rho as fields, and the sums of the region gamma >= d_cut per label and class (xb_dori_field / xb_dori_sum,
// host_dori.h; the definition is in include/bader_hip.h and DESIGN.md section 26).  Included by bader_hip.hip (one translation
// unit) behind k_nci.h, whose nci_sign it uses, and k_stencil.h, whose tile, readers, staging and wave sums it uses.
#pragma once

// One function, dori_voxel, forms (rho, N, S, whether the Hessian is not zero, sigma) of a voxel from a reader; the tile route
// hands it an StTileReader, the gather route (XB_STENCIL_GATHER) an StGatherReader, so both run the same expressions in the same
// order: the same bits.  rho^6 cancels between N and D, so gamma = N / (N + D) is multiplications, additions and one division of
// the voxel's ten stencil values: no sqrt, no cbrt, no eigen-solve, and gamma itself is bit-defined.
//
// LDS per workgroup and workgroups per compute unit (160 KiB = 163 840 B, the arithmetic of k_stencil.h's header):
//   k_dori_field          the tile, 10 x 10 x 34 doubles = 27 200 B: six (163 200 B), as k_nci_field
//   k_dori_sum<true>      the tile + StBins<ST_BINS> (256 keys x 20 B = 5 120 B) = 32 320 B: five, as k_nci_sum<true>;
//                         3 n <= ST_BINS keys, n <= NCI_LABELS_LDS = 85
//   k_dori_sum<false>     the tile (the unused bin is dropped by the compiler): six
//   the gather kernels    no tile: 0 B (field) and 5 120 B (sums), eight workgroups -- every wave slot -- per compute unit
static_assert((ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2) * 8 <= 160 * 1024 / 6, "six workgroups per compute unit (the field)");
static_assert((ST_TX + 2) * (ST_TY + 2) * (ST_TZ + 2) * 8 + ST_BINS * 20 <= 160 * 1024 / 5, "five workgroups per compute unit (the sums)");
static_assert(3 * NCI_LABELS_LDS <= ST_BINS, "the keys 3 a + class of NCI_LABELS_LDS labels fit the LDS bins");

struct DoriVoxel {
    double rho, n, s;   // the density, N and S = N + D of the definition
    bool curved;        // some component of the Hessian is not 0
    int sig;            // the sign of the Hessian's middle eigenvalue (nci_sign): -1, 0, +1; 0 when no colour is asked
};

// colour: sigma is wanted (uniform over the launch)
template <class R>
__device__ __forceinline__ DoriVoxel dori_voxel(const R &r, const StCoeffs &K, bool colour = true) {
    const double c = r(0, 0, 0);
    double d[6], g[3], H[6];
    st_second(r, c, d);
    const double g0 = r(1, 0, 0) - r(-1, 0, 0), g1 = r(0, 1, 0) - r(0, -1, 0), g2 = r(0, 0, 1) - r(0, 0, -1);
#pragma unroll
    for (int al = 0; al < 3; al++) g[al] = ((K.t[3 * al] * g0) + K.t[3 * al + 1] * g1) + K.t[3 * al + 2] * g2;
#pragma unroll
    for (int k = 0; k < 6; k++) H[k] = st_dot6(K.h + 6 * k, d);
    const double xx = H[0], xy = H[1], xz = H[2], yy = H[3], yz = H[4], zz = H[5];
    const double gg = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
    const double h0 = (xx * g[0] + xy * g[1]) + xz * g[2];
    const double h1 = (xy * g[0] + yy * g[1]) + yz * g[2];
    const double h2 = (xz * g[0] + yz * g[1]) + zz * g[2];
    const double u0 = c * h0 - gg * g[0], u1 = c * h1 - gg * g[1], u2 = c * h2 - gg * g[2];
    DoriVoxel v;
    v.rho = c;
    v.n = 4.0 * ((u0 * u0 + u1 * u1) + u2 * u2);
    v.s = v.n + (gg * gg) * gg;
    v.curved = (xx != 0.) | (xy != 0.) | (xz != 0.) | (yy != 0.) | (yz != 0.) | (zz != 0.);
    v.sig = 0;
    if (colour) {
        const double I1 = (xx + yy) + zz;
        const double I2 = ((xx * yy - xy * xy) + (xx * zz - xz * xz)) + (yy * zz - yz * yz);
        const double I3 = (xx * (yy * zz - yz * yz) - xy * (xy * zz - yz * xz)) + xz * (xy * yz - yy * xz);
        v.sig = nci_sign(I1, I2, I3);
    }
    return v;
}

// gamma of the definition: 0 where rho is not above rho_min (NaN, +0, -0, negative), N / S where S > 0 is finite, 1 at a critical
// point of the discrete field (S == 0 with a Hessian that is not zero), 0 elsewhere (a flat field, an overflow, a NaN)
__device__ __forceinline__ double dori_gamma(const DoriVoxel &v, double rho_min) {
    if (!(v.rho > rho_min)) return 0.;
    if (v.s > 0. && v.s < __builtin_huge_val()) return v.n / v.s;
    return v.s == 0. && v.curved ? 1. : 0.;
}
// x = sigma rho where rho > rho_min, +0 elsewhere
__device__ __forceinline__ double dori_colour(const DoriVoxel &v, double rho_min) {
    return v.rho > rho_min ? (double)v.sig * v.rho : 0.;
}

// ---- the fields -------------------------------------------------------------------------------------------------------------------
// x_out may be null: gamma alone
__global__ __launch_bounds__(TPB) void k_dori_field(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K, double rho_min,
                                                    double *__restrict__ g_out, double *__restrict__ x_out) {
    __shared__ StTile s_rho[ST_TX + 2];
    int x0, y0, z0;
    st_stage(s_rho, nx, ny, nz, rho, x0, y0, z0);
    const int tz = threadIdx.x % ST_TZ, ty = threadIdx.x / ST_TZ;
    const int y = y0 + ty, z = z0 + tz;
    if (y >= ny || z >= nz) return;
    const bool colour = x_out != nullptr;
#pragma unroll 2
    for (int tx = 0; tx < ST_TX; tx++) {
        const int x = x0 + tx;
        if (x >= nx) break;
        const StTileReader r{s_rho, tx + 1, ty + 1, tz + 1};
        const DoriVoxel v = dori_voxel(r, K, colour);
        const long long at = ((long long)x * ny + y) * nz + z;
        g_out[at] = dori_gamma(v, rho_min);
        if (colour) x_out[at] = dori_colour(v, rho_min);
    }
}

__global__ __launch_bounds__(TPB) void k_dori_field_gather(int nx, int ny, int nz, const double *__restrict__ rho, StCoeffs K,
                                                           double rho_min, double *__restrict__ g_out, double *__restrict__ x_out) {
    const long long at = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    if (at >= nx * nyz) return;
    const int x = (int)(at / nyz), q = (int)(at - x * nyz), y = q / nz, z = q - y * nz;
    const StGatherReader r(rho, x, y, z, nx, ny, nz);
    const bool colour = x_out != nullptr;
    const DoriVoxel v = dori_voxel(r, K, colour);
    g_out[at] = dori_gamma(v, rho_min);
    if (colour) x_out[at] = dori_colour(v, rho_min);
}

// ---- the region's sums per label and class ------------------------------------------------------------------------------------
struct DoriCuts {
    double d_cut, rho_min, rho_split;   // d_cut in (0, 1]: a voxel of the region has rho > rho_min
};
// the key 3 a + class of a voxel with label a in [0, n) inside the region, else -1: the comparison the stored field would meet
__device__ __forceinline__ int dori_key(const DoriVoxel &v, int a, const DoriCuts &C) {
    if (!(dori_gamma(v, C.rho_min) >= C.d_cut)) return -1;
    const double x = dori_colour(v, C.rho_min);
    return 3 * a + (x < -C.rho_split ? 0 : (x > C.rho_split ? 2 : 1));
}

// BINS: 3 n <= ST_BINS and the adds go to LDS.  sum (rho), sq (rho^2), cnt: [3 n] each, zero on entry
template <bool BINS>
__global__ __launch_bounds__(TPB) void k_dori_sum(int nx, int ny, int nz, const double *__restrict__ rho, const int *__restrict__ labels,
                                                  int n, StCoeffs K, DoriCuts C, double *sum, double *sq, unsigned long long *cnt) {
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
                const DoriVoxel v = dori_voxel(r, K);
                key = dori_key(v, a, C);
                if (key >= 0) { s = v.rho; m = v.rho * v.rho; }
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
__global__ __launch_bounds__(TPB) void k_dori_sum_gather(int nx, int ny, int nz, const double *__restrict__ rho,
                                                         const int *__restrict__ labels, int n, StCoeffs K, DoriCuts C, double *sum,
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
            const DoriVoxel w = dori_voxel(r, K);
            key = dori_key(w, a, C);
            if (key >= 0) { s = w.rho; m = w.rho * w.rho; }
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
