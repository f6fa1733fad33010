// k_moments.h -- device kernels of libbader_hip.so: zeroth, first and second moments of the density of every label about a centre
// (xb_moment_sum, host_moments.h; the definition is in include/bader_hip.h and DESIGN.md section 13).
// Included by bader_hip.hip (one translation unit).
#pragma once

// One pass over the owned voxels: 12 B read per voxel, the 27-image search and ten terms in float64.  What is summed is bit-defined;
// the sums are float atomics in any order (as k_charge_sum_*).
//
// Labels are spatially coherent, so a wave first asks whether all its voxels of this step carry ONE label.  While they do, every
// lane adds its terms into registers; the wave reduces them with shuffles and one lane adds the eleven numbers when the label
// changes or the wave ends.  A step with several labels is peeled label by label: a label that MS_GROUP lanes or more share is
// reduced with shuffles, a smaller group adds per lane.
//
// Two routes by the label count n, as k_charge_sum_lds / _glb:
//   n <= MS_BINS  the adds go to bins in LDS (ten doubles and a count per label), a block's non-empty bins to global memory at its end
//   any n         the adds go to global memory
// MS_BINS = 224: 224 * 84 B = 18.4 KiB per block, so eight blocks of 256 threads -- 32 waves, every wave slot of a compute unit -- fit
// the 160 KiB of LDS of a gfx950 compute unit (8 * 18.4 = 147 KiB); the next size that matters, 256 bins, would leave seven.
#define MS_BINS 224
#define MS_TERMS 10
#define MS_PER_THREAD 16   // voxels per thread: a block covers TPB * MS_PER_THREAD consecutive voxels
#define MS_GROUP 8         // lanes of one label in a mixed step from which a shuffle reduction replaces per-lane adds

// what the image search reads with a uniform index: pbc[i][j] of image i = (x + 1) * 9 + (y + 1) * 3 + (z + 1), computed on the
// host as (lat[j] * x + lat[3 + j] * y) + lat[6 + j] * z (IEEE, no contraction) and passed by value (scalar loads)
struct MsImages { double pbc[27][3]; };

// tab: the position table of k_ms_tables (k_cell.h); pbc_dev: MsImages again, for the one lookup by a per-lane index
struct MsGeom {
    const double *tab;
    const double *pbc_dev;
    const double *centres;   // n * 3
    int nx, ny, nz, nyz;
};

// the ten terms of voxel v with label a (0 <= a < n) and density w
__device__ __forceinline__ void ms_terms(const MsGeom &G, const MsImages &I, int v, int a, double w, double t[MS_TERMS]) {
    const int p0 = v / G.nyz;
    const int r = v - p0 * G.nyz;
    const int p1 = r / G.nz, p2 = r - p1 * G.nz;
    double pc[3], ce[3];
    cell_pos(G.tab, G.nx, G.ny, G.nz, p0, p1, p2, pc);
#pragma unroll
    for (int j = 0; j < 3; j++) ce[j] = G.centres[3 * (size_t)a + j];
    double best = 1.7976931348623157e308;
    int which = 0;
#pragma unroll
    for (int i = 0; i < 27; i++) {
        const double d2 = cell_d2(pc, ce[0] + I.pbc[i][0], ce[1] + I.pbc[i][1], ce[2] + I.pbc[i][2]);
        if (d2 < best) { best = d2; which = i; }
    }
    double d[3];
#pragma unroll
    for (int j = 0; j < 3; j++) d[j] = pc[j] - (ce[j] + G.pbc_dev[3 * which + j]);
    const double t0 = w * d[0], t1 = w * d[1], t2 = w * d[2];
    t[0] = w; t[1] = t0; t[2] = t1; t[3] = t2;
    t[4] = t0 * d[0]; t[5] = t0 * d[1]; t[6] = t0 * d[2];
    t[7] = t1 * d[1]; t[8] = t1 * d[2];
    t[9] = t2 * d[2];
}

// where a wave's sums go: bins in LDS or the result arrays
struct MsSinkLds {
    double *sum;          // [n][MS_TERMS]
    unsigned int *cnt;    // [n]
    __device__ __forceinline__ void add(int a, int k, double x) const { atomicAdd(&sum[a * MS_TERMS + k], x); }
    __device__ __forceinline__ void count(int a, unsigned int c) const { atomicAdd(&cnt[a], c); }
};
struct MsSinkGlb {
    double *sum;
    unsigned long long *cnt;
    __device__ __forceinline__ void add(int a, int k, double x) const { atomicAdd(&sum[(size_t)a * MS_TERMS + k], x); }
    __device__ __forceinline__ void count(int a, unsigned int c) const { atomicAdd(&cnt[a], (unsigned long long)c); }
};

// all lanes call it; t[] of the lanes outside `mine` must be zero; lane `leader` adds the wave's sums for label a
template <class Sink>
__device__ __forceinline__ void ms_wave_add(const Sink &S, int a, double t[MS_TERMS], unsigned int c, int leader) {
#pragma unroll
    for (int k = 0; k < MS_TERMS; k++)
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) t[k] += __shfl_xor(t[k], o);
    if ((int)(threadIdx.x % XB_WAVE) == leader) {
#pragma unroll
        for (int k = 0; k < MS_TERMS; k++) S.add(a, k, t[k]);
        S.count(a, c);
    }
}

template <class Sink>
__device__ __forceinline__ void ms_stream(const Sink &S, const Grid &g, const MsGeom &G, const MsImages &I,
                                          const double *__restrict__ rho, const int *__restrict__ labels, int n) {
    const long long vbeg = (long long)g.x0 * g.nyz, vend = (long long)g.x1 * g.nyz;
    long long v = vbeg + (long long)blockIdx.x * TPB * MS_PER_THREAD + threadIdx.x;
    double acc[MS_TERMS];
#pragma unroll
    for (int k = 0; k < MS_TERMS; k++) acc[k] = 0.;
    unsigned int acc_n = 0;   // voxels in acc, summed over the wave (uniform)
    int cur = -1;             // the label acc belongs to (uniform)
    for (int it = 0; it < MS_PER_THREAD; it++, v += TPB) {
        int a = -1;
        double t[MS_TERMS];
#pragma unroll
        for (int k = 0; k < MS_TERMS; k++) t[k] = 0.;
        if (v < vend) {
            a = labels[v];
            if (a >= 0 && a < n) ms_terms(G, I, (int)v, a, rho[v], t);
            else a = -1;
        }
        const unsigned long long act = __ballot(a >= 0);
        if (!act) continue;
        const int la = __shfl(a, __ffsll((long long)act) - 1);
        if (__ballot(a == la) == act) {   // one label in this step
            if (la != cur && cur >= 0) {
                ms_wave_add(S, cur, acc, acc_n, 0);
#pragma unroll
                for (int k = 0; k < MS_TERMS; k++) acc[k] = 0.;
                acc_n = 0;
            }
            cur = la;
#pragma unroll
            for (int k = 0; k < MS_TERMS; k++) acc[k] += t[k];
            acc_n += (unsigned int)__popcll(act);
            continue;
        }
        // several labels: peel them off one by one
        unsigned long long todo = act;
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lb = __shfl(a, leader);
            const bool mine = a == lb;
            const unsigned long long grp = __ballot(mine);
            const unsigned int c = (unsigned int)__popcll(grp);
            if (c >= MS_GROUP) {
                double u[MS_TERMS];
#pragma unroll
                for (int k = 0; k < MS_TERMS; k++) u[k] = mine ? t[k] : 0.;
                ms_wave_add(S, lb, u, c, leader);
            } else if (mine) {
#pragma unroll
                for (int k = 0; k < MS_TERMS; k++) S.add(a, k, t[k]);
                S.count(a, 1u);
            }
            todo &= ~grp;
        }
    }
    if (cur >= 0) ms_wave_add(S, cur, acc, acc_n, 0);
}

__global__ __launch_bounds__(TPB) void k_moment_sum_lds(Grid g, MsGeom G, MsImages I, const double *__restrict__ rho,
                                                        const int *__restrict__ labels, int n, double *sums,
                                                        unsigned long long *count) {
    __shared__ double sm[MS_BINS * MS_TERMS];
    __shared__ unsigned int sn[MS_BINS];
    for (int i = threadIdx.x; i < n * MS_TERMS; i += TPB) sm[i] = 0.;
    for (int i = threadIdx.x; i < n; i += TPB) sn[i] = 0;
    __syncthreads();
    ms_stream(MsSinkLds{sm, sn}, g, G, I, rho, labels, n);
    __syncthreads();
    for (int i = threadIdx.x; i < n * MS_TERMS; i += TPB)
        if (sn[i / MS_TERMS]) atomicAdd(&sums[i], sm[i]);
    for (int i = threadIdx.x; i < n; i += TPB)
        if (sn[i]) atomicAdd(&count[i], (unsigned long long)sn[i]);
}

__global__ __launch_bounds__(TPB) void k_moment_sum_glb(Grid g, MsGeom G, MsImages I, const double *__restrict__ rho,
                                                        const int *__restrict__ labels, int n, double *sums,
                                                        unsigned long long *count) {
    ms_stream(MsSinkGlb{sums, count}, g, G, I, rho, labels, n);
}
