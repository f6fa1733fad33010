// k_isa.h -- device kernels of libbader_hip.so: iterative stockholder atoms (ISA), Hirshfeld weights whose tables are the spherical
// averages of the atoms' own shares (xb_isa_setup / xb_isa_iterate, host_isa.h; the definition is in include/bader_hip.h and
// DESIGN.md section 23).  Included by bader_hip.hip after k_hirshfeld.h, whose phases it calls.
#pragma once

// k_isa runs k_hirshfeld's tile: phase 1 (hs_candidates), the two voxels of a thread (cell_two_voxels), pass 1 (hs_total, with the
// table pairs (A[a][k], +0.0): the same code, the same bits as the field kernels form).  Pass 2 is new: every (voxel, image) pair
// with a term gets its shell k (hs_term forms it with the term) and its integer share q, and q goes into bin[a][k].  The bins are
// 64-bit INTEGERS, so the order of the atomics is free and every bin is bit-defined; a negative q is added as its two's complement.
//   ISA_COUNT  q = 1 for every pair with d2 < rc2 (no density, no P): count[a][k], once per setup
//   ISA_SHELL  q = llrint(ldexp(rho * (term / P), e)) for P > 0 and term > 0
//
// Unlike the sums of section 19, the lanes of a wave hit DIFFERENT shells of one image.  Two routes, the same bins:
//   (a) direct      one global atomic per pair with q != 0.  Overflowing tiles and XB_HIRSHFELD_FULL_SEARCH always go this way.
//   (b) aggregated  per image, the wave's 128 voxels (two x-planes of the tile) span a contiguous run of shells.  Each WAVE keeps a
//                   window of ISA_WIN integer bins in LDS that starts at the smallest shell its lanes hit (a min over the wave),
//                   adds with LDS 64-bit atomics, and flushes the non-zero bins, ISA_WIN / 64 per lane, with one global atomic each after
//                   the image.  A pair beyond the window goes out directly.  The window belongs to one wave, so it needs no
//                   workgroup barrier: a wave-level fence orders its lanes' LDS operations.
// LDS: the candidates (12 KiB), the wave counts, 4 windows of ISA_WIN * 8 B = 8 KiB: 20 512 B, six workgroups per compute unit
// as the 75 VGPRs allow anyway.
#ifndef ISA_WIN
#define ISA_WIN 256   // (a multiple of the wave; measured at 512^3 with 64, 128, 256, 512: DESIGN.md section 23)
#endif
enum { ISA_COUNT = 0, ISA_SHELL = 1 };

struct IsaArgs {
    unsigned long long *bins;   // [n][K]: count (ISA_COUNT) or bin (ISA_SHELL)
    unsigned long long *viol;   // the voxels whose density is not within rho_bound
    double rho_bound;
    int e;
    int direct;                 // route (a) for every tile
};

// the integer share of one pair (0: none)
template <int MODE>
__device__ __forceinline__ long long isa_share(bool ok, int shell, double term, double P, double rho, int e) {
    if (!ok || shell < 0) return 0;
    if (MODE == ISA_COUNT) return 1;
    if (!(P > 0.) || !(term > 0.)) return 0;
    return llrint(ldexp(rho * (term / P), e));
}
__device__ __forceinline__ void isa_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int MODE>
__global__ __launch_bounds__(256) void k_isa(HsGeom G, const double *__restrict__ rho, int forced, IsaArgs A, unsigned int *stats) {
    __shared__ HsCand s_cand[XB_HIRSHFELD_CAND_MAX];
    __shared__ unsigned long long s_win[4][ISA_WIN];
    __shared__ unsigned int s_wcnt[2][4];
    const int tid = threadIdx.x, lane = tid % XB_WAVE, wave = tid / XB_WAVE;
    static_assert(ISA_WIN % XB_WAVE == 0, "a lane flushes every 64th bin of the window");
    for (int j = lane; j < ISA_WIN; j += XB_WAVE) s_win[wave][j] = 0ull;
    const int ntiles = G.ntx * G.nty * G.ntz;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int x0, y0, z0;
        cell_tile_origin<HS_TILE>(G, tile, x0, y0, z0);
        const unsigned int cnt = forced ? 0u : hs_candidates(G, x0, y0, z0, s_cand, s_wcnt, stats);
        __syncthreads();   // the candidates
        const bool full = forced || cnt > (unsigned int)XB_HIRSHFELD_CAND_MAX;
        HsVox V;
        cell_two_voxels<HS_TILE>(G, x0, y0, z0, V);
        V.Pa = 0.; V.Pb = 0.; V.ra = 0.; V.rb = 0.;
        if (MODE == ISA_SHELL) {
            hs_total(G, V, s_cand, cnt, full);
            V.ra = V.oka ? rho[V.va] : 0.;
            V.rb = V.okb ? rho[V.vb] : 0.;
            // a density beyond the bound could overflow a bin: such a voxel adds nothing and makes the call fail
            const bool xa = !(fabs(V.ra) <= A.rho_bound), xb = !(fabs(V.rb) <= A.rho_bound);
            if (xa) V.oka = false;
            if (xb) V.okb = false;
            const unsigned long long ma = __ballot(xa), mb = __ballot(xb);
            if ((ma | mb) && lane == 0) atomicAdd(A.viol, (unsigned long long)(__popcll(ma) + __popcll(mb)));
        }
        if (!full && !A.direct) {
            for (unsigned int i = 0; i < cnt; i++) {
                const HsCand &d = s_cand[i];
                const double2 *pr = MODE == ISA_SHELL ? G.pairs + (size_t)d.s * G.K : nullptr;
                int ka, kb;
                const double ta = hs_term(V.pa, d.q[0], d.q[1], d.q[2], d.rc2, d.ih2, pr, G.K, ka);
                const double tb = hs_term(V.pb, d.q[0], d.q[1], d.q[2], d.rc2, d.ih2, pr, G.K, kb);
                const long long qa = isa_share<MODE>(V.oka, ka, ta, V.Pa, V.ra, A.e), qb = isa_share<MODE>(V.okb, kb, tb, V.Pb, V.rb, A.e);
                if (!__ballot(qa != 0 || qb != 0)) continue;   // (wave-uniform)
                int kmin = min(qa != 0 ? ka : G.K, qb != 0 ? kb : G.K);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) kmin = min(kmin, __shfl_xor(kmin, o));
                unsigned long long *row = A.bins + (size_t)d.a * G.K;
                if (qa != 0) {
                    if (ka - kmin < ISA_WIN) atomicAdd(&s_win[wave][ka - kmin], (unsigned long long)qa);
                    else atomicAdd(&row[ka], (unsigned long long)qa);
                }
                if (qb != 0) {
                    if (kb - kmin < ISA_WIN) atomicAdd(&s_win[wave][kb - kmin], (unsigned long long)qb);
                    else atomicAdd(&row[kb], (unsigned long long)qb);
                }
                isa_wave_sync();
#pragma unroll
                for (int j = lane; j < ISA_WIN; j += XB_WAVE) {
                    const unsigned long long v = s_win[wave][j];
                    if (v != 0ull) {   // (then kmin + j is a shell some lane hit: below K)
                        s_win[wave][j] = 0ull;
                        atomicAdd(&row[kmin + j], v);
                    }
                }
                isa_wave_sync();
            }
        } else {
            const unsigned int m = full ? G.n_img : cnt;
            for (unsigned int i = 0; i < m; i++) {
                double q0, q1, q2, rc2, ih2;
                int a, s;
                if (full) {
                    const HsImage im = G.img[i];
                    const double *sp = G.sp + 3 * (size_t)im.s;
                    q0 = im.q[0]; q1 = im.q[1]; q2 = im.q[2]; rc2 = sp[1]; ih2 = sp[2]; a = im.a; s = im.s;
                } else {
                    const HsCand &d = s_cand[i];
                    q0 = d.q[0]; q1 = d.q[1]; q2 = d.q[2]; rc2 = d.rc2; ih2 = d.ih2; a = d.a; s = d.s;
                }
                const double2 *pr = MODE == ISA_SHELL ? G.pairs + (size_t)s * G.K : nullptr;
                int ka, kb;
                const double ta = hs_term(V.pa, q0, q1, q2, rc2, ih2, pr, G.K, ka);
                const double tb = hs_term(V.pb, q0, q1, q2, rc2, ih2, pr, G.K, kb);
                const long long qa = isa_share<MODE>(V.oka, ka, ta, V.Pa, V.ra, A.e), qb = isa_share<MODE>(V.okb, kb, tb, V.Pb, V.rb, A.e);
                unsigned long long *row = A.bins + (size_t)a * G.K;
                if (qa != 0) atomicAdd(&row[ka], (unsigned long long)qa);
                if (qb != 0) atomicAdd(&row[kb], (unsigned long long)qb);
            }
        }
        __syncthreads();   // every wave is done with the candidates
    }
}

// the bins become the next tables: A' = bin > 0 ? ldexp((double)bin / (double)count, -e) : 0 as the pair (A', +0.0) in `next`, the
// bins are cleared, qsum[a] += bin.  With a voxel beyond the bound (*viol != 0) `next` gets the OLD table instead: every table area
// then holds what the call found, whichever the later iterations of the call read.  total = n * K entries, one per thread.
__global__ __launch_bounds__(256) void k_isa_update(const long long *__restrict__ count, long long *__restrict__ bins,
                                                    const double2 *__restrict__ old, double2 *__restrict__ next,
                                                    unsigned long long *__restrict__ qsum, const unsigned long long *__restrict__ viol,
                                                    int K, long long total, int e) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = idx < total;
    const long long at = have ? idx : total - 1;
    const long long b = have ? bins[at] : 0;
    const int a = (int)(at / K);
    if (have) {
        double v = b > 0 ? ldexp((double)b / (double)count[at], -e) : 0.;
        if (*viol) v = old[at].x;
        next[at] = make_double2(v, 0.);
        bins[at] = 0;
    }
    // one atomic per wave where the wave lies within one atom's row
    if (__shfl(a, 0) == __shfl(a, XB_WAVE - 1)) {
        unsigned long long s = (unsigned long long)b;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (threadIdx.x % XB_WAVE == 0 && s != 0ull) atomicAdd(&qsum[a], s);
    } else if (b != 0) {
        atomicAdd(&qsum[a], (unsigned long long)b);
    }
}

// max |x| of a density as float64 bits (non-negative doubles order as their bit patterns; a NaN sorts above infinity)
__global__ __launch_bounds__(256) void k_isa_absmax(const double *__restrict__ rho, long long N, unsigned long long *out) {
    unsigned long long m = 0ull;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(fabs(rho[i]));
        m = b > m ? b : m;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long x = __shfl_xor(m, o);
        m = x > m ? x : m;
    }
    if (threadIdx.x % XB_WAVE == 0 && m != 0ull) atomicMax(out, m);
}
