// k_mbis.h -- device kernels of libbader_hip.so: minimal-basis iterative stockholder atoms (MBIS; Verstraelen et al. 2016), Hirshfeld
// weights whose pro-atoms are sums of a few Slater shells N/(8 pi sigma^3) exp(-r/sigma) fitted to the atoms' own shares
// (xb_mbis_setup / xb_mbis_iterate / xb_mbis_field, host_mbis.h; the definition is in include/bader_hip.h and DESIGN.md section 24).
// Included by bader_hip.hip after k_isa.h; it calls k_hirshfeld.h's phase 1 and k_cell.h's voxels.
#pragma once

// k_mbis runs k_hirshfeld's tile: phase 1 (hs_candidates, with species[a] = a: the cutoff is the atom's), the two voxels of a thread
// (cell_two_voxels).  The term of an image is new: r = sqrt(d2), and per shell of the atom u = (r/sigma) J, a lookup in the ONE shared
// table E[k] = exp(-k/J) held as pairs (E[k], E[k+1] - E[k]) -- no exp on the device.  The atom's (c, 1/sigma) pairs are read
// through a wave-uniform index (readfirstlane: scalar loads), the table per lane with one 16-byte load.
//   MBIS_COUNT  count[a] += 1 per pair with d2 < rc2[a] (no density, no P), once per setup
//   MBIS_FIELD  pass 1 alone: P or rho - P at every voxel
//   MBIS_SHELL  pass 1 forms P; pass 2 forms every pair's integer shares and adds them into the atom's 2 m + 1 bins
//
// Unlike ISA's (k_isa.h), every lane of a wave adds to THE SAME few integers of an atom.  Pass 2 therefore keeps the 2 MS + 1 int64
// partial sums of the current atom's run of images in registers (the list order groups images by atom), and at the end of the run
// -- skipped, by a ballot, when no lane was reached -- reduces them over the wave with shuffles; lane 0 adds them into LDS integer bins:
// a row per ATOM when n rows fit (kept over all the tiles of the workgroup, flushed once), a row per slot of the tile's list otherwise
// (flushed after the tile), one global 64-bit atomic per non-zero bin.  Runs beyond the LDS rows, tiles that run over the whole list
// without per-atom rows, and every pair with XB_MBIS_DIRECT go to global memory directly.  All bins are INTEGERS: the order of the
// adds is free and every route gives the same bits.  MS (1, 2, 4, 8) is the least of these that holds the setup's largest shell
// count: it sizes the registers and the rows, not the results.
// LDS: the candidates (12 KiB), at most MBIS_LDS_WORDS words of bins (16 KiB), the slots' atoms, the rest, the wave counts.
#define MBIS_LDS_WORDS 2048
#define MBIS_EIGHT_PI (8.0 * 3.14159265358979323846)
enum { MBIS_COUNT = 0, MBIS_SHELL = 1, MBIS_FIELD = 2 };

struct MbisArgs {
    const double2 *E;           // KE pairs (E[k], E[k+1] - E[k])
    const double2 *cis;         // [n][M] pairs (c, 1/sigma) of the current parameters
    const int *shells;          // [n]
    unsigned long long *bins;   // MBIS_SHELL: [n][2 MS + 1] (binN[MS], binS[MS], binV), then restq, restn;  MBIS_COUNT: count[n]
    unsigned long long *viol;   // the voxels whose density is not within rho_bound
    double *out;                // MBIS_FIELD: N doubles
    double rho_bound, Jd, KEd;  // J and KE as doubles
    int M, n_atoms;
    int eN, eS, eV, eR;
    int direct;                 // one global atomic per pair and shell
    int deform;                 // MBIS_FIELD: rho - P instead of P
};

// what a shell's (N, sigma) become for the kernel: the same expressions on the host (setup, load) and in k_mbis_update
__host__ __device__ inline void mbis_shell(double N, double sigma, double &c, double &is) {
    const double den = ((MBIS_EIGHT_PI * sigma) * sigma) * sigma;
    const double q = N / den;
    c = (N > 0. && __builtin_isfinite(q)) ? q : 0.;
    is = 1.0 / sigma;
}

// t_i of the atom's m shells at distance r, and T = ((0 + t_0) + t_1) + ...
template <int MS>
__device__ __forceinline__ double mbis_terms(double r, int m, const double2 *__restrict__ cis, const MbisArgs &A, double (&t)[MS]) {
    double T = 0.;
#pragma unroll
    for (int i = 0; i < MS; i++) {
        t[i] = 0.;
        if (i < m) {
            const double2 p = cis[i];
            const double u = (r * p.y) * A.Jd;
            if (u < A.KEd) {
                const int k = (int)u;
                const double w = u - (double)k;
                const double2 f = A.E[k];
                t[i] = p.x * (f.x + w * f.y);
            }
            T += t[i];
        }
    }
    return T;
}

struct MbisImg { double q0, q1, q2, rc2; int a; };
// image k of the tile's candidates or (full) of the whole list; the atom comes back wave-uniform
__device__ __forceinline__ MbisImg mbis_image(const HsGeom &G, const HsCand *s_cand, unsigned int k, bool full) {
    MbisImg o;
    if (full) {
        const HsImage im = G.img[k];
        o.q0 = im.q[0]; o.q1 = im.q[1]; o.q2 = im.q[2]; o.rc2 = G.sp[3 * (size_t)im.s + 1]; o.a = im.a;
    } else {
        const HsCand &d = s_cand[k];
        o.q0 = d.q[0]; o.q1 = d.q[1]; o.q2 = d.q[2]; o.rc2 = d.rc2; o.a = d.a;
    }
    o.a = __builtin_amdgcn_readfirstlane(o.a);
    return o;
}

__device__ __forceinline__ long long mbis_wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// one (voxel, image) pair of pass 2: its shares go into acc (binN[MS], binS[MS], binV) or, with `row`, out with global atomics;
// -> the lane holds something in acc
template <int MS>
__device__ __forceinline__ bool mbis_pair(bool ok, const double pc[3], const MbisImg &im, int m, const double2 *__restrict__ cis,
                                          const MbisArgs &A, double P, double rh, long long (&acc)[2 * MS + 1], unsigned long long *row) {
    if (!ok || !(P > 0.)) return false;
    const double d2 = cell_d2(pc, im.q0, im.q1, im.q2);
    if (!(d2 < im.rc2)) return false;
    const double r = sqrt(d2);
    double t[MS];
    const double T = mbis_terms<MS>(r, m, cis, A, t);
    if (!(T > 0.)) return false;   // (t_i <= T: no shell has a term either)
#pragma unroll
    for (int i = 0; i < MS; i++)
        if (i < m && t[i] > 0.) {
            const double s = rh * (t[i] / P);
            const long long qn = llrint(ldexp(s, A.eN)), qs = llrint(ldexp(r * s, A.eS));
            if (row) {
                if (qn != 0) atomicAdd(&row[i], (unsigned long long)qn);
                if (qs != 0) atomicAdd(&row[MS + i], (unsigned long long)qs);
            } else {
                acc[i] += qn; acc[MS + i] += qs;
            }
        }
    const long long qv = llrint(ldexp(T / P, A.eV));
    if (row) {
        if (qv != 0) atomicAdd(&row[2 * MS], (unsigned long long)qv);
        return false;
    }
    acc[2 * MS] += qv;
    return true;
}

// stats: [0] tiles answered by the full search, [1] the largest candidate count (both untouched when `forced`)
template <int MODE, int MS>
__global__ __launch_bounds__(256) void k_mbis(HsGeom G, const double *__restrict__ rho, int forced, MbisArgs A, unsigned int *stats) {
    constexpr int NB = 2 * MS + 1;
    constexpr int CAP = MODE != MBIS_SHELL ? 1 : (XB_HIRSHFELD_CAND_MAX * NB <= MBIS_LDS_WORDS ? XB_HIRSHFELD_CAND_MAX : MBIS_LDS_WORDS / NB);
    __shared__ HsCand s_cand[XB_HIRSHFELD_CAND_MAX];
    __shared__ unsigned long long s_bins[CAP * NB];
    __shared__ int s_bina[CAP];
    __shared__ unsigned long long s_rest;
    __shared__ unsigned int s_restn;
    __shared__ unsigned int s_wcnt[2][4];
    const int tid = threadIdx.x, lane = tid % XB_WAVE;
    if (MODE == MBIS_SHELL) {
        for (int j = tid; j < CAP * NB; j += 256) s_bins[j] = 0ull;
        if (tid == 0) { s_rest = 0ull; s_restn = 0u; }
    }
    // few atoms: a row per ATOM, kept over all the tiles of this workgroup and flushed once; more: a row per slot of the tile's list
    const bool by_atom = A.n_atoms <= CAP;
    const int ntiles = G.ntx * G.nty * G.ntz;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int x0, y0, z0;
        cell_tile_origin<HS_TILE>(G, tile, x0, y0, z0);
        const unsigned int cnt = forced ? 0u : hs_candidates(G, x0, y0, z0, s_cand, s_wcnt, stats);
        __syncthreads();   // the candidates and the cleared bins
        const bool full = forced || cnt > (unsigned int)XB_HIRSHFELD_CAND_MAX;
        const unsigned int m_img = full ? G.n_img : cnt;
        CellVox V;
        cell_two_voxels<HS_TILE>(G, x0, y0, z0, V);
        double Pa = 0., Pb = 0., ra = 0., rb = 0.;
        if (MODE != MBIS_COUNT) {   // pass 1: P
            for (unsigned int k = 0; k < m_img; k++) {
                const MbisImg im = mbis_image(G, s_cand, k, full);
                const int m = A.shells[im.a];
                const double2 *cis = A.cis + (size_t)im.a * A.M;
                double t[MS];
                const double da = cell_d2(V.pa, im.q0, im.q1, im.q2), db = cell_d2(V.pb, im.q0, im.q1, im.q2);
                if (da < im.rc2) Pa += mbis_terms<MS>(sqrt(da), m, cis, A, t);
                if (db < im.rc2) Pb += mbis_terms<MS>(sqrt(db), m, cis, A, t);
            }
        }
        if (MODE == MBIS_FIELD) {
            if (V.oka) A.out[V.va] = A.deform ? rho[V.va] - Pa : Pa;
            if (V.okb) A.out[V.vb] = A.deform ? rho[V.vb] - Pb : Pb;
        }
        int nslots = 0;
        if (MODE == MBIS_SHELL) {
            ra = V.oka ? rho[V.va] : 0.;
            rb = V.okb ? rho[V.vb] : 0.;
            // a density beyond the bound could overflow a bin: such a voxel adds nothing and makes the call fail
            const bool xa = !(fabs(ra) <= A.rho_bound), xb = !(fabs(rb) <= A.rho_bound);
            if (xa) V.oka = false;
            if (xb) V.okb = false;
            const unsigned long long ma = __ballot(xa), mb = __ballot(xb);
            if ((ma | mb) && lane == 0) atomicAdd(A.viol, (unsigned long long)(__popcll(ma) + __popcll(mb)));
            // the rest: voxels no atom reaches
            const bool za = V.oka && !(Pa > 0.), zb = V.okb && !(Pb > 0.);
            if (__ballot(za || zb)) {
                const long long s = mbis_wave_sum((za ? llrint(ldexp(ra, A.eR)) : 0ll) + (zb ? llrint(ldexp(rb, A.eR)) : 0ll));
                const unsigned int m = (unsigned int)__popcll(__ballot(za)) + (unsigned int)__popcll(__ballot(zb));
                if (lane == 0) { atomicAdd(&s_rest, (unsigned long long)s); atomicAdd(&s_restn, m); }
            }
        }
        if (MODE != MBIS_FIELD) {
            // pass 2 over each run of one atom.  The run of atom `cur` is over (every lane calls it): the wave's sums go into row
            // `bin` of the LDS bins, or with bin < 0 into the atom's row in global memory
            int cur = -1, m = 0, bin = -1;
            const double2 *cis = nullptr;
            bool hit = false;
            long long acc[NB];
#pragma unroll
            for (int j = 0; j < NB; j++) acc[j] = 0;
            auto close_run = [&]() {
                if (cur < 0 || !__ballot(hit)) return;
                if (MODE == MBIS_COUNT) {
                    const long long v = mbis_wave_sum(acc[0]);
                    if (lane == 0) atomicAdd(&A.bins[cur], (unsigned long long)v);
                } else {
                    unsigned long long *lds = &s_bins[(bin < 0 ? 0 : bin) * NB], *glb = A.bins + (size_t)cur * NB;
#pragma unroll
                    for (int j = 0; j < NB; j++) {
                        if (j < 2 * MS && j % MS >= m) continue;   // (wave-uniform: the atom has no such shell)
                        const long long v = mbis_wave_sum(acc[j]);
                        if (lane == 0 && v != 0) atomicAdd(bin < 0 ? &glb[j] : &lds[j], (unsigned long long)v);
                    }
                }
#pragma unroll
                for (int j = 0; j < NB; j++) acc[j] = 0;
                hit = false;
            };
            for (unsigned int k = 0; k < m_img; k++) {
                const MbisImg im = mbis_image(G, s_cand, k, full);
                if (im.a != cur) {
                    close_run();
                    cur = im.a;
                    if (MODE == MBIS_SHELL) {
                        m = A.shells[cur];
                        cis = A.cis + (size_t)cur * A.M;
                        if (by_atom) bin = cur;
                        else if (full) bin = -1;
                        else {
                            bin = nslots < CAP ? nslots : -1;
                            if (tid == 0 && nslots < CAP) s_bina[nslots] = cur;
                            nslots++;
                        }
                    }
                }
                if (MODE == MBIS_COUNT) {
                    const int ca = (V.oka && cell_d2(V.pa, im.q0, im.q1, im.q2) < im.rc2) + (V.okb && cell_d2(V.pb, im.q0, im.q1, im.q2) < im.rc2);
                    acc[0] += ca;
                    hit = hit || ca != 0;
                } else {
                    unsigned long long *row = A.direct ? A.bins + (size_t)cur * NB : nullptr;
                    const bool ha = mbis_pair<MS>(V.oka, V.pa, im, m, cis, A, Pa, ra, acc, row);
                    const bool hb = mbis_pair<MS>(V.okb, V.pb, im, m, cis, A, Pb, rb, acc, row);
                    hit = hit || ha || hb;
                }
            }
            close_run();
        }
        __syncthreads();   // every wave is done with the candidates; the tile's bins are complete
        if (MODE == MBIS_SHELL && !by_atom) {
            const int rows = min(nslots, CAP);
            for (int j = tid; j < rows * NB; j += 256) {
                const unsigned long long v = s_bins[j];
                if (v != 0ull) {
                    atomicAdd(&A.bins[(size_t)s_bina[j / NB] * NB + j % NB], v);
                    s_bins[j] = 0ull;   // (the next tile's first atomic lies behind its own barrier)
                }
            }
        }
    }
    if (MODE != MBIS_SHELL) return;
    if (by_atom)
        for (int j = tid; j < A.n_atoms * NB; j += 256) {
            const unsigned long long v = s_bins[j];
            if (v != 0ull) atomicAdd(&A.bins[j], v);
        }
    if (tid == 0 && s_restn) {
        atomicAdd(&A.bins[(size_t)A.n_atoms * NB], s_rest);
        atomicAdd(&A.bins[(size_t)A.n_atoms * NB + 1], (unsigned long long)s_restn);
    }
}

// The bins become the next parameters, one thread per (atom, shell): par = (c, 1/sigma)[n][M], then N[n][M], then sigma[n][M].
//   raw = ldexp((double)binN, -eN);  binN > 0: N' = raw*vv, s1 = ldexp((double)binS, -eS) / (3.0*raw), sigma' = s1 where binS > 0 and
//   s1 > 0 and finite, else sigma;  otherwise N' = 0, sigma' = sigma: a dead shell stays dead.
// With a voxel beyond the bound (*viol != 0) `next` gets the OLD parameters, with `keep` nothing.  row (zeroed by the caller):
// qsum[n], vsum[n], restq, restn of this iteration.  The bins are cleared.
__global__ __launch_bounds__(256) void k_mbis_update(unsigned long long *__restrict__ bins, const double *__restrict__ old, double *__restrict__ next,
                                                     unsigned long long *__restrict__ row, const unsigned long long *__restrict__ viol,
                                                     int n, int M, int MS, int eN, int eS, double vv, int keep) {
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x, nm = (long long)n * M;
    if (idx >= nm) return;
    const int a = (int)(idx / M), i = (int)(idx % M), NB = 2 * MS + 1;
    unsigned long long *b = bins + (size_t)a * NB;
    const long long bN = (long long)b[i], bS = (long long)b[MS + i];
    const double oN = old[2 * nm + idx], oS = old[3 * nm + idx];
    double N1 = 0., S1 = oS;
    if (bN > 0) {
        const double raw = ldexp((double)bN, -eN);
        N1 = raw * vv;
        const double s1 = ldexp((double)bS, -eS) / (3.0 * raw);
        if (bS > 0 && s1 > 0. && __builtin_isfinite(s1)) S1 = s1;
    }
    if (*viol) { N1 = oN; S1 = oS; }
    if (!keep) {
        double c, is;
        mbis_shell(N1, S1, c, is);
        reinterpret_cast<double2 *>(next)[idx] = make_double2(c, is);
        next[2 * nm + idx] = N1;
        next[3 * nm + idx] = S1;
    }
    b[i] = 0ull; b[MS + i] = 0ull;
    if (bN != 0) atomicAdd(&row[a], (unsigned long long)bN);
    if (i == 0) { row[n + a] = b[2 * MS]; b[2 * MS] = 0ull; }
    if (idx == 0) {
        unsigned long long *r = bins + (size_t)n * NB;
        row[2 * (size_t)n] = r[0]; row[2 * (size_t)n + 1] = r[1];
        r[0] = 0ull; r[1] = 0ull;
    }
}
