// k_igm.h -- device kernels of libbader_hip.so: IGM, the independent gradient model on the table terms of a Hirshfeld or ISA setup
// -- delta-g and delta-g_inter as fields, and the sums of a region val >= cut per label and class (xb_igm_field / xb_igm_sum,
// host_igm.h; the definition is in include/bader_hip.h and DESIGN.md section 27).  Included by bader_hip.hip (one translation
// unit) behind k_hirshfeld.h, whose candidate list, images and geometry it uses (and does not change), k_cell.h (a thread's two
// voxels) and k_stencil.h (the gather reader, the coefficients, the wave-uniform label reduction and the LDS bins).
#pragma once

// k_igm<MODE, F> has the shape of k_hirshfeld's field modes: a workgroup of 256 threads per 8^3 tile, hs_candidates in list
// order (12 KiB of LDS and the wave counts: 12 320 B), cell_two_voxels.  What is new is the pass over the (voxel, image) pairs: it
// keeps VECTORS -- per voxel the gradient sums of all images (gP), of the current atom's run (gp_a), of all atoms (g), of their
// magnitudes (gI) and of each of F fragments (gF) -- where k_hirshfeld keeps two scalars.
//   XB_IGM_PRO          one pass: P (the floor's test) over every image; p_a, gp_a over each run of an atom with a fragment
//   XB_IGM_STOCKHOLDER  pass 1 forms P and gP; then rho and section 18's gradient gr through StGatherReader (7 loads per voxel
//                       against roughly a hundred table terms); pass 2 forms p_a, gp_a per run and closes it with
//                       ga = w gr + rho ((gp_a - w gP) / P)
// A run is one atom's images: the list is in atom order, so is every tile's candidate list, and the atoms are closed ascending.
// The atom, its fragment and the image are uniform over the workgroup (scalar loads, scalar branches); whether an atom reaches a
// voxel (p_a > 0) is per lane.  The fragment accumulators are registers: F is a compile-time 2 or 4 (a caller's 1 or 3 is mapped
// up: an empty fragment adds +0.0 to gX, which changes no bit of a sum of magnitudes), the fragment selects its accumulator by
// F uniform comparisons, and no array is indexed by a run-time value.
//
// A tile over XB_HIRSHFELD_CAND_MAX, or every tile with XB_HIRSHFELD_FULL_SEARCH, reads the whole image list from global memory
// (IgmSrcAll) instead of the candidates in LDS (IgmSrcLds); igm_tile is one template over the two, so both routes form the same
// expressions in the same order: the same bits.  An image beyond its cutoff is skipped, not added as a zero.
//
// REGISTERS.  A voxel's state is 1 + 3 (P, gP) + 1 + 3 (p_a, gp_a) + 3 + 3 + 3 F (g, gI, gF) + 4 (rho, gr) + 3 (position) doubles,
// 33 for F = 4 in STOCKHOLDER mode -- 66 VGPRs a voxel before a single temporary, and a thread carries two voxels (they share
// every read of the candidate list).  Held to 128 registers such a kernel would spill, so the larger instantiations are bounded
// to fewer waves instead (IGM_WAVES): the choice is lower occupancy, not one voxel at a time, and none uses scratch (DESIGN.md
// section 27 lists what the compiler reports).  The run is closed in line, at one place: through a lambda called from two the
// accumulators were kept in scratch.  All stores are plain vector stores; there are no atomics but the two statistics words of
// hs_candidates, and no workgroup waits for another.
enum { IGM_PRO = 0, IGM_STOCKHOLDER = 1 };

// the term of one image at one voxel: T, and G = the gradient of the table's own interpolant; false: d2 >= rc2, nothing
__device__ __forceinline__ bool igm_term(const double pc[3], double q0, double q1, double q2, double rc2, double ih2,
                                         const double2 *__restrict__ pr, int K, double &T, double Gv[3]) {
    const double e0 = pc[0] - q0, e1 = pc[1] - q1, e2 = pc[2] - q2;
    const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
    if (d2 >= rc2) return false;
    const double u = d2 * ih2;
    const int k = min((int)u, K - 1);
    const double t = u - (double)k;
    const double2 f = pr[k];
    T = f.x + t * f.y;
    const double sl = f.y * ih2;
    const double c = sl + sl;
    Gv[0] = c * e0; Gv[1] = c * e1; Gv[2] = c * e2;
    return true;
}
__device__ __forceinline__ double igm_nrm(const double v[3]) { return sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]); }

struct IgmImage { double q0, q1, q2, rc2, ih2; const double2 *pr; int a; };
// where the images come from: the tile's candidates in LDS, or the whole list in global memory
struct IgmSrcLds {
    const HsCand *cand;
    __device__ __forceinline__ IgmImage get(const HsGeom &G, unsigned int k) const {
        const HsCand &d = cand[k];
        return IgmImage{d.q[0], d.q[1], d.q[2], d.rc2, d.ih2, G.pairs + (size_t)d.s * G.K, d.a};
    }
};
struct IgmSrcAll {
    __device__ __forceinline__ IgmImage get(const HsGeom &G, unsigned int k) const {
        const HsImage im = G.img[k];
        const double *sp = G.sp + 3 * (size_t)im.s;
        return IgmImage{im.q[0], im.q[1], im.q[2], sp[1], sp[2], G.pairs + (size_t)im.s * G.K, im.a};
    }
};

// NV voxels of this thread (positions pc, clamped coordinates xyz, linear indices at, flags ok) against n images of S
template <int MODE, int F, int NV, class Src>
__device__ __forceinline__ void igm_tile(const HsGeom &G, const Src &S, unsigned int n, const double (*pc)[3], const int (*xyz)[3],
                                         const size_t *at, const bool *ok, const double *__restrict__ rho, const int *__restrict__ frag,
                                         const StCoeffs &K, double p_min, double *__restrict__ dg, double *__restrict__ dgi) {
    double P[NV], gP[NV][3], r[NV], gr[NV][3], iP[NV];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        P[v] = 0.; r[v] = 0.; iP[v] = 0.;
#pragma unroll
        for (int j = 0; j < 3; j++) { gP[v][j] = 0.; gr[v][j] = 0.; }
    }
    if (MODE == IGM_STOCKHOLDER) {
        for (unsigned int k = 0; k < n; k++) {   // pass 1: P and gP
            const IgmImage im = S.get(G, k);
#pragma unroll
            for (int v = 0; v < NV; v++) {
                double T, Gv[3];
                if (igm_term(pc[v], im.q0, im.q1, im.q2, im.rc2, im.ih2, im.pr, G.K, T, Gv)) {
                    P[v] += T;
                    gP[v][0] += Gv[0]; gP[v][1] += Gv[1]; gP[v][2] += Gv[2];
                }
            }
        }
#pragma unroll
        for (int v = 0; v < NV; v++) {
            if (!(P[v] > p_min)) continue;   // (not reached: +0.0 is stored, whatever pass 2 forms)
            iP[v] = 1.0 / P[v];
            const StGatherReader R(rho, xyz[v][0], xyz[v][1], xyz[v][2], G.nx, G.ny, G.nz);
            r[v] = R(0, 0, 0);
            const double g0 = R(1, 0, 0) - R(-1, 0, 0), g1 = R(0, 1, 0) - R(0, -1, 0), g2 = R(0, 0, 1) - R(0, 0, -1);
#pragma unroll
            for (int al = 0; al < 3; al++) gr[v][al] = ((K.t[3 * al] * g0) + K.t[3 * al + 1] * g1) + K.t[3 * al + 2] * g2;
        }
    }
    // the runs: p_a and gp_a of one atom's images, closed into g, gI and gF[fragment] when the atom changes
    double pa[NV], gpa[NV][3], g[NV][3], gI[NV][3], gF[NV][F][3];
#pragma unroll
    for (int v = 0; v < NV; v++) {
        pa[v] = 0.;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            gpa[v][j] = 0.; g[v][j] = 0.; gI[v][j] = 0.;
#pragma unroll
            for (int f = 0; f < F; f++) gF[v][f][j] = 0.;
        }
    }
    int cur = -1, fr = -1;
    for (unsigned int k = 0; k <= n; k++) {   // (one step past the images closes the last run)
        const bool end = k == n;
        const IgmImage im = S.get(G, end ? 0u : k);
        if (end || im.a != cur) {
            if (fr >= 0) {   // (not before the first run, not an atom of no fragment)
#pragma unroll
                for (int v = 0; v < NV; v++) {
                    if (!(pa[v] > 0.)) continue;
                    double ga[3];
                    if (MODE == IGM_PRO) {
                        ga[0] = gpa[v][0]; ga[1] = gpa[v][1]; ga[2] = gpa[v][2];
                    } else {
                        const double w = pa[v] * iP[v];
#pragma unroll
                        for (int j = 0; j < 3; j++) ga[j] = w * gr[v][j] + r[v] * ((gpa[v][j] - w * gP[v][j]) * iP[v]);
                    }
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        g[v][j] += ga[j];
                        gI[v][j] += fabs(ga[j]);
                    }
#pragma unroll
                    for (int f = 0; f < F; f++)
                        if (fr == f) { gF[v][f][0] += ga[0]; gF[v][f][1] += ga[1]; gF[v][f][2] += ga[2]; }
                }
            }
            if (end) break;
            cur = im.a; fr = frag[cur];
#pragma unroll
            for (int v = 0; v < NV; v++) { pa[v] = 0.; gpa[v][0] = 0.; gpa[v][1] = 0.; gpa[v][2] = 0.; }
        }
        if (MODE == IGM_STOCKHOLDER && fr < 0) continue;   // (it entered P and gP in pass 1)
#pragma unroll
        for (int v = 0; v < NV; v++) {
            double T, Gv[3];
            if (igm_term(pc[v], im.q0, im.q1, im.q2, im.rc2, im.ih2, im.pr, G.K, T, Gv)) {
                if (MODE == IGM_PRO) P[v] += T;
                if (fr >= 0) {
                    pa[v] += T;
                    gpa[v][0] += Gv[0]; gpa[v][1] += Gv[1]; gpa[v][2] += Gv[2];
                }
            }
        }
    }
#pragma unroll
    for (int v = 0; v < NV; v++) {
        if (!ok[v]) continue;
        const bool reached = P[v] > p_min;
        const double ng = igm_nrm(g[v]);
        if (dg) dg[at[v]] = reached ? igm_nrm(gI[v]) - ng : 0.;
        if (dgi) {
            double gX[3];
#pragma unroll
            for (int j = 0; j < 3; j++) {
                gX[j] = fabs(gF[v][0][j]) + fabs(gF[v][1][j]);
#pragma unroll
                for (int f = 2; f < F; f++) gX[j] += fabs(gF[v][f][j]);
            }
            dgi[at[v]] = reached ? igm_nrm(gX) - ng : 0.;
        }
    }
}

// waves per SIMD the instantiations are bounded to; with them the compiler reports 114 (PRO, F = 2), 138 (PRO, F = 4), 159
// (STOCKHOLDER, F = 2) and 181 (STOCKHOLDER, F = 4) VGPRs and no scratch: 4, 3, 3 and 2 workgroups per compute unit
#define IGM_WAVES(MODE, F) ((MODE) == IGM_STOCKHOLDER || (F) == 4 ? 2 : 4)
// dg, dgi: N doubles each, either may be null.  frag: the fragment of every atom of the setup.  stats: hs_candidates' two words
template <int MODE, int F>
__global__ __launch_bounds__(256, IGM_WAVES(MODE, F)) void k_igm(HsGeom G, const double *__restrict__ rho, const int *__restrict__ frag,
                                                                 StCoeffs K, double p_min, int forced, double *__restrict__ dg,
                                                                 double *__restrict__ dgi, unsigned int *stats) {
    static_assert(F == 2 || F == 4, "the fragment accumulators are instantiated for 2 and 4");
    __shared__ HsCand s_cand[XB_HIRSHFELD_CAND_MAX];
    __shared__ unsigned int s_wcnt[2][4];
    int x0, y0, z0;
    cell_tile_origin<HS_TILE>(G, blockIdx.x, x0, y0, z0);
    const unsigned int cnt = forced ? 0u : hs_candidates(G, x0, y0, z0, s_cand, s_wcnt, stats);
    __syncthreads();   // the candidates
    const bool full = forced || cnt > (unsigned int)XB_HIRSHFELD_CAND_MAX;
    CellVox V;
    cell_two_voxels<HS_TILE>(G, x0, y0, z0, V);
    // the clamped coordinates of the two voxels, as cell_two_voxels forms them (the gather reader wants them)
    const int lane = threadIdx.x % XB_WAVE, wave = threadIdx.x / XB_WAVE;
    const int cy = min(y0 + lane / HS_TILE, G.ny - 1), cz = min(z0 + lane % HS_TILE, G.nz - 1);
    const int cxa = min(x0 + wave, G.nx - 1), cxb = min(x0 + wave + HS_TILE / 2, G.nx - 1);
    const double pc[2][3] = {{V.pa[0], V.pa[1], V.pa[2]}, {V.pb[0], V.pb[1], V.pb[2]}};
    const int xyz[2][3] = {{cxa, cy, cz}, {cxb, cy, cz}};
    const size_t at[2] = {V.va, V.vb};
    const bool ok[2] = {V.oka, V.okb};
    if (!full) igm_tile<MODE, F, 2>(G, IgmSrcLds{s_cand}, cnt, pc, xyz, at, ok, rho, frag, K, p_min, dg, dgi);
    else igm_tile<MODE, F, 2>(G, IgmSrcAll{}, G.n_img, pc, xyz, at, ok, rho, frag, K, p_min, dg, dgi);
}

// ---- the sums of a region per label and class ----------------------------------------------------------------------------------
// One streaming pass over the resident density and labels and two device fields: val (the region is val >= cut, decided on the
// STORED value) and x (the class, as xb_nci_sum's: x < -rho_split, in between, x > rho_split).  A block takes IGM_SUM_STEPS
// consecutive runs of TPB voxels; a wave's step goes through st_step2 of k_stencil.h under the key 3 a + class, so a wave whose
// voxels share a key adds into registers.  sum (rho), sv (val), cnt: [3 n] each, zero on entry.  BINS: 3 n <= ST_BINS and the
// adds go to LDS (5 120 B: eight workgroups per compute unit), the block's non-empty bins to global memory at its end.
#define IGM_SUM_STEPS 8
template <bool BINS>
__global__ __launch_bounds__(TPB) void k_igm_sum(long long N, const double *__restrict__ rho, const int *__restrict__ labels,
                                                 const double *__restrict__ val, const double *__restrict__ x, int n, double cut,
                                                 double rho_split, double *sum, double *sv, unsigned long long *cnt) {
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;   // (one bin nobody uses without BINS)
    if (BINS) {
        st_bins_clear(s_bins, 3 * n);
        __syncthreads();
    }
    StAcc A;
    const long long base = (long long)blockIdx.x * (IGM_SUM_STEPS * TPB) + threadIdx.x;
#pragma unroll 2
    for (int i = 0; i < IGM_SUM_STEPS; i++) {
        const long long v = base + (long long)i * TPB;
        int key = -1;
        double s = 0., m = 0.;
        if (v < N) {
            const int a = labels[v];
            if (a >= 0 && a < n) {
                const double f = val[v];
                if (f >= cut) {
                    const double c = x[v];
                    key = 3 * a + (c < -rho_split ? 0 : (c > rho_split ? 2 : 1));
                    s = rho[v]; m = f;
                }
            }
        }
        if (BINS) st_step2(s_bins.sink(), A, key, s, m);
        else st_step2(StSinkGlb{sum, sv, cnt}, A, key, s, m);
    }
    if (BINS) {
        st_finish(s_bins.sink(), A);
        __syncthreads();
        st_bins_flush(s_bins, 3 * n, sum, sv, cnt);
    } else
        st_finish(StSinkGlb{sum, sv, cnt}, A);
}
