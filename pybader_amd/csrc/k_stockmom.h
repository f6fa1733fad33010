// k_stockmom.h -- device kernel of libbader_hip.so: the atomic multipoles and radial moments of a stockholder partition -- charge,
// dipole, second moments, <r^3> and <r^4> of every atom's share w_a rho, on whichever setup is current: Hirshfeld or ISA (the radial
// tables of k_hirshfeld.h) or MBIS (the Slater shells of k_mbis.h) (xb_stockholder_moments, host_stockmom.h; the definition is in
// include/bader_hip.h and DESIGN.md section 25).  Included by bader_hip.hip after k_mbis.h; it calls k_hirshfeld.h's phase 1, term and
// pass 1, k_mbis.h's terms and k_cell.h's voxels, and edits none of them.
#pragma once

// k_stockmom runs the tile of k_hirshfeld and k_mbis: phase 1 (hs_candidates, in list order), the two voxels of a thread
// (cell_two_voxels), pass 1 for P -- hs_total on a table setup, k_mbis's loop on a Slater one: the same expressions in the same order,
// hence the P those kernels form -- and pass 2 over each run of one atom's images.
//   SM_COUNT    count[a] += 1 per pair with d2 < rc2 (no density, no P): what a plain Hirshfeld setup lacks, once per setup
//   SM_MOMENTS  a pair's twelve integer shares go into the atom's twelve bins
// KIND says what the term of an image is: SM_TABLE hs_term, SM_SLATER mbis_terms' T with r = sqrt(d2) (MS as k_mbis's: it sizes
// the registers of the shells' terms, not the results).
//
// As in k_mbis every lane of a wave adds to the same few integers of an atom: the twelve int64 partial sums of the current run stay
// in registers and at the end of the run -- skipped, by a ballot, when no lane was reached -- are reduced over the wave with shuffles;
// lane 0 adds them into LDS integer bins: a row per ATOM when n rows fit (kept over all the tiles of the workgroup, flushed once), a
// row per slot of the tile's list otherwise (flushed and cleared after the tile), one global 64-bit atomic per non-zero bin.  Runs
// beyond the LDS rows, tiles that run over the whole list without per-atom rows, and every pair with XB_STOCKMOM_DIRECT go to global
// memory directly.  All bins are INTEGERS: the order of the adds is free and every route gives the same bits.
// LDS: the candidates (12 KiB), SM_LDS_WORDS words of bins (16 KiB: 170 rows of twelve), the slots' atoms, the wave counts.
// No workgroup waits for another, nothing depends on a fresh plain load (the bins are reached by atomics alone, the results are
// read after the launch), and every store is a vector store or an atomic.
#define SM_LDS_WORDS 2048
#define SM_BINS 12
enum { SM_COUNT = 0, SM_MOMENTS = 1 };
enum { SM_TABLE = 0, SM_SLATER = 1 };

struct SmArgs {
    MbisArgs mb;                // SM_SLATER: E, cis, shells, Jd, KEd, M of the current parameters (nothing else of it is read)
    unsigned long long *bins;   // SM_MOMENTS: [n][SM_BINS];  SM_COUNT: count[n]
    unsigned long long *viol;   // the voxels whose density is not within rho_bound
    double rho_bound;
    int n_atoms;
    int e[5];                   // E0 .. E4
    int direct;                 // one global atomic per pair and bin
};

struct SmImg { double q0, q1, q2, rc2, ih2; int a, s; };
// image k of the tile's candidates or (full) of the whole list; k is wave-uniform, atom and species come back so
__device__ __forceinline__ SmImg sm_image(const HsGeom &G, const HsCand *s_cand, unsigned int k, bool full) {
    SmImg o;
    if (full) {
        const HsImage im = G.img[k];
        const double *sp = G.sp + 3 * (size_t)im.s;
        o.q0 = im.q[0]; o.q1 = im.q[1]; o.q2 = im.q[2]; o.rc2 = sp[1]; o.ih2 = sp[2]; o.a = im.a; o.s = im.s;
    } else {
        const HsCand &d = s_cand[k];
        o.q0 = d.q[0]; o.q1 = d.q[1]; o.q2 = d.q[2]; o.rc2 = d.rc2; o.ih2 = d.ih2; o.a = d.a; o.s = d.s;
    }
    o.a = __builtin_amdgcn_readfirstlane(o.a);
    o.s = __builtin_amdgcn_readfirstlane(o.s);
    return o;
}

// one (voxel, image) pair of pass 2: its twelve shares go into acc or, with `row`, out with global atomics; -> the lane holds
// something in acc
template <int KIND, int MS>
__device__ __forceinline__ bool sm_pair(bool ok, const double pc[3], const SmImg &im, int m, const double2 *__restrict__ cis, const HsGeom &G,
                                        const SmArgs &A, double P, double rh, long long (&acc)[SM_BINS], unsigned long long *row) {
    if (!ok || !(P > 0.)) return false;
    const double e0 = pc[0] - im.q0, e1 = pc[1] - im.q1, e2 = pc[2] - im.q2;
    const double d2 = cell_d2(pc, im.q0, im.q1, im.q2);   // (= (e0*e0 + e1*e1) + e2*e2 of these e)
    if (!(d2 < im.rc2)) return false;
    const double r = sqrt(d2);
    double T;
    if (KIND == SM_TABLE) T = hs_term(pc, im.q0, im.q1, im.q2, im.rc2, im.ih2, G.pairs + (size_t)im.s * G.K, G.K);
    else {
        double t[MS];
        T = mbis_terms<MS>(r, m, cis, A.mb, t);
    }
    if (!(T > 0.)) return false;
    const double w = T / P, s = rh * w;
    const double t0 = s * e0, t1 = s * e1, t2 = s * e2, u = s * d2;
    long long q[SM_BINS];
    q[0] = llrint(ldexp(s, A.e[0]));
    q[1] = llrint(ldexp(t0, A.e[1])); q[2] = llrint(ldexp(t1, A.e[1])); q[3] = llrint(ldexp(t2, A.e[1]));
    q[4] = llrint(ldexp(t0 * e0, A.e[2])); q[5] = llrint(ldexp(t0 * e1, A.e[2])); q[6] = llrint(ldexp(t0 * e2, A.e[2]));
    q[7] = llrint(ldexp(t1 * e1, A.e[2])); q[8] = llrint(ldexp(t1 * e2, A.e[2])); q[9] = llrint(ldexp(t2 * e2, A.e[2]));
    q[10] = llrint(ldexp(u * r, A.e[3]));
    q[11] = llrint(ldexp(u * d2, A.e[4]));
#pragma unroll
    for (int j = 0; j < SM_BINS; j++) {
        if (row) {
            if (q[j] != 0) atomicAdd(&row[j], (unsigned long long)q[j]);
        } else acc[j] += q[j];
    }
    return row == nullptr;
}

// stats: [0] tiles answered by the full search, [1] the largest candidate count (both untouched when `forced`)
template <int MODE, int KIND, int MS>
__global__ __launch_bounds__(256) void k_stockmom(HsGeom G, const double *__restrict__ rho, int forced, SmArgs A, unsigned int *stats) {
    constexpr int NB = MODE == SM_COUNT ? 1 : SM_BINS;
    constexpr int CAP = MODE == SM_COUNT ? 1 : SM_LDS_WORDS / SM_BINS;
    static_assert(CAP <= XB_HIRSHFELD_CAND_MAX, "no more rows than a tile's list has slots");
    __shared__ HsCand s_cand[XB_HIRSHFELD_CAND_MAX];
    __shared__ unsigned long long s_bins[CAP * NB];
    __shared__ int s_bina[CAP];
    __shared__ unsigned int s_wcnt[2][4];
    const int tid = threadIdx.x, lane = tid % XB_WAVE;
    if (MODE == SM_MOMENTS)
        for (int j = tid; j < CAP * NB; j += 256) s_bins[j] = 0ull;
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
        HsVox V;
        cell_two_voxels<HS_TILE>(G, x0, y0, z0, V);
        V.Pa = 0.; V.Pb = 0.; V.ra = 0.; V.rb = 0.;
        if (MODE == SM_MOMENTS) {
            // pass 1: P, as the setup's own kernel forms it
            if (KIND == SM_TABLE) hs_total(G, V, s_cand, cnt, full);
            else
                for (unsigned int k = 0; k < m_img; k++) {
                    const MbisImg im = mbis_image(G, s_cand, k, full);
                    const int m = A.mb.shells[im.a];
                    const double2 *cis = A.mb.cis + (size_t)im.a * A.mb.M;
                    double t[MS];
                    const double da = cell_d2(V.pa, im.q0, im.q1, im.q2), db = cell_d2(V.pb, im.q0, im.q1, im.q2);
                    if (da < im.rc2) V.Pa += mbis_terms<MS>(sqrt(da), m, cis, A.mb, t);
                    if (db < im.rc2) V.Pb += mbis_terms<MS>(sqrt(db), m, cis, A.mb, t);
                }
            V.ra = V.oka ? rho[V.va] : 0.;
            V.rb = V.okb ? rho[V.vb] : 0.;
            // a density beyond the bound could overflow a bin: such a voxel adds nothing and makes the call fail
            const bool xa = V.oka && !(fabs(V.ra) <= A.rho_bound), xb = V.okb && !(fabs(V.rb) <= A.rho_bound);
            if (xa) V.oka = false;
            if (xb) V.okb = false;
            const unsigned long long ma = __ballot(xa), mb = __ballot(xb);
            if ((ma | mb) && lane == 0) atomicAdd(A.viol, (unsigned long long)(__popcll(ma) + __popcll(mb)));
        }
        // pass 2 over each run of one atom.  The run of atom `cur` is over (every lane calls it): the wave's sums go into row `bin`
        // of the LDS bins, or with bin < 0 into the atom's row in global memory
        int nslots = 0, cur = -1, m = 0, bin = -1;
        const double2 *cis = nullptr;
        bool hit = false;
        long long acc[SM_BINS];
#pragma unroll
        for (int j = 0; j < SM_BINS; j++) acc[j] = 0;
        auto close_run = [&]() {
            if (cur < 0 || !__ballot(hit)) return;
            if (MODE == SM_COUNT) {
                const long long v = mbis_wave_sum(acc[0]);
                if (lane == 0) atomicAdd(&A.bins[cur], (unsigned long long)v);
            } else {
                unsigned long long *lds = &s_bins[(bin < 0 ? 0 : bin) * NB], *glb = A.bins + (size_t)cur * NB;
#pragma unroll
                for (int j = 0; j < NB; j++) {
                    const long long v = mbis_wave_sum(acc[j]);
                    if (lane == 0 && v != 0) atomicAdd(bin < 0 ? &glb[j] : &lds[j], (unsigned long long)v);
                }
            }
#pragma unroll
            for (int j = 0; j < SM_BINS; j++) acc[j] = 0;
            hit = false;
        };
        for (unsigned int k = 0; k < m_img; k++) {
            const SmImg im = sm_image(G, s_cand, k, full);
            if (im.a != cur) {
                close_run();
                cur = im.a;
                if (MODE == SM_MOMENTS) {
                    if (KIND == SM_SLATER) {
                        m = A.mb.shells[cur];
                        cis = A.mb.cis + (size_t)cur * A.mb.M;
                    }
                    if (by_atom) bin = cur;
                    else if (full) bin = -1;
                    else {
                        bin = nslots < CAP ? nslots : -1;
                        if (tid == 0 && nslots < CAP) s_bina[nslots] = cur;
                        nslots++;
                    }
                }
            }
            if (MODE == SM_COUNT) {
                const int ca = (V.oka && cell_d2(V.pa, im.q0, im.q1, im.q2) < im.rc2) + (V.okb && cell_d2(V.pb, im.q0, im.q1, im.q2) < im.rc2);
                acc[0] += ca;
                hit = hit || ca != 0;
            } else {
                unsigned long long *row = A.direct ? A.bins + (size_t)cur * NB : nullptr;
                const bool ha = sm_pair<KIND, MS>(V.oka, V.pa, im, m, cis, G, A, V.Pa, V.ra, acc, row);
                const bool hb = sm_pair<KIND, MS>(V.okb, V.pb, im, m, cis, G, A, V.Pb, V.rb, acc, row);
                hit = hit || ha || hb;
            }
        }
        close_run();
        __syncthreads();   // every wave is done with the candidates; the tile's bins are complete
        if (MODE == SM_MOMENTS && !by_atom) {
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
    if (MODE != SM_MOMENTS || !by_atom) return;
    for (int j = tid; j < A.n_atoms * NB; j += 256) {
        const unsigned long long v = s_bins[j];
        if (v != 0ull) atomicAdd(&A.bins[j], v);
    }
}
