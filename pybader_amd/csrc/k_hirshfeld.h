// k_hirshfeld.h -- device kernel of libbader_hip.so: Hirshfeld (stockholder) weights from radial pro-atom tables -- the sums per
// atom, the promolecular density and the deformation density (xb_hirshfeld_sum / xb_hirshfeld_field, host_hirshfeld.h; the
// definition is in include/bader_hip.h and DESIGN.md section 19).  Included by bader_hip.hip (one translation unit).
#pragma once

// One workgroup of 256 threads handles one tile of 8 x 8 x 8 voxels (the part of it the grid holds), two voxels per thread, laid
// out as k_voronoi's: wave w takes the x-planes w and w + 4, a lane the voxel (y, z) = (lane / 8, lane % 8) of either.
//
// Phase 1, the candidate list.  c = the centre of the tile's voxels, R = half the longest body diagonal of the box they span.
// Image i of species s is kept iff  d_c(i) <= r_cut[s] + R + slack:  |d(v, i) - d_c(i)| <= R for a voxel v of the tile, so a
// dropped image lies at or beyond r_cut from every voxel of the tile and its term is the exact zero of the definition.
//
// SLACK (k_cell.h derives it, with lim = r_cut + R).  rc2 = r_cut * r_cut carries one u, its root half of one: a voxel with
// computed d2(v, i) < rc2 has  D(c, i) <= (r_cut + R) (1 + 8 u) + 28 u L.  Here the slack only has to be conservative: an image
// kept without need adds +0 to every voxel -- time, not bits.
//
// THE ORDER MATTERS (unlike k_voronoi's): P and p_a are running sums in the canonical order of the image list.  The survivors
// are compacted deterministically, a round of 256 images at a time: a ballot per wave, the four wave counts through LDS (two sets
// of counts in turn, so one barrier per round), a prefix over the waves -- no atomic.  Image idx of round r lands behind every
// survivor with a smaller idx.
//
// LDS.  XB_HIRSHFELD_CAND_MAX = 256 candidates of 48 B (q, rc2, inv_h2, atom, species) are 12 KiB; the bins of the sums (two
// doubles and the atom per slot -- a tile's candidates belong to at most as many atoms as it has candidates) 5 KiB; with the wave
// counts and the two words of the rest 17 456 B per workgroup for the sums, 12 320 B for the fields.  The field kernels compile to
// 64 VGPRs and no scratch: eight workgroups -- 32 waves, every wave slot of a compute unit -- on 96 KiB of the 160 KiB.  The sums'
// kernel compiles to 70 VGPRs and no scratch: seven workgroups on 119 KiB (held to 64 registers it spilled 36 bytes per lane,
// hence the bound of seven waves in __launch_bounds__).  A cap of 512 would leave four.  At bench.py's 216 atoms in 6 A with
// r_cut = 3 A a 512^3 tile keeps 136 images at most; 256 holds that.
//
// Phase 2.  Pass 1 forms P of the thread's two voxels over the candidates in order (a wave-uniform LDS address: broadcast reads);
// the field kernels store P or rho - P and end.  Pass 2 of the sums forms p_a over each run of candidates of one atom, w_a = p_a / P
// and term_a = rho * w_a, adds the two voxels' values, reduces them over the wave with shuffles -- skipped, by a ballot, when no
// lane of the wave is reached by the atom: it would add zeros -- and adds the wave's sums into the LDS bins of the atom's slot in
// the tile's list; the workgroup flushes its non-empty bins with one global atomic each after the tile.  A WORKGROUP OF THE SUMS
// TAKES MANY TILES (blockIdx.x, + gridDim.x, ...; at most HS_ROUNDS * HS_SUM_WAVES workgroups per compute unit), and with at most XB_HIRSHFELD_CAND_MAX atoms the
// bins are indexed by the ATOM instead, live over all its tiles and are flushed once at its end.  Measured at 512^3: with a
// workgroup and a flush per tile the 2 n atomics from each of 262 144 tiles onto 2 n addresses took 11 of the sum's 15 ms for 8
// atoms (all 16 words lie in one cache line).  Exactly as many workgroups as were thought to fit at once (2048) removed that but
// cost the fields and the 216-atom sums 20 %: the tiles' costs differ and nothing evens them out.  So the sums launch four times
// as many workgroups as fit, which the dispatcher deals out as others end, and the fields, which have no bins, one per tile.
//
// A tile with more survivors than the cap, or every tile with XB_HIRSHFELD_FULL_SEARCH, runs over the whole image list from
// global memory instead (wave-uniform addresses): the same expressions in the same order, hence the same bits; its wave sums go
// to global memory directly.
//
// The tables stay in global memory, as (f[k], f[k+1] - f[k]) pairs: one 16-byte load per term, the same bits as the definition's
// expression (the difference is formed on the host in IEEE float64).
#define HS_TILE 8
#define HS_SUM_WAVES 7   // waves per SIMD the sums' kernel is bounded to: as many workgroups (of four waves) per compute unit
#define HS_ROUNDS 4      // a sums launch has at most HS_ROUNDS times the workgroups the device holds at once (host_hirshfeld.h)
enum { HS_SUM = 0, HS_PRO = 1, HS_DEF = 2 };

struct HsCand { double q[3]; double rc2, ih2; int a, s; };   // 48 B
struct HsImage { double q[3]; int a, s; };                   // 32 B, the list of the setup

struct HsGeom : CellGeom {
    const HsImage *img;       // the canonical image list
    const double *sp;         // per species: r_cut, rc2, inv_h2
    const double2 *pairs;     // per species K pairs (f[k], f[k+1] - f[k])
    unsigned int n_img;
    int K;
};

// the term of one image at one voxel, and its shell (-1: d2 >= rc2); pr = nullptr (k_isa's counting pass): the shell alone
__device__ __forceinline__ double hs_term(const double pc[3], double q0, double q1, double q2, double rc2, double ih2,
                                          const double2 *__restrict__ pr, int K, int &shell) {
    const double d2 = cell_d2(pc, q0, q1, q2);
    shell = -1;
    if (d2 >= rc2) return 0.;
    const double u = d2 * ih2;
    const int k = min((int)u, K - 1);
    shell = k;
    if (!pr) return 0.;
    const double t = u - (double)k;
    const double2 f = pr[k];
    return f.x + t * f.y;
}
__device__ __forceinline__ double hs_term(const double pc[3], double q0, double q1, double q2, double rc2, double ih2,
                                          const double2 *__restrict__ pr, int K) {
    int shell;
    __builtin_assume(pr != nullptr);   // (the Hirshfeld kernels always have a table: no test of it per term)
    return hs_term(pc, q0, q1, q2, rc2, ih2, pr, K, shell);
}
__device__ __forceinline__ double hs_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// the two voxels of a thread in phase 2 (cell_two_voxels), their P and their density
struct HsVox : CellVox {
    double Pa, Pb, ra, rb;
};

// one atom's run is over: w_a and term_a of the two voxels, over the wave; lane 0 gets the sums (false: the wave holds none)
__device__ __forceinline__ bool hs_close_run(const HsVox &V, double pa_, double pb_, double &tc, double &tv) {
    const bool hit = (V.oka && pa_ > 0.) || (V.okb && pb_ > 0.);
    if (!__ballot(hit)) return false;
    const double wa = (V.oka && V.Pa > 0.) ? pa_ / V.Pa : 0., wb = (V.okb && V.Pb > 0.) ? pb_ / V.Pb : 0.;
    const double ta = (V.oka && V.Pa > 0.) ? V.ra * wa : 0., tb = (V.okb && V.Pb > 0.) ? V.rb * wb : 0.;
    tc = hs_wave_sum(ta + tb);
    tv = hs_wave_sum(wa + wb);
    return true;
}

// phase 1 of one tile (every thread of the workgroup calls it: its barriers are uniform): the survivors of the image list, compacted
// in list order into s_cand; -> how many survive (more than the cap: the list holds the first XB_HIRSHFELD_CAND_MAX and is not used)
__device__ __forceinline__ unsigned int hs_candidates(const HsGeom &G, int x0, int y0, int z0, HsCand *s_cand, unsigned int (*s_wcnt)[4],
                                                      unsigned int *stats) {
    const int tid = threadIdx.x, lane = tid % XB_WAVE, wave = tid / XB_WAVE;
    unsigned int cnt = 0;
    double c[3];
    const double R = 0.5 * sqrt(cell_tile_ball<HS_TILE>(G, x0, y0, z0, c));
    // keep and compact in the list's order (every thread runs every round: the barrier is uniform; n_img + 256 fits 32 bits)
    int flip = 0;
    for (unsigned int base = 0; base < G.n_img; base += 256u, flip ^= 1) {
        const unsigned int idx = base + tid;
        bool keep = false;
        HsImage im = {};
        double rc2 = 0., ih2 = 0.;
        if (idx < G.n_img) {
            im = G.img[idx];
            const double *sp = G.sp + 3 * (size_t)im.s;
            rc2 = sp[1]; ih2 = sp[2];
            keep = cell_d2(c, im.q[0], im.q[1], im.q[2]) <= cell_slack2(sp[0] + R, G.len);
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wcnt[flip][wave] = (unsigned int)__popcll(mask);
        __syncthreads();
        const unsigned int w0 = s_wcnt[flip][0], w1 = s_wcnt[flip][1], w2 = s_wcnt[flip][2], w3 = s_wcnt[flip][3];
        const unsigned int before = wave == 0 ? 0u : (wave == 1 ? w0 : (wave == 2 ? w0 + w1 : w0 + w1 + w2));
        const unsigned int slot = cnt + before + (unsigned int)__popcll(mask & ((1ull << lane) - 1ull));
        if (keep && slot < (unsigned int)XB_HIRSHFELD_CAND_MAX) {
            HsCand &d = s_cand[slot];
            d.q[0] = im.q[0]; d.q[1] = im.q[1]; d.q[2] = im.q[2];
            d.rc2 = rc2; d.ih2 = ih2; d.a = im.a; d.s = im.s;
        }
        cnt += (w0 + w1) + (w2 + w3);
    }
    if (tid == 0) {
        if (cnt > *(volatile unsigned int *)&stats[1]) atomicMax(&stats[1], cnt);
        if (cnt > (unsigned int)XB_HIRSHFELD_CAND_MAX) atomicAdd(&stats[0], 1u);
    }
    return cnt;
}

// pass 1: P of the two voxels, over the tile's candidates in order or (full) over the whole list
__device__ __forceinline__ void hs_total(const HsGeom &G, HsVox &V, const HsCand *s_cand, unsigned int cnt, bool full) {
    V.Pa = 0.; V.Pb = 0.;
    if (!full) {
#pragma unroll 2
        for (unsigned int k = 0; k < cnt; k++) {
            const HsCand &d = s_cand[k];
            const double q0 = d.q[0], q1 = d.q[1], q2 = d.q[2], rc2 = d.rc2, ih2 = d.ih2;
            const double2 *pr = G.pairs + (size_t)d.s * G.K;
            V.Pa += hs_term(V.pa, q0, q1, q2, rc2, ih2, pr, G.K);
            V.Pb += hs_term(V.pb, q0, q1, q2, rc2, ih2, pr, G.K);
        }
    } else {
        for (unsigned int k = 0; k < G.n_img; k++) {
            const HsImage im = G.img[k];
            const double *sp = G.sp + 3 * (size_t)im.s;
            const double rc2 = sp[1], ih2 = sp[2];
            const double2 *pr = G.pairs + (size_t)im.s * G.K;
            V.Pa += hs_term(V.pa, im.q[0], im.q[1], im.q[2], rc2, ih2, pr, G.K);
            V.Pb += hs_term(V.pb, im.q[0], im.q[1], im.q[2], rc2, ih2, pr, G.K);
        }
    }
}

// acc (HS_SUM): charge[n], then volume[n], then the rest's density sum; restn: its voxel count.  out (HS_PRO, HS_DEF): N doubles.
// stats: [0] tiles answered by the full search, [1] the largest candidate count (both untouched when `forced`)
template <int MODE>
__global__ __launch_bounds__(256, MODE == HS_SUM ? HS_SUM_WAVES : 8) void k_hirshfeld(HsGeom G, const double *__restrict__ rho, int forced, int n_atoms,
                                                   double *__restrict__ acc, unsigned long long *__restrict__ restn,
                                                   double *__restrict__ out, unsigned int *stats) {
    __shared__ HsCand s_cand[XB_HIRSHFELD_CAND_MAX];
    __shared__ double s_binc[MODE == HS_SUM ? XB_HIRSHFELD_CAND_MAX : 1], s_binv[MODE == HS_SUM ? XB_HIRSHFELD_CAND_MAX : 1];
    __shared__ int s_bina[MODE == HS_SUM ? XB_HIRSHFELD_CAND_MAX : 1];
    __shared__ double s_rest;
    __shared__ unsigned int s_restn;
    __shared__ unsigned int s_wcnt[2][4];
    const int tid = threadIdx.x, lane = tid % XB_WAVE;
    if (MODE == HS_SUM) {
        s_binc[tid] = 0.; s_binv[tid] = 0.;
        if (tid == 0) { s_rest = 0.; s_restn = 0u; }
    }
    static_assert(XB_HIRSHFELD_CAND_MAX == 256, "a bin per thread");
    // few atoms: a bin per ATOM, kept over all the tiles of this workgroup and flushed once; more: a bin per slot of the tile's list
    const bool by_atom = n_atoms <= XB_HIRSHFELD_CAND_MAX;
    const int ntiles = G.ntx * G.nty * G.ntz;
    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        int x0, y0, z0;
        cell_tile_origin<HS_TILE>(G, tile, x0, y0, z0);
        const unsigned int cnt = forced ? 0u : hs_candidates(G, x0, y0, z0, s_cand, s_wcnt, stats);
        __syncthreads();   // the candidates and the cleared bins
        const bool full = forced || cnt > (unsigned int)XB_HIRSHFELD_CAND_MAX;
        // phase 2: this thread's two voxels (indices clamped into the grid; a voxel outside it is neither stored nor summed)
        HsVox V;
        cell_two_voxels<HS_TILE>(G, x0, y0, z0, V);
        hs_total(G, V, s_cand, cnt, full);   // pass 1: P
        if (MODE != HS_SUM) {
            if (V.oka) out[V.va] = MODE == HS_PRO ? V.Pa : rho[V.va] - V.Pa;
            if (V.okb) out[V.vb] = MODE == HS_PRO ? V.Pb : rho[V.vb] - V.Pb;
        }
        int nslots = 0;
        if (MODE == HS_SUM) {
            V.ra = V.oka ? rho[V.va] : 0.;
            V.rb = V.okb ? rho[V.vb] : 0.;
            // the rest: voxels no pro-atom reaches
            {
                const bool za = V.oka && !(V.Pa > 0.), zb = V.okb && !(V.Pb > 0.);
                if (__ballot(za || zb)) {
                    const double s = hs_wave_sum((za ? V.ra : 0.) + (zb ? V.rb : 0.));
                    const unsigned int m = (unsigned int)__popcll(__ballot(za)) + (unsigned int)__popcll(__ballot(zb));
                    if (lane == 0) { atomicAdd(&s_rest, s); atomicAdd(&s_restn, m); }
                }
            }
            // pass 2: p_a over each run of one atom.  A run of atom `cur` is over (every lane calls it): close the run, and lane 0 adds
            // the wave's sums into the atom's bin -- s_binc, s_binv[bin] in LDS, or its result in global memory
            int cur = -1;
            double pa_ = 0., pb_ = 0.;
            auto add_run = [&](bool lds, int bin) {
                double tc, tv;
                if (cur < 0 || !hs_close_run(V, pa_, pb_, tc, tv) || lane != 0) return;
                if (lds) { atomicAdd(&s_binc[bin], tc); atomicAdd(&s_binv[bin], tv); }
                else { atomicAdd(&acc[cur], tc); atomicAdd(&acc[n_atoms + cur], tv); }
            };
            if (!full) {
                for (unsigned int k = 0; k < cnt; k++) {
                    const HsCand &d = s_cand[k];
                    const int a = d.a;
                    if (a != cur) {
                        add_run(true, by_atom ? cur : nslots - 1);
                        if (tid == 0 && !by_atom) s_bina[nslots] = a;
                        nslots++;
                        cur = a; pa_ = 0.; pb_ = 0.;
                    }
                    const double q0 = d.q[0], q1 = d.q[1], q2 = d.q[2], rc2 = d.rc2, ih2 = d.ih2;
                    const double2 *pr = G.pairs + (size_t)d.s * G.K;
                    pa_ += hs_term(V.pa, q0, q1, q2, rc2, ih2, pr, G.K);
                    pb_ += hs_term(V.pb, q0, q1, q2, rc2, ih2, pr, G.K);
                }
                add_run(true, by_atom ? cur : nslots - 1);
            } else {
                for (unsigned int k = 0; k <= G.n_img; k++) {   // (one step past the list closes the last run)
                    const bool end = k == G.n_img;
                    const HsImage im = G.img[end ? 0u : k];
                    if (end || im.a != cur) {
                        add_run(by_atom, cur);
                        if (end) break;
                        cur = im.a; pa_ = 0.; pb_ = 0.;
                    }
                    const double *sp = G.sp + 3 * (size_t)im.s;
                    const double rc2 = sp[1], ih2 = sp[2];
                    const double2 *pr = G.pairs + (size_t)im.s * G.K;
                    pa_ += hs_term(V.pa, im.q[0], im.q[1], im.q[2], rc2, ih2, pr, G.K);
                    pb_ += hs_term(V.pb, im.q[0], im.q[1], im.q[2], rc2, ih2, pr, G.K);
                }
                nslots = 0;   // (no slot bins on this route)
            }
        }
        __syncthreads();   // every wave is done with the candidates; the tile's bins are complete
        if (MODE == HS_SUM && !by_atom && tid < nslots) {   // (nslots <= cnt <= 256: a bin per thread)
            if (s_binc[tid] != 0. || s_binv[tid] != 0.) {
                const int a = s_bina[tid];
                atomicAdd(&acc[a], s_binc[tid]);
                atomicAdd(&acc[n_atoms + a], s_binv[tid]);
            }
            s_binc[tid] = 0.; s_binv[tid] = 0.;   // (the next tile's first atomic lies behind its own barrier)
        }
    }
    if (MODE != HS_SUM) return;
    if (by_atom && tid < n_atoms && (s_binc[tid] != 0. || s_binv[tid] != 0.)) {
        atomicAdd(&acc[tid], s_binc[tid]);
        atomicAdd(&acc[n_atoms + tid], s_binv[tid]);
    }
    if (tid == 0 && s_restn) {
        atomicAdd(&acc[2 * (size_t)n_atoms], s_rest);
        atomicAdd(restn, (unsigned long long)s_restn);
    }
}
