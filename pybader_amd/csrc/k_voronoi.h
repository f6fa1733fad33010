// k_voronoi.h -- device kernel of libbader_hip.so: the Voronoi partition, every voxel to its nearest atom over the 27 periodic images
// (xb_voronoi_assign, host_voronoi.h; the definition is in include/bader_hip.h and DESIGN.md section 16).
// Included by bader_hip.hip (one translation unit).
#pragma once

// One workgroup of 256 threads handles one tile of 8 x 8 x 8 voxels (the part of it the grid holds), two voxels per thread: wave w
// takes the x-planes w and w + 4 of the tile, a lane the voxel (y, z) = (lane / 8, lane % 8) of either -- a row of eight labels is a
// whole 32-byte sector.  The cube is the tile of 512 voxels with the smallest circumradius, so it keeps the fewest candidates; the
// search is bound by float64 arithmetic (eight operations and the comparison per voxel and candidate), not by its 4 B per voxel of
// stores, so a z-longer tile would buy wider stores the kernel does not wait for at the price of more candidates.
//
// Phase 1, the candidate list.  c = the centre of the tile's voxels, R = half the longest body diagonal of the box they span (both
// from the voxel lattice, for the clipped extent of a tile the grid cuts).  With d_c(i) the distance from c to image i and d_min
// the smallest of them, image i is kept iff  d_c(i) <= d_min + 2 R + slack:  for a voxel v of the tile |d(v, i) - d_c(i)| <= R, so
// a dropped image is farther from every voxel of the tile than the image of d_min is.  Everything is compared squared; the one
// square root is d_min's.
//
// SLACK (k_cell.h derives it, with lim = d_min + 2 R).  Here it decides labels, so ties matter.  w wins, or ties in computed d2, at
// voxel v; m is the image of d_min.  computed d2(v, w) <= computed d2(v, m) gives  D(v, w) (1 - 3 u) <= D(v, m) (1 + 3 u),  hence
// D(c, w) <= D(c, m) + 2 R + (7 u + ...) (D(c, m) + 2 R) + 28 u L;  d_min's computed root adds one u.  The slack is about 1e-12 of
// the radius, so it keeps no candidate a sharp bound would drop unless the image is tied to that precision.  A computed tie
// satisfies the comparison like a win: an image tied with the winner is kept, so the lexicographic minimum of (d2, atom) over the
// candidates is the one over all images.
//
// The survivors go to LDS as q and the atom's index, compacted per wave by ballot and prefix count (their order is free: a
// lexicographic minimum does not depend on it).  XB_VORONOI_CAND_MAX = 512 candidates of 32 B are 16 KiB, with the image vectors and
// the reduction words 17 072 B per workgroup: eight workgroups -- 32 waves, every wave slot of a compute unit; the kernel compiles to
// 48 VGPRs, no scratch -- take 133 KiB of the 160 KiB of LDS.  (The image loop of the full search is kept rolled: unrolled 27 times
// it held 204 registers and two waves per SIMD.)
//
// Phase 2: every voxel runs over the LDS candidates (a wave-uniform address: one broadcast read) with the definition's expression.
// A tile with more survivors than the cap, or every tile with XB_VORONOI_FULL_SEARCH, runs over all 27 n images from global memory
// instead (the atom is wave-uniform there as well): the same expression on the same q, hence the same labels.
#define VO_TILE 8

struct VoCand { double q[3]; int a; int pad; };   // 32 B: two 16-byte LDS reads

struct VoGeom : CellGeom {
    const double *pbc;      // 27 image vectors, [i][j]
    const double *atoms;    // n * 3, Cartesian
    int n;
};

// the lexicographic minimum of (d2, a), in any order of the calls
__device__ __forceinline__ void vo_take(double d2, int a, double &best, int &who) {
    if (d2 < best || (d2 == best && a < who)) { best = d2; who = a; }
}

// stats: [0] tiles answered by the full search, [1] the largest candidate count (both untouched when `forced`)
__global__ __launch_bounds__(256) void k_voronoi(VoGeom G, const double *__restrict__ rho, int use_vac, double tol, int forced,
                                                 int *__restrict__ labels, unsigned int *stats) {
    __shared__ VoCand s_cand[XB_VORONOI_CAND_MAX];
    __shared__ double s_pbc[81];
    __shared__ double s_red[4];
    __shared__ int s_cnt;
    const int tid = threadIdx.x, lane = tid % XB_WAVE, wave = tid / XB_WAVE;
    int x0, y0, z0;
    cell_tile_origin<VO_TILE>(G, blockIdx.x, x0, y0, z0);
    if (tid < 81) s_pbc[tid] = G.pbc[tid];
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    const unsigned int total = 27u * (unsigned int)G.n;   // (n <= INT_MAX / 27, checked on the host: total + 256 fits 32 bits)
    int cnt = 0;
    if (!forced) {
        double c[3];
        const double two_r = sqrt(cell_tile_ball<VO_TILE>(G, x0, y0, z0, c));
        // pass 1: d_min
        double m2 = __builtin_huge_val();
        for (unsigned int idx = tid; idx < total; idx += 256u) {
            const int a = (int)(idx / 27u), i = (int)(idx - 27u * (unsigned int)a);
            const double *at = G.atoms + 3 * (size_t)a;
            m2 = fmin(m2, cell_d2(c, at[0] + s_pbc[3 * i], at[1] + s_pbc[3 * i + 1], at[2] + s_pbc[3 * i + 2]));
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m2 = fmin(m2, __shfl_xor(m2, o));
        if (lane == 0) s_red[wave] = m2;
        __syncthreads();
        m2 = fmin(fmin(s_red[0], s_red[1]), fmin(s_red[2], s_red[3]));
        const double lim2 = cell_slack2(sqrt(m2) + two_r, G.len);
        // pass 2: keep and compact (every lane of a wave runs the same number of rounds)
        for (unsigned int base = 0; base < total; base += 256u) {
            const unsigned int idx = base + tid;
            bool keep = false;
            double q0 = 0., q1 = 0., q2 = 0.;
            int a = 0;
            if (idx < total) {
                a = (int)(idx / 27u);
                const int i = (int)(idx - 27u * (unsigned int)a);
                const double *at = G.atoms + 3 * (size_t)a;
                q0 = at[0] + s_pbc[3 * i]; q1 = at[1] + s_pbc[3 * i + 1]; q2 = at[2] + s_pbc[3 * i + 2];
                keep = cell_d2(c, q0, q1, q2) <= lim2;
            }
            const unsigned long long mask = __ballot(keep);
            if (mask) {
                int first = 0;
                if (lane == 0) first = atomicAdd(&s_cnt, __popcll(mask));
                first = __shfl(first, 0);
                const int slot = first + __popcll(mask & ((1ull << lane) - 1ull));
                if (keep && slot < XB_VORONOI_CAND_MAX) {
                    s_cand[slot].q[0] = q0; s_cand[slot].q[1] = q1; s_cand[slot].q[2] = q2;
                    s_cand[slot].a = a;
                }
            }
        }
        __syncthreads();
        cnt = s_cnt;
        if (tid == 0) {
            if ((unsigned int)cnt > *(volatile unsigned int *)&stats[1]) atomicMax(&stats[1], (unsigned int)cnt);
            if (cnt > XB_VORONOI_CAND_MAX) atomicAdd(&stats[0], 1u);
        }
    }
    const bool full = forced || cnt > XB_VORONOI_CAND_MAX;
    // phase 2: this thread's two voxels (indices clamped into the grid; a voxel outside it is not stored)
    CellVox V;
    cell_two_voxels<VO_TILE>(G, x0, y0, z0, V);
    double besta = __builtin_huge_val(), bestb = __builtin_huge_val();
    int whoa = XB_INT_MAX, whob = XB_INT_MAX;
    if (!full) {
#pragma unroll 2
        for (int k = 0; k < cnt; k++) {
            const double q0 = s_cand[k].q[0], q1 = s_cand[k].q[1], q2 = s_cand[k].q[2];
            const int a = s_cand[k].a;
            vo_take(cell_d2(V.pa, q0, q1, q2), a, besta, whoa);
            vo_take(cell_d2(V.pb, q0, q1, q2), a, bestb, whob);
        }
    } else {
        for (int a = 0; a < G.n; a++) {
            const double *at = G.atoms + 3 * (size_t)a;
            const double a0 = at[0], a1 = at[1], a2 = at[2];
#pragma unroll 1
            for (int i = 0; i < 27; i++) {
                const double q0 = a0 + s_pbc[3 * i], q1 = a1 + s_pbc[3 * i + 1], q2 = a2 + s_pbc[3 * i + 2];
                vo_take(cell_d2(V.pa, q0, q1, q2), a, besta, whoa);
                vo_take(cell_d2(V.pb, q0, q1, q2), a, bestb, whob);
            }
        }
    }
    if (V.oka) {
        if (use_vac && rho[V.va] <= tol) whoa = -1;
        labels[V.va] = whoa;
    }
    if (V.okb) {
        if (use_vac && rho[V.vb] <= tol) whob = -1;
        labels[V.vb] = whob;
    }
}
