// k_weight.h -- device kernels of the weight method (Yu & Trinkle, J. Chem. Phys. 134, 064111): charge and volume per maximum
// with surface voxels split fractionally.  No counterpart in the reference (pybader has the on-grid and near-grid methods only).
//
//   flux          f_ij = alpha_d * max(rho_j - rho_i, 0) for the 26 neighbours j = i + d, S_i = sum_d f_ij, J_ij = f_ij / S_i
//   accumulation  A_i = q_i + sum_d J_ji * A_j over the neighbours j with f_ji > 0 (the adjoint of the paper's weights: the same
//                 basin integrals in O(N) storage); V_i the same with 1 in place of q_i
// Neighbour order everywhere: the C order of the alpha table, indices 0 / 1 / 2 meaning steps 0 / +1 / -1 (as dist_mat).  An
// offset with alpha_d == 0 is skipped (an orthogonal cell keeps its six faces); a vacuum voxel (label -1) is absent: it gets
// S = -1, is never listed, sends and receives nothing.  Every A_i is written once, by one thread, from finished inputs in that
// fixed order -- with -ffp-contract=off the result is a pure function of the inputs.
//
//   k_w_flux    pass 1: tile-staged 26-point stencil over rho -> S, pending (flux-carrying lower neighbours, one byte), the
//               first frontier (pending == 0)
//   k_w_level   pass 2, one level from a work list: A and V by pull, pending of the higher neighbours decremented with an integer
//               atomic on the byte's 32-bit word, a neighbour that reaches zero appended to the next list
//   k_w_tail    the same, level after level inside ONE workgroup while the frontier stays small
//   k_w_maxima / k_w_gather   the maxima (S == 0) and their A, V
// The level loop's state lives on the device (WS_*): a kernel reads the current list and its length there, and the last workgroup
// of a launch -- found by a ticket that every workgroup takes, the idle ones included -- swaps the lists.  The host queues batches
// of launches and waits once per batch.
#pragma once

struct WAlpha { double a[27]; };

enum { WS_CUR = 0, WS_N0 = 1, WS_N1 = 2, WS_TICKET = 3, WS_LEVELS = 4, WS_BATCHED = 5, WS_TAIL = 6, WS_DONE = 7, WS_TOTAL = 8,
       WS_NMAX = 9, WS_PEAK = 10, WS_COUNT = 16 };

#define WT_X 4
#define WT_Y 4
#define WT_Z 16
#define W_TAIL_THREADS 1024
static_assert(WT_X * WT_Y * WT_Z == TPB, "one voxel of the tile per thread");

// step of table index 0 / 1 / 2
__device__ __forceinline__ int w_step(int i) { return i == 2 ? -1 : i; }

__global__ __launch_bounds__(TPB) void k_w_flux(int nx, int ny, int nz, WAlpha al, const double *__restrict__ rho,
                                               const int *__restrict__ labels /* null: no vacuum */, double *__restrict__ S,
                                               unsigned char *__restrict__ pending, int *__restrict__ list, int *ws) {
    __shared__ double s_rho[WT_X + 2][WT_Y + 2][WT_Z + 2];
    __shared__ unsigned char s_vac[WT_X + 2][WT_Y + 2][WT_Z + 2];
    __shared__ int s_base;
    const int tiles_z = (nz + WT_Z - 1) / WT_Z, tiles_y = (ny + WT_Y - 1) / WT_Y;
    const int bz = blockIdx.x % tiles_z, by = (blockIdx.x / tiles_z) % tiles_y, bx = blockIdx.x / (tiles_z * tiles_y);
    const int x0 = bx * WT_X, y0 = by * WT_Y, z0 = bz * WT_Z;
    const int tid = threadIdx.x;
    // the tile and its one-voxel halo, z fastest; every coordinate wraps (an axis of one or two voxels meets itself)
    for (int e = tid; e < (WT_X + 2) * (WT_Y + 2) * (WT_Z + 2); e += TPB) {
        const int hz = e % (WT_Z + 2), hy = (e / (WT_Z + 2)) % (WT_Y + 2), hx = e / ((WT_Z + 2) * (WT_Y + 2));
        const int x = ((x0 - 1 + hx) % nx + nx) % nx, y = ((y0 - 1 + hy) % ny + ny) % ny, z = ((z0 - 1 + hz) % nz + nz) % nz;
        const long long v = ((long long)x * ny + y) * nz + z;
        s_rho[hx][hy][hz] = rho[v];
        s_vac[hx][hy][hz] = labels ? (unsigned char)(labels[v] == -1) : (unsigned char)0;
    }
    __syncthreads();
    const int tz = tid % WT_Z, ty = (tid / WT_Z) % WT_Y, tx = tid / (WT_Z * WT_Y);
    const int x = x0 + tx, y = y0 + ty, z = z0 + tz;
    const bool inside = x < nx && y < ny && z < nz;
    const bool vac = s_vac[tx + 1][ty + 1][tz + 1] != 0;
    const double ri = s_rho[tx + 1][ty + 1][tz + 1];
    double s = 0.;
    int pend = 0;
#pragma unroll
    for (int n = 1; n < 27; n++) {
        const double a = al.a[n];
        if (a == 0.) continue;
        const int dx = w_step(n / 9), dy = w_step((n / 3) % 3), dz = w_step(n % 3);
        if (s_vac[tx + 1 + dx][ty + 1 + dy][tz + 1 + dz]) continue;
        const double rj = s_rho[tx + 1 + dx][ty + 1 + dy][tz + 1 + dz];
        const double up = rj - ri, down = ri - rj;
        s = s + a * (up > 0. ? up : 0.);
        if (a * (down > 0. ? down : 0.) > 0.) pend++;
    }
    const bool live = inside && !vac;
    if (inside) {
        const long long v = ((long long)x * ny + y) * nz + z;
        S[v] = vac ? -1. : s;
        pending[v] = (unsigned char)(vac ? 255 : pend);
    }
    const int n_live = __syncthreads_count(live);
    const int mine = live && pend == 0;
    int total;
    const int off = block_scan_excl(mine, total);
    if (tid == 0) {
        if (n_live) atomicAdd(&ws[WS_TOTAL], n_live);
        s_base = total ? atomicAdd(&ws[WS_N0], total) : 0;
    }
    __syncthreads();
    if (mine) list[s_base + off] = (int)(((long long)x * ny + y) * nz + z);
}

// the voxel at offset n (table index) of (x, y, z)
__device__ __forceinline__ int w_neighbour(int n, int x, int y, int z, int nx, int ny, int nz) {
    const int dx = w_step(n / 9), dy = w_step((n / 3) % 3), dz = w_step(n % 3);
    int X = x + dx, Y = y + dy, Z = z + dz;
    X = X < 0 ? nx - 1 : (X >= nx ? 0 : X);
    Y = Y < 0 ? ny - 1 : (Y >= ny ? 0 : Y);
    Z = Z < 0 ? nz - 1 : (Z >= nz ? 0 : Z);
    return (X * ny + Y) * nz + Z;
}

// One listed voxel: A and V by pull from its finished lower neighbours, then one decrement per flux-carrying higher neighbour.
// Returns the mask of offsets whose neighbour this decrement made ready (bit n).  The decrement of a byte goes through its
// 32-bit word: a byte is decremented exactly as often as pass 1 counted, so it never borrows from the byte above.
__device__ __forceinline__ unsigned w_visit(int v, int nx, int ny, int nz, const WAlpha &al, const double *__restrict__ rho,
                                            const double *__restrict__ S, double *A, double *V, unsigned char *pending) {
    const int x = v / (ny * nz), r = v - x * (ny * nz), y = r / nz, z = r - y * nz;
    const double ri = rho[v];
    double acc = A[v], vol = 1.;
    unsigned up = 0;
#pragma unroll
    for (int n = 1; n < 27; n++) {
        const double a = al.a[n];
        if (a == 0.) continue;
        const int j = w_neighbour(n, x, y, z, nx, ny, nz);
        const double rj = rho[j];
        const double down = ri - rj, rise = rj - ri;
        const double f = a * (down > 0. ? down : 0.);
        if (f > 0.) {
            const double sj = S[j];
            if (sj > 0.) {             // (-1: vacuum)
                const double J = f / sj;
                acc = acc + J * A[j];
                vol = vol + J * V[j];
            }
        } else if (a * (rise > 0. ? rise : 0.) > 0.) up |= 1u << n;
    }
    A[v] = acc;
    V[v] = vol;
    unsigned ready = 0;
    while (up) {
        const int n = __ffs(up) - 1;
        up &= up - 1;
        const int j = w_neighbour(n, x, y, z, nx, ny, nz);
        if (S[j] < 0.) continue;       // vacuum receives nothing
        const unsigned sh = (unsigned)(j & 3) * 8u;
        const unsigned old = atomicSub(reinterpret_cast<unsigned *>(pending) + (j >> 2), 1u << sh);
        if (((old >> sh) & 0xFFu) == 1u) ready |= 1u << n;
    }
    return ready;
}

__device__ __forceinline__ int w_ready_voxel(unsigned &ready, int v, int nx, int ny, int nz) {
    const int n = __ffs(ready) - 1;
    ready &= ready - 1;
    const int x = v / (ny * nz), r = v - x * (ny * nz), y = r / nz, z = r - y * nz;
    return w_neighbour(n, x, y, z, nx, ny, nz);
}

// One level.  EVERY workgroup of the launch reads the state first and takes a ticket last -- also the ones the list leaves nothing
// for, which may be dispatched long after the working ones are done -- and the holder of the last ticket swaps the lists: the
// state cannot change under a workgroup that has yet to read it (as k_brick_grow_dev counts its whole grid, k_fused.h).  A launch
// on an empty list changes nothing.
__global__ __launch_bounds__(TPB) void k_w_level(int nx, int ny, int nz, WAlpha al, const double *__restrict__ rho,
                                                const double *__restrict__ S, double *A, double *V, unsigned char *pending,
                                                int *list0, int *list1, int *ws) {
    __shared__ int s_base;
    const int cur = ws[WS_CUR], n = ws[WS_N0 + cur];
    const int *in = cur ? list1 : list0;
    int *out = cur ? list0 : list1, *out_n = &ws[WS_N0 + (cur ^ 1)];
    for (int base = blockIdx.x * TPB; base < n; base += gridDim.x * TPB) {
        const int k = base + (int)threadIdx.x;
        const int v = k < n ? in[k] : -1;
        unsigned ready = v >= 0 ? w_visit(v, nx, ny, nz, al, rho, S, A, V, pending) : 0u;
        int total;
        const int off = block_scan_excl(__popc(ready), total);
        if (total) {                   // (uniform)
            if (threadIdx.x == 0) s_base = atomicAdd(out_n, total);
            __syncthreads();
            int at = s_base + off;
            while (ready) out[at++] = w_ready_voxel(ready, v, nx, ny, nz);
            __syncthreads();
        }
    }
    __syncthreads();                   // every wave of the workgroup has read the state (and is done) before its ticket is taken
    if (threadIdx.x == 0) {
        __threadfence();
        if (atomicAdd(&ws[WS_TICKET], 1) == (int)gridDim.x - 1) {
            __threadfence();
            ws[WS_TICKET] = 0;
            if (n == 0) return;            // nothing was listed: the state stays as it is
            ws[WS_N0 + cur] = 0;
            ws[WS_CUR] = cur ^ 1;
            ws[WS_LEVELS] += 1;
            ws[WS_BATCHED] += 1;
            ws[WS_DONE] += n;
            const int next = atomicAdd(out_n, 0);
            if (next > ws[WS_PEAK]) ws[WS_PEAK] = next;
        }
    }
}

// The tail: one workgroup runs level after level while the frontier holds at most `cross` voxels -- a barrier of the workgroup
// orders the levels instead of a kernel boundary (its own stores and atomics are visible to it behind __syncthreads()).  It ends
// on an empty frontier (done, or nothing left to do here) or on one above `cross` (the batched levels take over again).
__global__ __launch_bounds__(W_TAIL_THREADS) void k_w_tail(int nx, int ny, int nz, WAlpha al, const double *__restrict__ rho,
                                                         const double *__restrict__ S, double *A, double *V,
                                                         unsigned char *pending, int *list0, int *list1, int *ws, int cross) {
    __shared__ int s_next;
    int cur = ws[WS_CUR], n = ws[WS_N0 + cur], levels = 0, done = 0;
    while (n > 0 && n <= cross) {
        if (threadIdx.x == 0) s_next = 0;
        __syncthreads();
        const int *in = cur ? list1 : list0;
        int *out = cur ? list0 : list1;
        for (int k = threadIdx.x; k < n; k += W_TAIL_THREADS) {
            const int v = in[k];
            unsigned ready = w_visit(v, nx, ny, nz, al, rho, S, A, V, pending);
            while (ready) out[atomicAdd(&s_next, 1)] = w_ready_voxel(ready, v, nx, ny, nz);
        }
        __syncthreads();
        done += n;
        levels++;
        n = s_next;
        cur ^= 1;
        __syncthreads();
    }
    if (threadIdx.x == 0 && levels) {
        ws[WS_CUR] = cur;
        ws[WS_N0 + cur] = n;
        ws[WS_N0 + (cur ^ 1)] = 0;
        ws[WS_LEVELS] += levels;
        ws[WS_TAIL] += levels;
        ws[WS_DONE] += done;
    }
}

// the maxima (S == 0: a non-vacuum voxel with no higher neighbour across a facet), in any order
__global__ __launch_bounds__(TPB) void k_w_maxima(const double *__restrict__ S, long long N, int *__restrict__ list, int *ws) {
    __shared__ int s_base;
    for (long long base = (long long)blockIdx.x * TPB; base < N; base += (long long)gridDim.x * TPB) {
        const long long v = base + threadIdx.x;
        const int mine = v < N && S[v] == 0.;
        int total;
        const int off = block_scan_excl(mine, total);
        if (total) {
            if (threadIdx.x == 0) s_base = atomicAdd(&ws[WS_NMAX], total);
            __syncthreads();
            if (mine) list[s_base + off] = (int)v;
            __syncthreads();
        }
    }
}

__global__ __launch_bounds__(TPB) void k_w_gather(const int *__restrict__ list, int n, const double *__restrict__ A,
                                                 const double *__restrict__ V, double *__restrict__ out) {
    const int k = blockIdx.x * TPB + threadIdx.x;
    if (k >= n) return;
    out[k] = A[list[k]];
    out[n + k] = V[list[k]];
}
