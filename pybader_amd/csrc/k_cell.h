// k_cell.h -- device side of the geometry the atom-centred analyses share (k_moments.h, k_voronoi.h, k_hirshfeld.h, k_isa.h, k_mbis.h; the
// host side is host_cell.h): the position of a voxel, the squared distance, the tile of T^3 voxels, its ball and the slack of a
// bound on it, a thread's two voxels.  Every result of those analyses is bit-defined, so each float64 expression they must agree on
// is written here ONCE.  Included by bader_hip.hip (one translation unit); everything but k_ms_tables inlines into its caller.
#pragma once

// tab: the three terms of the voxel position per axis index, pos[j][p] = lat[3 * axis + j] * p / n_axis, laid out
// tab[j * (nx + ny + nz) + offset(axis) + p]
__global__ __launch_bounds__(TPB) void k_ms_tables(int nx, int ny, int nz, const double *__restrict__ lat, double *__restrict__ tab) {
    const int len = nx + ny + nz, t = blockIdx.x * TPB + threadIdx.x;
    if (t >= 3 * len) return;
    const int j = t / len, q = t - j * len;
    const int axis = q < nx ? 0 : (q < nx + ny ? 1 : 2);
    const int p = axis == 0 ? q : (axis == 1 ? q - nx : q - nx - ny);
    const int n = axis == 0 ? nx : (axis == 1 ? ny : nz);
    tab[t] = lat[3 * axis + j] * (double)p / (double)n;
}

// what the tile kernels know of the cell and the grid (VoGeom and HsGeom begin with it; host_cell.h fills it)
struct CellGeom {
    const double *tab;      // the position table of k_ms_tables
    double lat[9];
    double len;             // L = |a| + |b| + |c|
    int nx, ny, nz;
    int ntx, nty, ntz;      // tiles per axis
};

// a thread's two voxels of a tile (cell_two_voxels)
struct CellVox {
    double pa[3], pb[3];    // their positions (of the indices clamped into the grid)
    size_t va, vb;          // their linear indices (clamped likewise)
    bool oka, okb;          // the grid holds them
};

// the position of voxel (p0, p1, p2): the three terms of the table, added in this order
__device__ __forceinline__ void cell_pos(const double *tab, int nx, int ny, int nz, int p0, int p1, int p2, double pc[3]) {
    const int len = nx + ny + nz;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double *tj = tab + (size_t)j * len;
        pc[j] = tj[p0];
        pc[j] += tj[nx + p1];
        pc[j] += tj[nx + ny + p2];
    }
}

__device__ __forceinline__ double cell_d2(const double pc[3], double q0, double q1, double q2) {
    const double e0 = pc[0] - q0, e1 = pc[1] - q1, e2 = pc[2] - q2;
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// tile number `tile` (C order over the tiles) -> its first voxel
template <int T>
__device__ __forceinline__ void cell_tile_origin(const CellGeom &G, int tile, int &x0, int &y0, int &z0) {
    const int tz = tile % G.ntz; tile /= G.ntz;
    const int ty = tile % G.nty;
    const int tx = tile / G.nty;
    x0 = tx * T; y0 = ty * T; z0 = tz * T;
}

// the ball around the voxels of the tile at (x0, y0, z0), of the extent the grid leaves of it: c = their centre; -> the square of
// the longest body diagonal of the box they span, (2 R)^2 (both from the voxel lattice)
template <int T>
__device__ __forceinline__ double cell_tile_ball(const CellGeom &G, int x0, int y0, int z0, double c[3]) {
    const double ex = (double)(min(T, G.nx - x0) - 1), ey = (double)(min(T, G.ny - y0) - 1), ez = (double)(min(T, G.nz - z0) - 1);
    const double fx = (double)x0 + 0.5 * ex, fy = (double)y0 + 0.5 * ey, fz = (double)z0 + 0.5 * ez;
    double diag2 = 0.;
    double u[3][3];
#pragma unroll
    for (int j = 0; j < 3; j++) {
        c[j] = G.lat[j] * fx / (double)G.nx;
        c[j] += G.lat[3 + j] * fy / (double)G.ny;
        c[j] += G.lat[6 + j] * fz / (double)G.nz;
        u[0][j] = G.lat[j] * ex / (double)G.nx;
        u[1][j] = G.lat[3 + j] * ey / (double)G.ny;
        u[2][j] = G.lat[6 + j] * ez / (double)G.nz;
    }
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const double s1 = (s & 1) ? -1. : 1., s2 = (s & 2) ? -1. : 1.;
        double d2 = 0.;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double d = (u[0][j] + s1 * u[1][j]) + s2 * u[2][j];
            d2 += d * d;
        }
        diag2 = fmax(diag2, d2);
    }
    return diag2;
}

// SLACK.  A tile kernel keeps the images q(i) = atom + shift with  d_c(i) <= lim,  d_c the distance from c, where lim is a bound on
// the distance from a VOXEL of the tile plus R or 2 R: |d(v, i) - d_c(i)| <= R for a voxel v of the tile.  The test is made on
// computed numbers, so lim gets a slack.  Read the computed float64 triples -- pc(v) of a voxel, c, q(i) -- as exact points and write
// D for exact distances between them, u = 2^-53, L = |a| + |b| + |c| of the cell.
//   (a) pc(v) and c are sums of three terms lat * p / n, each rounded twice, added with two roundings: every component lies within
//       4 u L of the exact position, so  max_v D(pc(v), c) <= R_exact + 14 u L,  and the computed R >= R_exact (1 - 8 u).
//   (b) the computed d2 = (e0 e0 + e1 e1) + e2 e2 with e = pc - q carries at most (1 + u)^5 on D^2: its root lies within 3 u D of D.
//       The computed d_c^2 likewise; a computed root adds one u.
//   (c) an image that must be kept satisfies, on computed numbers, a comparison at some voxel v (k_voronoi.h and k_hirshfeld.h say
//       which); with (b), the triangle inequality and (a) that gives  D(c, i) <= lim + (7 u + ...) lim + 28 u L.
//   (d) squaring the threshold and the sums that form it add a few u more.
// All of it is below 64 u (lim + L).  cell_slack2 adds 2^-40 (lim + L) = 8192 u (...) before squaring and 2^-40 of the square
// after: more than a hundred times the need, and about 1e-12 of the radius.
// -> the square d_c^2 is compared with
__device__ __forceinline__ double cell_slack2(double lim, double len) {
    lim += 0x1p-40 * (lim + len);
    double lim2 = lim * lim;
    lim2 += 0x1p-40 * lim2;
    return lim2;
}

// the two voxels of this thread in the tile at (x0, y0, z0) of a workgroup of four waves: wave w takes the x-planes w and w + T / 2,
// a lane the voxel (y, z) = (lane / T, lane % T) of either.  The indices are clamped into the grid: a voxel outside it has the
// position and the index of one inside and is told by its flag.
template <int T>
__device__ __forceinline__ void cell_two_voxels(const CellGeom &G, int x0, int y0, int z0, CellVox &V) {
    static_assert(T * T == XB_WAVE, "a wave is one x-plane of the tile");
    const int lane = threadIdx.x % XB_WAVE, wave = threadIdx.x / XB_WAVE;
    const int py = y0 + lane / T, pz = z0 + lane % T;
    const int pxa = x0 + wave, pxb = x0 + wave + T / 2;
    const int cy = min(py, G.ny - 1), cz = min(pz, G.nz - 1), cxa = min(pxa, G.nx - 1), cxb = min(pxb, G.nx - 1);
    cell_pos(G.tab, G.nx, G.ny, G.nz, cxa, cy, cz, V.pa);
    cell_pos(G.tab, G.nx, G.ny, G.nz, cxb, cy, cz, V.pb);
    V.oka = py < G.ny && pz < G.nz && pxa < G.nx;
    V.okb = py < G.ny && pz < G.nz && pxb < G.nx;
    const size_t row = (size_t)cy * G.nz + cz, plane = (size_t)G.ny * G.nz;
    V.va = (size_t)cxa * plane + row; V.vb = (size_t)cxb * plane + row;
}
