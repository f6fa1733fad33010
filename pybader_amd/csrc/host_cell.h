// host_cell.h -- host side of the geometry the atom-centred analyses share (k_cell.h): the image vectors, the cell's length, the
// tiles per axis, the finite checks, the block head with the position table, the statistics of a tile kernel's two routes.
// Used by host_moments.h, host_voronoi.h, host_hirshfeld.h, host_isa.h and host_mbis.h.  The first part is plain C++ (<cmath>, <cstdint>) and
// compiles alone (tests/test_cell_cpu.py); the second needs the library's translation unit.
#pragma once
#include <cmath>
#include <cstdint>

// component j of the lattice shift (x, y, z), exactly as the definitions write it (IEEE, no contraction)
static inline double cell_shift(const double *lattice, int x, int y, int z, int j) {
    return (lattice[j] * (double)x + lattice[3 + j] * (double)y) + lattice[6 + j] * (double)z;
}
// the 27 image vectors, image i = (x + 1) * 9 + (y + 1) * 3 + (z + 1)
static inline void cell_images27(const double *lattice, double out[27][3]) {
    for (int x = -1; x < 2; x++)
        for (int y = -1; y < 2; y++)
            for (int z = -1; z < 2; z++)
                for (int j = 0; j < 3; j++) out[(x + 1) * 9 + (y + 1) * 3 + (z + 1)][j] = cell_shift(lattice, x, y, z, j);
}
// L = |a| + |b| + |c|
static inline double cell_len(const double *lattice) {
    double len = 0.;
    for (int k = 0; k < 3; k++)
        len += std::sqrt((lattice[3 * k] * lattice[3 * k] + lattice[3 * k + 1] * lattice[3 * k + 1]) + lattice[3 * k + 2] * lattice[3 * k + 2]);
    return len;
}
// tiles of edge T along an axis of n voxels
static inline int cell_tiles(int n, int T) { return (n + T - 1) / T; }

#ifdef __HIPCC__
// The head of a block (host_moments.h, host_voronoi.h), in doubles: [0, 96) the 27 image vectors (81 used), [96, 112) the lattice
// (9 used); the position table of k_ms_tables, 3 * (nx + ny + nz), follows it.
#define CELL_HEAD 112

static int cell_check(const char *who, const double *lattice, const double *atoms, int64_t n) {
    for (int k = 0; k < 9; k++)
        if (!std::isfinite(lattice[k])) return fail(XB_E_ARG, "%s: the lattice is not finite", who);
    for (int64_t k = 0; k < 3 * n; k++)
        if (!std::isfinite(atoms[k])) return fail(XB_E_ARG, "%s: atom %lld is not finite", who, (long long)(k / 3));
    return XB_OK;
}

static void cell_geom(CellGeom &G, const Grid &g, const double *lattice, int T, const double *tab) {
    G.tab = tab;
    for (int k = 0; k < 9; k++) G.lat[k] = lattice[k];
    G.len = cell_len(lattice);
    G.nx = g.nx; G.ny = g.ny; G.nz = g.nz;
    G.ntx = cell_tiles(g.nx, T); G.nty = cell_tiles(g.ny, T); G.ntz = cell_tiles(g.nz, T);
}

// the position table of the grid from the lattice at lat_dev, on the context's stream
static void cell_tables(xb_ctx *c, const double *lat_dev, double *tab) {
    const Grid &g = c->g;
    k_ms_tables<<<nblocks(3 * ((long long)g.nx + g.ny + g.nz)), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, lat_dev, tab);
}

// the head is formed in `head` (the caller's: it lives until the stream is waited for) and copied to buf; cell_tables(c, buf + 96,
// buf + CELL_HEAD) then makes the table (its own call: xb_moment_sum times its kernels, not this copy)
static int cell_head(xb_ctx *c, const double *lattice, double head[CELL_HEAD], double *buf) {
    for (int k = 0; k < CELL_HEAD; k++) head[k] = 0.;
    cell_images27(lattice, reinterpret_cast<double(*)[3]>(head));
    for (int k = 0; k < 9; k++) head[96 + k] = lattice[k];
    HIPCHK(hipMemcpyAsync(buf, head, CELL_HEAD * sizeof(double), hipMemcpyHostToDevice, c->stream));
    return XB_OK;
}

// stats[0..2] of a tile kernel: tiles answered from the list, by the full search, the largest candidate count; st: the kernel's
// two words (untouched when `forced`)
static void tile_route_stats(int64_t *stats, long long tiles, int forced, const unsigned int st[2]) {
    if (!stats) return;
    const long long full = forced ? tiles : (long long)st[0];
    stats[0] = tiles - full;
    stats[1] = full;
    stats[2] = st[1];
}
#endif
