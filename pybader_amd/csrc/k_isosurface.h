// k_isosurface.h -- device kernels of libbader_hip.so: isosurfaces by marching tetrahedra on the Freudenthal triangulation of the
// periodic voxel lattice (xb_isosurface, host_isosurface.h; the definition is in include/bader_hip.h and DESIGN.md section 21).
// Included by bader_hip.hip (one translation unit) behind k_critical.h and k_stencil.h, whose tile, wrap and label sums it uses.
#pragma once

// Everything about a cube -- the crossing edges its voxel owns, its triangles, their corners, its inside volume -- is a function
// of the field at the cube's eight corners, so both routes run ONE routine per voxel over a reader of those eight values:
//   tile     a workgroup stages the CP_TX x CP_TY x CP_TZ tile and its +1 halo on the three positive sides in LDS (9 x 9 x 33
//            doubles, 21 384 B), wraps resolved at staging time; a thread owns the column (ty, tz) and walks its CP_TX voxels
//   gather   (XB_ISO_GATHER) one thread per voxel reads the eight values from global memory: the second implementation
// Vertex ids and triangle slots are ranks in C order of the voxels, so the passes are
//   count    per voxel a 32-bit word: the 7 crossing bits of the edges it owns and the number of its cube's triangles
//   offsets  per run of ISO_BLOCK consecutive voxels an exclusive scan (wave shuffles, one LDS step): the word becomes
//            crossing bits | vertex offset in the run << 7 | triangle offset in the run << 18; the run's two totals go out
//   scan     the runs' totals: sums per ISO_CHUNK runs, their exclusive scan by one workgroup, the scan inside every chunk --
//            three launches, no workgroup ever waits for another
//   emit     vertices, colour, triangles, wrap, cell at their ranks; area, volume, per-label volumes; its own counts
// A wave whose cubes all lie outside leaves either pass after one ballot.
#define ISO_BLOCK TPB
#define ISO_CHUNK 2048            // runs per chunk of the scan: ISO_CHUNK / TPB per thread
#define ISO_VOFF_SHIFT 7
#define ISO_TOFF_SHIFT 18
#define ISO_SLOTS 64               // addresses the workgroups' sums are spread over
static_assert(7 * (ISO_BLOCK - 1) < (1 << (ISO_TOFF_SHIFT - ISO_VOFF_SHIFT)) && 12 * (ISO_BLOCK - 1) < (1 << (32 - ISO_TOFF_SHIFT)),
              "the offsets inside a run fit their bits");
static_assert(ISO_CHUNK % TPB == 0, "whole threads");

// ---- the table ---------------------------------------------------------------------------------------------------------------------
// e[tau][m]: byte 0 the number of triangles of tetrahedron tau with the inside corners m (bit i: corner P_i of the path), bytes
// 1 .. 6 their corners as edge codes (owner corner of the cube << 3 | k: the cube corner 4 cx + 2 cy + cz that owns the edge
// and its offset index), 255 where unused; loc: the same corners as pair indices 01 02 03 12 13 23 inside the tetrahedron.
struct IsoTable {
    unsigned char e[6][16][8];
    unsigned char loc[6][16][8];
};
constexpr __host__ __device__ int iso_perm(int tau, int j) {
    return tau == 0 ? (j == 0 ? 0 : (j == 1 ? 1 : 2)) : tau == 1 ? (j == 0 ? 0 : (j == 1 ? 2 : 1)) : tau == 2 ? (j == 0 ? 1 : (j == 1 ? 0 : 2))
         : tau == 3 ? (j == 0 ? 1 : (j == 1 ? 2 : 0)) : tau == 4 ? (j == 0 ? 2 : (j == 1 ? 0 : 1)) : (j == 0 ? 2 : (j == 1 ? 1 : 0));
}
// corner P_i of tetrahedron tau as cube corner bits 4 x + 2 y + z: the path 0 -> e_a -> e_a + e_b -> (1, 1, 1)
constexpr __host__ __device__ int iso_corner(int tau, int i) {
    int c = 0;
    for (int j = 0; j < i; j++) c |= 4 >> iso_perm(tau, j);
    return c;
}
constexpr __host__ __device__ int iso_pair(int lo, int hi) { return lo == 0 ? hi - 1 : (lo == 1 ? hi + 1 : 5); }
constexpr IsoTable iso_make_table() {
    IsoTable T{};
    for (int tau = 0; tau < 6; tau++)
        for (int m = 0; m < 16; m++) {
            for (int b = 0; b < 8; b++) { T.e[tau][m][b] = 255; T.loc[tau][m][b] = 255; }
            T.e[tau][m][0] = 0; T.loc[tau][m][0] = 0;
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int i = 0; i < 4; i++) {
                if ((m >> i) & 1) in[ni++] = i;
                else out[no++] = i;
            }
            if (ni == 0 || ni == 4) continue;
            int tri[2][3][2] = {}, nt = 0;
            if (ni == 1 || ni == 3) {
                const int apex = ni == 1 ? in[0] : out[0];
                int q = 0;
                for (int j = 0; j < 4; j++)
                    if (j != apex) { tri[0][q][0] = j < apex ? j : apex; tri[0][q][1] = j < apex ? apex : j; q++; }
                nt = 1;
            } else {   // the quadrilateral ik il jl jk, split along ik -- jl
                const int i = in[0], j = in[1], k = out[0], l = out[1];
                const int ik[2] = {i < k ? i : k, i < k ? k : i}, il[2] = {i < l ? i : l, i < l ? l : i};
                const int jl[2] = {j < l ? j : l, j < l ? l : j}, jk[2] = {j < k ? j : k, j < k ? k : j};
                tri[0][0][0] = ik[0]; tri[0][0][1] = ik[1]; tri[0][1][0] = il[0]; tri[0][1][1] = il[1]; tri[0][2][0] = jl[0]; tri[0][2][1] = jl[1];
                tri[1][0][0] = ik[0]; tri[1][0][1] = ik[1]; tri[1][1][0] = jl[0]; tri[1][1][1] = jl[1]; tri[1][2][0] = jk[0]; tri[1][2][1] = jk[1];
                nt = 2;
            }
            // outward: with every crossing at its edge's midpoint, (q1 - q0) x (q2 - q0) . (mean outside - mean inside) > 0
            int dir[3] = {0, 0, 0};
            for (int a = 0; a < 3; a++) {
                for (int s = 0; s < no; s++) dir[a] += ni * ((iso_corner(tau, out[s]) >> (2 - a)) & 1);
                for (int s = 0; s < ni; s++) dir[a] -= no * ((iso_corner(tau, in[s]) >> (2 - a)) & 1);
            }
            for (int t = 0; t < nt; t++) {
                int q[3][3] = {};
                for (int v = 0; v < 3; v++)
                    for (int a = 0; a < 3; a++)
                        q[v][a] = ((iso_corner(tau, tri[t][v][0]) >> (2 - a)) & 1) + ((iso_corner(tau, tri[t][v][1]) >> (2 - a)) & 1);
                int e1[3] = {}, e2[3] = {};
                for (int a = 0; a < 3; a++) { e1[a] = q[1][a] - q[0][a]; e2[a] = q[2][a] - q[0][a]; }
                const int dot = (e1[1] * e2[2] - e1[2] * e2[1]) * dir[0] + (e1[2] * e2[0] - e1[0] * e2[2]) * dir[1] +
                                (e1[0] * e2[1] - e1[1] * e2[0]) * dir[2];
                if (dot < 0)
                    for (int s = 0; s < 2; s++) { const int x = tri[t][1][s]; tri[t][1][s] = tri[t][2][s]; tri[t][2][s] = x; }
                for (int v = 0; v < 3; v++) {
                    const int lo = iso_corner(tau, tri[t][v][0]), hi = iso_corner(tau, tri[t][v][1]);
                    T.e[tau][m][1 + 3 * t + v] = (unsigned char)((lo << 3) | ((hi ^ lo) - 1));
                    T.loc[tau][m][1 + 3 * t + v] = (unsigned char)iso_pair(tri[t][v][0], tri[t][v][1]);
                }
            }
            T.e[tau][m][0] = (unsigned char)nt; T.loc[tau][m][0] = (unsigned char)nt;
        }
    return T;
}
static constexpr IsoTable iso_tab_h = iso_make_table();
__device__ __constant__ const IsoTable iso_tab_d = iso_make_table();
static_assert(XB_ISO_TABLE_SIZE == sizeof(iso_tab_h.e), "6 tetrahedra, 16 masks, 8 bytes");
static_assert(iso_corner(0, 1) == 4 && iso_corner(0, 2) == 6 && iso_corner(5, 1) == 1 && iso_corner(5, 2) == 3 && iso_corner(3, 3) == 7,
              "the paths of the definition");

// the inside bits of tetrahedron tau's corners out of the cube's eight (bit c: corner 4 cx + 2 cy + cz)
__host__ __device__ __forceinline__ unsigned iso_tet_mask(unsigned cm, int tau) {
    return (cm & 1u) | (((cm >> iso_corner(tau, 1)) & 1u) << 1) | (((cm >> iso_corner(tau, 2)) & 1u) << 2) | (((cm >> 7) & 1u) << 3);
}
// triangles of a cube: one per tetrahedron with 1 or 3 inside corners, two with 2
__device__ __forceinline__ unsigned iso_cube_triangles(unsigned cm) {
    unsigned nt = 0;
#pragma unroll
    for (int tau = 0; tau < 6; tau++) {
        const unsigned p = (unsigned)__popc(iso_tet_mask(cm, tau));
        nt += p == 2u ? 2u : ((p == 1u || p == 3u) ? 1u : 0u);
    }
    return nt;
}
// bit k: the edge (v, k) crosses -- the voxel and its neighbour at offset k + 1 (as corner bits) differ
__device__ __forceinline__ unsigned iso_cross_bits(unsigned cm) { return ((cm >> 1) ^ (0u - (cm & 1u))) & 0x7fu; }

// ---- readers of the eight corners ----------------------------------------------------------------------------------------------------
typedef double IsoTile[CP_TY + 1][CP_TZ + 1];
struct IsoTileReader {
    const IsoTile *s;
    int tx, ty, tz;
    __device__ __forceinline__ double operator()(int c) const { return s[tx + ((c >> 2) & 1)][ty + ((c >> 1) & 1)][tz + (c & 1)]; }
};
// the wrapped neighbours of a voxel: coordinates and linear indices of the eight corners
struct IsoCorners {
    int xs[2], ys[2], zs[2];
    int ny, nz;
    __device__ __forceinline__ IsoCorners(int x, int y, int z, int nx, int ny_, int nz_) : ny(ny_), nz(nz_) {
        xs[0] = x; xs[1] = x + 1 < nx ? x + 1 : 0;
        ys[0] = y; ys[1] = y + 1 < ny_ ? y + 1 : 0;
        zs[0] = z; zs[1] = z + 1 < nz_ ? z + 1 : 0;
    }
    __device__ __forceinline__ long long lin(int c) const { return ((long long)xs[(c >> 2) & 1] * ny + ys[(c >> 1) & 1]) * nz + zs[c & 1]; }
};
struct IsoGatherReader {
    const double *f;
    const IsoCorners *C;
    __device__ __forceinline__ double operator()(int c) const { return f[C->lin(c)]; }
};
template <class R>
__device__ __forceinline__ unsigned iso_cube_mask(const R &r, double level) {
    unsigned cm = 0;
#pragma unroll
    for (int c = 0; c < 8; c++) cm |= (r(c) >= level ? 1u : 0u) << c;   // (a NaN is outside)
    return cm;
}
// the tile of workgroup blockIdx.x and its +1 halo on the positive sides, z fastest; every coordinate wraps
__device__ __forceinline__ void iso_stage(IsoTile *s, int nx, int ny, int nz, const double *__restrict__ f, int &x0, int &y0, int &z0) {
    const int tiles_z = (nz + CP_TZ - 1) / CP_TZ, tiles_y = (ny + CP_TY - 1) / CP_TY;
    const int bz = blockIdx.x % tiles_z, by = (blockIdx.x / tiles_z) % tiles_y, bx = blockIdx.x / (tiles_z * tiles_y);
    x0 = bx * CP_TX; y0 = by * CP_TY; z0 = bz * CP_TZ;
    for (int e = threadIdx.x; e < (CP_TX + 1) * (CP_TY + 1) * (CP_TZ + 1); e += TPB) {
        const int hz = e % (CP_TZ + 1), hy = (e / (CP_TZ + 1)) % (CP_TY + 1), hx = e / ((CP_TZ + 1) * (CP_TY + 1));
        const int x = cp_wrap(x0 + hx, nx), y = cp_wrap(y0 + hy, ny), z = cp_wrap(z0 + hz, nz);
        s[hx][hy][hz] = f[((long long)x * ny + y) * nz + z];
    }
    __syncthreads();
}

// ---- count --------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_iso_count(int nx, int ny, int nz, const double *__restrict__ f, double level,
                                                  unsigned int *__restrict__ word) {
    __shared__ IsoTile s_f[CP_TX + 1];
    int x0, y0, z0;
    iso_stage(s_f, nx, ny, nz, f, x0, y0, z0);
    const int tz = threadIdx.x % CP_TZ, ty = threadIdx.x / CP_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool col = y < ny && z < nz;
    unsigned cm[CP_TX];
    bool any = false;
#pragma unroll
    for (int tx = 0; tx < CP_TX; tx++) {
        cm[tx] = col && x0 + tx < nx ? iso_cube_mask(IsoTileReader{s_f, tx, ty, tz}, level) : 0u;
        any = any || (cm[tx] != 0u && cm[tx] != 255u);
    }
    const bool busy = __ballot(any) != 0ull;   // (else: a wave of uniform cubes -- every word is zero)
    if (!col) return;
#pragma unroll
    for (int tx = 0; tx < CP_TX; tx++) {
        if (x0 + tx >= nx) break;
        word[((long long)(x0 + tx) * ny + y) * nz + z] = busy ? (iso_cross_bits(cm[tx]) | (iso_cube_triangles(cm[tx]) << 7)) : 0u;
    }
}
__global__ __launch_bounds__(TPB) void k_iso_count_gather(int nx, int ny, int nz, const double *__restrict__ f, double level,
                                                         unsigned int *__restrict__ word) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    if (v >= nx * nyz) return;
    const int x = (int)(v / nyz), q = (int)(v - x * nyz), y = q / nz, z = q - y * nz;
    const IsoCorners C(x, y, z, nx, ny, nz);
    const unsigned cm = iso_cube_mask(IsoGatherReader{f, &C}, level);
    word[v] = iso_cross_bits(cm) | (iso_cube_triangles(cm) << 7);
}

// ---- offsets inside a run, and the scan of the runs' totals -----------------------------------------------------------------------
// word[v]: crossing bits | triangles << 7 on entry.  tot[2 b], tot[2 b + 1]: the vertices and triangles of run b.
__global__ __launch_bounds__(TPB) void k_iso_offsets(long long N, unsigned int *__restrict__ word, unsigned long long *__restrict__ tot) {
    __shared__ unsigned int s_wave[TPB / XB_WAVE];
    const long long v = (long long)blockIdx.x * ISO_BLOCK + threadIdx.x;
    const unsigned int w = v < N ? word[v] : 0u;
    const unsigned int own = (unsigned int)__popc(w & 0x7fu) | (((w >> 7) & 15u) << 16);   // (vertices | triangles << 16: both below 2^16)
    const int lane = threadIdx.x % XB_WAVE, wave = threadIdx.x / XB_WAVE;
    unsigned int inc = own;
#pragma unroll
    for (int o = 1; o < XB_WAVE; o <<= 1) {
        const unsigned int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == XB_WAVE - 1) s_wave[wave] = inc;
    __syncthreads();
    unsigned int before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < TPB / XB_WAVE; k++) {
        if (k < wave) before += s_wave[k];
        all += s_wave[k];
    }
    const unsigned int ex = before + inc - own;
    if (v < N) word[v] = (w & 0x7fu) | ((ex & 0xffffu) << ISO_VOFF_SHIFT) | ((ex >> 16) << ISO_TOFF_SHIFT);
    if (threadIdx.x == 0) {
        tot[2 * (long long)blockIdx.x] = all & 0xffffu;
        tot[2 * (long long)blockIdx.x + 1] = all >> 16;
    }
}
// part[2 b], part[2 b + 1]: the sums over chunk b of the nb pairs of tot
__global__ __launch_bounds__(TPB) void k_iso_scan_sums(const unsigned long long *__restrict__ tot, long long nb, unsigned long long *__restrict__ part) {
    __shared__ unsigned long long s_sum[2][TPB / XB_WAVE];
    const long long first = (long long)blockIdx.x * ISO_CHUNK;
    unsigned long long a = 0, b = 0;
    for (long long i = first + threadIdx.x; i < first + ISO_CHUNK && i < nb; i += TPB) { a += tot[2 * i]; b += tot[2 * i + 1]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if (threadIdx.x % XB_WAVE == 0) { s_sum[0][threadIdx.x / XB_WAVE] = a; s_sum[1][threadIdx.x / XB_WAVE] = b; }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0;
        for (int k = 0; k < TPB / XB_WAVE; k++) s += s_sum[threadIdx.x][k];
        part[2 * (long long)blockIdx.x + threadIdx.x] = s;
    }
}
// one workgroup: the exclusive scan of the np pairs of part in place; grand[0], grand[1]: the totals (np is N / (ISO_BLOCK ISO_CHUNK))
__global__ __launch_bounds__(XB_WAVE) void k_iso_scan_top(unsigned long long *__restrict__ part, long long np, unsigned long long *__restrict__ grand) {
    if (threadIdx.x >= 2) return;
    unsigned long long run = 0;
    for (long long i = 0; i < np; i++) {
        const unsigned long long x = part[2 * i + threadIdx.x];
        part[2 * i + threadIdx.x] = run;
        run += x;
    }
    grand[threadIdx.x] = run;
}
// the exclusive scan of tot inside chunk blockIdx.x, on top of part: tot becomes the runs' bases
__global__ __launch_bounds__(TPB) void k_iso_scan_apply(unsigned long long *__restrict__ tot, long long nb, const unsigned long long *__restrict__ part) {
    __shared__ unsigned long long s_sum[2][TPB / XB_WAVE];
    constexpr int PER = ISO_CHUNK / TPB;
    const long long first = (long long)blockIdx.x * ISO_CHUNK + (long long)threadIdx.x * PER;
    unsigned long long va[PER], vb[PER], a = 0, b = 0;
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const bool in = first + k < nb;
        va[k] = in ? tot[2 * (first + k)] : 0ull;
        vb[k] = in ? tot[2 * (first + k) + 1] : 0ull;
        a += va[k]; b += vb[k];
    }
    const int lane = threadIdx.x % XB_WAVE, wave = threadIdx.x / XB_WAVE;
    unsigned long long ia = a, ib = b;
#pragma unroll
    for (int o = 1; o < XB_WAVE; o <<= 1) {
        const unsigned long long ua = __shfl_up(ia, o), ub = __shfl_up(ib, o);
        if (lane >= o) { ia += ua; ib += ub; }
    }
    if (lane == XB_WAVE - 1) { s_sum[0][wave] = ia; s_sum[1][wave] = ib; }
    __syncthreads();
    unsigned long long ra = part[2 * (long long)blockIdx.x] + ia - a, rb = part[2 * (long long)blockIdx.x + 1] + ib - b;
    for (int k = 0; k < wave; k++) { ra += s_sum[0][k]; rb += s_sum[1][k]; }
#pragma unroll
    for (int k = 0; k < PER; k++) {
        if (first + k < nb) { tot[2 * (first + k)] = ra; tot[2 * (first + k) + 1] = rb; }
        ra += va[k]; rb += vb[k];
    }
}

// ---- emit ---------------------------------------------------------------------------------------------------------------------------
struct IsoGeom {
    double A[9];   // the voxel lattice, A[3 * i + j] = lattice[3 * i + j] / n_i
};
struct IsoOut {
    double *vert;                 // [3 V]
    double *colour;               // [V] or null
    long long *tri;               // [3 T]
    unsigned short *wrap;         // [T]
    long long *cell;              // [T]
    unsigned long long cap_v, cap_t;
    const double *g;              // the colour field or null
};
// what a thread adds up over its voxels
struct IsoSums {
    double area = 0., frac = 0.;
    unsigned long long nv = 0, nt = 0;
};
// the rank of the vertex on edge (corner c of the cube, k): the run's base, the owner's offset in the run, its crossing edges below k
__device__ __forceinline__ unsigned long long iso_vertex_id(const unsigned int *__restrict__ word, const unsigned long long *__restrict__ base,
                                                            long long lin_c, int k) {
    const unsigned int w = word[lin_c];
    return base[2 * (lin_c / ISO_BLOCK)] + ((w >> ISO_VOFF_SHIFT) & 0x7ffu) + (unsigned int)__popc(w & ((1u << k) - 1u));
}
// t of the definition on the edge from corner lo to corner hi of the cube: one division
template <class R>
__device__ __forceinline__ double iso_t(const R &r, double level, int lo, int hi) {
    const double a = r(lo), b = r(hi);
    return (level - a) / (b - a);
}

// One voxel v = (x, y, z) with the inside bits cm of its cube: the vertices on the edges it owns, the triangles of its cube, the
// cube's inside fraction per tetrahedron.  share[c]: what the cube credits to its corner c (in tetrahedra: times |det A| / 6).
template <class R>
__device__ __forceinline__ void iso_voxel(const R &r, unsigned cm, int x, int y, int z, int nx, int ny, int nz, long long lin, const IsoCorners &C,
                                          double level, const IsoGeom &G, const unsigned int *__restrict__ word,
                                          const unsigned long long *__restrict__ base, const IsoOut &O, IsoSums &S, double share[8]) {
    if (cm == 255u) {   // six whole tetrahedra, no vertex, no triangle: a quarter of each to each of its corners
        S.frac += 6.;
        share[0] += 1.5; share[7] += 1.5;
#pragma unroll
        for (int c = 1; c < 7; c++) share[c] += 0.5;
        return;
    }
    const IsoTable &T = iso_tab_d;
    const unsigned int w = word[lin];
    const unsigned long long *mybase = base + 2 * (lin / ISO_BLOCK);
    // the vertices this voxel owns
    const unsigned xm = iso_cross_bits(cm);
    if (xm) {
        unsigned long long id = mybase[0] + ((w >> ISO_VOFF_SHIFT) & 0x7ffu);
        const double p[3] = {(double)x, (double)y, (double)z};
        for (int k = 0; k < 7; k++) {
            if (!((xm >> k) & 1u)) continue;
            const double t = iso_t(r, level, 0, k + 1);
            if (id < O.cap_v) {
#pragma unroll
                for (int j = 0; j < 3; j++) O.vert[3 * id + j] = (((k + 1) >> (2 - j)) & 1) ? p[j] + t : p[j];
                if (O.colour) {
                    const double ga = O.g[lin], gb = O.g[C.lin(k + 1)];
                    O.colour[id] = ga + t * (gb - ga);
                }
                S.nv++;
            }
            id++;
        }
    }
    if (cm == 0u) return;
    unsigned long long ti = mybase[1] + (w >> ISO_TOFF_SHIFT);
    const double n[3] = {(double)nx, (double)ny, (double)nz};
    const int across[3] = {x + 1 >= nx ? 1 : 0, y + 1 >= ny ? 1 : 0, z + 1 >= nz ? 1 : 0};   // a corner at +1 wraps on this axis
    for (int tau = 0; tau < 6; tau++) {
        const unsigned m = iso_tet_mask(cm, tau);
        if (m == 0u) continue;
        const int ni = __popc(m);
        int pc[4];
        for (int i = 0; i < 4; i++) pc[i] = iso_corner(tau, i);
        double frac = 1.;
        if (m != 15u) {
            // t on the crossing edges of the tetrahedron, pairs 01 02 03 12 13 23
            double te[6];
            for (int lo = 0; lo < 3; lo++)
                for (int hi = lo + 1; hi < 4; hi++)
                    te[iso_pair(lo, hi)] = (((m >> lo) ^ (m >> hi)) & 1u) ? iso_t(r, level, pc[lo], pc[hi]) : 0.;
            // the triangles
            const int nt = T.e[tau][m][0];
            for (int t = 0; t < nt; t++) {
                double q[3][3];
                unsigned long long id[3];
                unsigned int wrap = 0;
                for (int v = 0; v < 3; v++) {
                    const int code = T.e[tau][m][1 + 3 * t + v], c = code >> 3, k = code & 7;
                    const double tv = te[T.loc[tau][m][1 + 3 * t + v]];
                    id[v] = iso_vertex_id(word, base, C.lin(c), k);
                    const int own[3] = {C.xs[(c >> 2) & 1], C.ys[(c >> 1) & 1], C.zs[c & 1]};
                    for (int j = 0; j < 3; j++) {
                        const double pj = (((k + 1) >> (2 - j)) & 1) ? (double)own[j] + tv : (double)own[j];
                        const int bit = ((c >> (2 - j)) & 1) & across[j];
                        q[v][j] = bit ? pj + n[j] : pj;
                        wrap |= (unsigned int)bit << (3 * v + j);
                    }
                }
                double E1[3], E2[3];
                for (int j = 0; j < 3; j++) {
                    const double a0 = q[1][0] - q[0][0], a1 = q[1][1] - q[0][1], a2 = q[1][2] - q[0][2];
                    const double b0 = q[2][0] - q[0][0], b1 = q[2][1] - q[0][1], b2 = q[2][2] - q[0][2];
                    E1[j] = (a0 * G.A[j] + a1 * G.A[3 + j]) + a2 * G.A[6 + j];
                    E2[j] = (b0 * G.A[j] + b1 * G.A[3 + j]) + b2 * G.A[6 + j];
                }
                const double cx = E1[1] * E2[2] - E1[2] * E2[1], cy = E1[2] * E2[0] - E1[0] * E2[2], cz = E1[0] * E2[1] - E1[1] * E2[0];
                if (ti < O.cap_t) {
                    O.tri[3 * ti] = (long long)id[0]; O.tri[3 * ti + 1] = (long long)id[1]; O.tri[3 * ti + 2] = (long long)id[2];
                    O.wrap[ti] = (unsigned short)wrap;
                    O.cell[ti] = lin;
                    S.nt++;
                }
                S.area += 0.5 * sqrt((cx * cx + cy * cy) + cz * cz);
                ti++;
            }
            // the inside fraction: u(a, b) = the crossing's distance from corner a on the edge towards corner b
            auto u = [&](int a, int b) { return a < b ? te[iso_pair(a, b)] : 1. - te[iso_pair(b, a)]; };
            int in[4], out[4], ki = 0, ko = 0;
            for (int i = 0; i < 4; i++) {
                if ((m >> i) & 1u) in[ki++] = i;
                else out[ko++] = i;
            }
            if (ni == 1) frac = (u(in[0], out[0]) * u(in[0], out[1])) * u(in[0], out[2]);
            else if (ni == 3) frac = 1. - (u(out[0], in[0]) * u(out[0], in[1])) * u(out[0], in[2]);
            else {
                const double uik = u(in[0], out[0]), uil = u(in[0], out[1]), ujk = u(in[1], out[0]), ujl = u(in[1], out[1]);
                frac = (uik * uil + (uik * ujl) * (1. - uil)) + (ujk * ujl) * (1. - uik);
            }
        }
        S.frac += frac;
        const double each = frac / (double)ni;
        for (int i = 0; i < 4; i++) {
            if (!((m >> i) & 1u)) continue;
#pragma unroll
            for (int c = 0; c < 8; c++) share[c] += c == pc[i] ? each : 0.;   // (no dynamic index: the shares stay in registers)
        }
    }
}

// the workgroup's sums to its slot of acc (all threads call it, at the kernel's end).  acc[4 s ..]: area, inside tetrahedra
// (doubles), vertices, triangles written (64-bit integers) of slot s = blockIdx.x % ISO_SLOTS -- one atomic per workgroup and
// value, spread over ISO_SLOTS addresses: a quarter of a million waves adding to ONE address took 3 ms at 512^3
__device__ __forceinline__ void iso_flush(IsoSums S, unsigned long long *acc) {
    __shared__ double s_d[2][TPB / XB_WAVE];
    __shared__ unsigned long long s_n[2][TPB / XB_WAVE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        S.area += __shfl_xor(S.area, o); S.frac += __shfl_xor(S.frac, o);
        S.nv += __shfl_xor(S.nv, o); S.nt += __shfl_xor(S.nt, o);
    }
    if (threadIdx.x % XB_WAVE == 0) {
        const int w = threadIdx.x / XB_WAVE;
        s_d[0][w] = S.area; s_d[1][w] = S.frac; s_n[0][w] = S.nv; s_n[1][w] = S.nt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double area = 0., frac = 0.;
        unsigned long long nv = 0, nt = 0;
        for (int w = 0; w < TPB / XB_WAVE; w++) { area += s_d[0][w]; frac += s_d[1][w]; nv += s_n[0][w]; nt += s_n[1][w]; }
        unsigned long long *slot = acc + 4 * (blockIdx.x % ISO_SLOTS);
        if (area != 0.) atomicAdd(reinterpret_cast<double *>(slot), area);
        if (frac != 0.) atomicAdd(reinterpret_cast<double *>(slot) + 1, frac);
        if (nv) atomicAdd(slot + 2, nv);
        if (nt) atomicAdd(slot + 3, nt);
    }
}
// the cube's shares to the labels of its corners (all lanes call it; share is zero where the lane has nothing)
template <class Sink>
__device__ __forceinline__ void iso_credit(const Sink &K, StAcc &A, const int *__restrict__ labels, int n, bool live, const IsoCorners &C,
                                           const double share[8]) {
#pragma unroll
    for (int c = 0; c < 8; c++) {
        int a = -1;
        if (live && share[c] != 0.) {
            a = labels[C.lin(c)];
            if (a < 0 || a >= n) a = -1;
        }
        st_step2(K, A, a, a >= 0 ? share[c] : 0., 0.);
    }
}

// BINS: 1 <= n <= ST_BINS and the per-label adds go to LDS; n == 0: no labels.  vol, mag, cnt: [n] each, zero on entry
template <bool BINS>
__global__ __launch_bounds__(TPB) void k_iso_emit(int nx, int ny, int nz, const double *__restrict__ f, double level, IsoGeom G,
                                                 const unsigned int *__restrict__ word, const unsigned long long *__restrict__ base, IsoOut O,
                                                 const int *__restrict__ labels, int n, double *vol, double *mag, unsigned long long *cnt,
                                                 unsigned long long *acc) {
    __shared__ IsoTile s_f[CP_TX + 1];
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;
    if (BINS) st_bins_clear(s_bins, n);   // (iso_stage's barrier covers it)
    int x0, y0, z0;
    iso_stage(s_f, nx, ny, nz, f, x0, y0, z0);
    const int tz = threadIdx.x % CP_TZ, ty = threadIdx.x / CP_TZ;
    const int y = y0 + ty, z = z0 + tz;
    const bool col = y < ny && z < nz;
    IsoSums S;
    StAcc A;
#pragma unroll 1
    for (int tx = 0; tx < CP_TX; tx++) {
        const int x = x0 + tx;
        const bool live = col && x < nx;
        const IsoTileReader r{s_f, tx, ty, tz};
        const unsigned cm = live ? iso_cube_mask(r, level) : 0u;
        if (!__ballot(cm != 0u)) continue;   // a wave of cubes that lie outside
        if (n == 0 && !__ballot(cm != 0u && cm != 255u)) {   // ... of whole cubes and cubes outside, and no labels to credit
            if (cm == 255u) S.frac += 6.;
            continue;
        }
        double share[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
        const IsoCorners C(live ? x : 0, live ? y : 0, live ? z : 0, nx, ny, nz);
        if (cm) iso_voxel(r, cm, x, y, z, nx, ny, nz, ((long long)x * ny + y) * nz + z, C, level, G, word, base, O, S, share);
        if (n > 0) {
            if (BINS) iso_credit(s_bins.sink(), A, labels, n, cm != 0u, C, share);
            else iso_credit(StSinkGlb{vol, mag, cnt}, A, labels, n, cm != 0u, C, share);
        }
    }
    if (n > 0) {
        if (BINS) {
            st_finish(s_bins.sink(), A);
            __syncthreads();
            st_bins_flush(s_bins, n, vol, mag, cnt);
        } else
            st_finish(StSinkGlb{vol, mag, cnt}, A);
    }
    iso_flush(S, acc);
}

template <bool BINS>
__global__ __launch_bounds__(TPB) void k_iso_emit_gather(int nx, int ny, int nz, const double *__restrict__ f, double level, IsoGeom G,
                                                        const unsigned int *__restrict__ word, const unsigned long long *__restrict__ base,
                                                        IsoOut O, const int *__restrict__ labels, int n, double *vol, double *mag,
                                                        unsigned long long *cnt, unsigned long long *acc) {
    __shared__ StBins<BINS ? ST_BINS : 1> s_bins;
    if (BINS) {
        st_bins_clear(s_bins, n);
        __syncthreads();
    }
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x, nyz = (long long)ny * nz;
    const bool live = v < nx * nyz;
    const long long vv = live ? v : 0;
    const int x = (int)(vv / nyz), q = (int)(vv - x * nyz), y = q / nz, z = q - y * nz;
    const IsoCorners C(x, y, z, nx, ny, nz);
    const IsoGatherReader r{f, &C};
    const unsigned cm = live ? iso_cube_mask(r, level) : 0u;
    IsoSums S;
    StAcc A;
    double share[8] = {0., 0., 0., 0., 0., 0., 0., 0.};
    if (cm) iso_voxel(r, cm, x, y, z, nx, ny, nz, vv, C, level, G, word, base, O, S, share);
    if (n > 0) {
        if (BINS) {
            const StSinkLds K = s_bins.sink();
            iso_credit(K, A, labels, n, cm != 0u, C, share);
            st_finish(K, A);
            __syncthreads();
            st_bins_flush(s_bins, n, vol, mag, cnt);
        } else {
            const StSinkGlb K{vol, mag, cnt};
            iso_credit(K, A, labels, n, cm != 0u, C, share);
            st_finish(K, A);
        }
    }
    iso_flush(S, acc);
}

// the NCI surface's mask (nci.nci_isosurface): s := XB_ISO_NCI_RAISED where rho >= rho_cut or s is not below it (+inf where rho <= 0)
__global__ __launch_bounds__(TPB) void k_iso_nci_mask(long long N, const double *__restrict__ rho, double rho_cut, double *__restrict__ s) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= N) return;
    if (rho[v] >= rho_cut || !(s[v] < XB_ISO_NCI_RAISED)) s[v] = XB_ISO_NCI_RAISED;
}
