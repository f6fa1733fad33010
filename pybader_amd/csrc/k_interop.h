// k_interop.h -- kernels of the device-array boundary (host_interop.h): a caller's device array becomes the resident
// float64 C-order density, the resident density masked by a label goes out into a caller's device array.  The reference
// has no counterpart (its arrays live in one address space).  Every kernel is a move plus at most one exact widening
// (float -> double) or one rounding (double -> float): memory bound, nothing else to win than coalescing.

// float -> double is exact for every finite value, +-inf and -0.0 (the library is built with float32 denormals on); a NaN
// stays a NaN.

// contiguous float32 -> float64, 4 values per thread: one 16-byte load, two 16-byte stores.  `in` is 16-byte aligned
// (the host checks), n4 = whole groups of four; the caller's k_io_gather does the few values behind them.
__global__ __launch_bounds__(TPB) void k_io_widen4(const float *__restrict__ in, double *__restrict__ out, long long n4) {
    const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
    if (i >= n4) return;
    const float4 q = reinterpret_cast<const float4 *>(in)[i];
    double2 *o = reinterpret_cast<double2 *>(out) + 2 * i;
    o[0] = make_double2((double)q.x, (double)q.y);
    o[1] = make_double2((double)q.z, (double)q.w);
}

// any strides (in elements; 0 = broadcast axis, negative = flipped axis): out[v] = in[x sx + y sy + z sz], one thread per
// voxel `first + ...` of the C-order destination.  Coalesced on the source side when sz is +-1.
template <typename T>
__global__ __launch_bounds__(TPB) void k_io_gather(const T *__restrict__ in, double *__restrict__ out, int ny, int nz,
                                                   long long sx, long long sy, long long sz, long long first, long long N) {
    const long long v = first + (long long)blockIdx.x * TPB + threadIdx.x;
    if (v >= N) return;
    const int z = (int)(v % nz);
    const long long xy = v / nz;
    const int y = (int)(xy % ny), x = (int)(xy / ny);
    out[v] = (double)in[x * sx + y * sy + z * sz];
}

// A permuted layout: the source runs fastest (stride 1) along the destination axis `f` (x or y), not along z.  A tile
// of IO_TILE (f) x IO_TILE (z) values goes through LDS: read with the lanes along f, written with the lanes along z,
// so both sides move whole 512-byte rows.  The tile is stored [f][z] as doubles with a pitch of IO_TILE + 1: the column
// write of the read phase (lanes IO_TILE + 1 doubles apart = 2 banks apart modulo 32) and the row read of the write
// phase are both free of bank conflicts.  `o` is the third axis; so / sz are the source strides of o and z, do / df the
// destination strides of o and f (z has 1).  One tile per workgroup, 4 waves, 16 rows each.
#define IO_TILE 64
template <typename T>
__global__ __launch_bounds__(TPB) void k_io_tiled(const T *__restrict__ in, double *__restrict__ out, int no, int nf, int nz,
                                                  long long so, long long sz, long long d_o, long long d_f, int tiles_f, int tiles_z) {
    __shared__ double tile[IO_TILE][IO_TILE + 1];
    long long b = blockIdx.x;
    const int tz = (int)(b % tiles_z); b /= tiles_z;
    const int tf = (int)(b % tiles_f);
    const long long o = b / tiles_f;
    if (o >= no) return;
    const int lane = threadIdx.x % IO_TILE, row0 = threadIdx.x / IO_TILE;
    const int f0 = tf * IO_TILE, z0 = tz * IO_TILE;
    const T *src = in + o * so;
    if (f0 + lane < nf)
        for (int r = row0; r < IO_TILE && z0 + r < nz; r += TPB / IO_TILE)
            tile[lane][r] = (double)src[(long long)(z0 + r) * sz + (f0 + lane)];
    __syncthreads();
    double *dst = out + o * d_o;
    if (z0 + lane < nz)
        for (int r = row0; r < IO_TILE && f0 + r < nf; r += TPB / IO_TILE)
            dst[(long long)(f0 + r) * d_f + (z0 + lane)] = tile[r][lane];
}

// utils.volume_mask (utils.py:461-476) into a device array: the density where the label equals vol_num, zero elsewhere;
// float64 bit for bit what k_volume_mask writes, float32 that value rounded once (to nearest even).
template <typename T>
__global__ __launch_bounds__(TPB) void k_io_volume(const double *__restrict__ rho, const int *__restrict__ labels, int vol_num,
                                                   T *__restrict__ out, long long N) {
    const long long v = (long long)blockIdx.x * TPB + threadIdx.x;
    if (v < N) out[v] = (labels[v] == vol_num) ? (T)rho[v] : (T)0.;
}
