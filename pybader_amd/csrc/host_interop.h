// host_interop.h -- host side, part 7: the in-memory boundary for arrays that already live on the device.  A caller's device
// array (a torch / CuPy tensor through __cuda_array_interface__, pybader_amd/device.py) becomes the resident density or label
// map, label maps and masked volumes go out into device arrays -- no trip through host memory.  The reference has no
// counterpart: its arrays live in one address space.
//
// Two rules hold for every entry point here.
//   VALIDATION comes first and happens on the host: the pointer is device memory of the context's device
//   (hipPointerGetAttributes) and every element the shape and strides address lies inside the allocation that holds it
//   (hipMemGetAddressRange).  A bad argument is XB_E_ARG before a kernel, a copy or an event is queued and before any cached
//   state of the context is touched.
//   ORDERING is by events, never by a host wait: the context's stream takes the work up after everything queued on the
//   caller's stream so far (io_after_caller), and the caller's stream goes on after the work (io_before_caller) -- the caller
//   may overwrite or free a source, or read a destination, on its stream right after the call returns.

static size_t io_float_size(int dtype) { return dtype == XB_F32 ? 4 : (dtype == XB_F64 ? 8 : 0); }

// The bytes [lo, hi) that `shape` and `stride` (in elements of isz bytes; zero and negative strides allowed) address from p
// must be device memory of c's device inside ONE allocation.  128-bit arithmetic: a stride is any int64.
static int io_check(xb_ctx *c, const char *who, const void *p, size_t isz, const int64_t shape[3], const int64_t stride[3],
                    uintptr_t *lo_out, uintptr_t *hi_out) {
    if (!p) return fail(XB_E_ARG, "%s: null device pointer", who);
    __int128 lo = 0, hi = 0;
    for (int j = 0; j < 3; j++) {
        const __int128 reach = (__int128)(shape[j] - 1) * stride[j];
        (reach < 0 ? lo : hi) += reach;
    }
    lo *= (__int128)isz;
    hi = (hi + 1) * (__int128)isz;
    hipPointerAttribute_t a;
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(XB_E_ARG, "%s: %p is not memory the HIP runtime knows (a host pointer?)", who, p);
    }
    if (a.type != hipMemoryTypeDevice) return fail(XB_E_ARG, "%s: %p is not device memory (memory type %d)", who, p, (int)a.type);
    if (a.device != c->device) return fail(XB_E_ARG, "%s: %p lives on device %d, the context on device %d", who, p, a.device, c->device);
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)p) != hipSuccess) {
        (void)hipGetLastError();
        return fail(XB_E_ARG, "%s: no allocation holds %p", who, p);
    }
    const __int128 first = (__int128)(uintptr_t)p + lo, last = (__int128)(uintptr_t)p + hi;
    if (first < (__int128)(uintptr_t)base || last > (__int128)(uintptr_t)base + (__int128)size)
        return fail(XB_E_ARG, "%s: shape and strides address bytes [%lld, %lld) from %p, its allocation holds [%lld, %lld)", who,
                    (long long)lo, (long long)hi, p, (long long)((uintptr_t)base - (uintptr_t)p),
                    (long long)((uintptr_t)base + size - (uintptr_t)p));
    *lo_out = (uintptr_t)first;
    *hi_out = (uintptr_t)last;
    return XB_OK;
}
static bool io_overlaps(uintptr_t lo, uintptr_t hi, const void *buf, size_t bytes) {
    return buf && lo < (uintptr_t)buf + bytes && (uintptr_t)buf < hi;
}
// a C-contiguous array of N elements
static int io_check_flat(xb_ctx *c, const char *who, const void *p, size_t isz, uintptr_t *lo, uintptr_t *hi) {
    const int64_t shape[3] = {(int64_t)c->N, 1, 1}, stride[3] = {1, 0, 0};
    return io_check(c, who, p, isz, shape, stride, lo, hi);
}
// ... that must also be aligned to its elements: the check of every dense device array a caller hands in or asks for
static int io_check_dense(xb_ctx *c, const char *who, const void *p, size_t isz, uintptr_t *lo, uintptr_t *hi) {
    if ((uintptr_t)p % isz) return fail(XB_E_ARG, "%s: %p is not aligned to its %zu-byte elements", who, p, isz);
    return io_check_flat(c, who, p, isz, lo, hi);
}

static int io_event(xb_ctx *c) {
    if (!c->io_ev) HIPCHK(hipEventCreateWithFlags(&c->io_ev, hipEventDisableTiming));
    return XB_OK;
}
static int io_after_caller(xb_ctx *c, hipStream_t s) {
    if (s == c->stream) return XB_OK;
    if (int rc = io_event(c)) return rc;
    HIPCHK(hipEventRecord(c->io_ev, s));
    HIPCHK(hipStreamWaitEvent(c->stream, c->io_ev, 0));
    return XB_OK;
}
static int io_before_caller(xb_ctx *c, hipStream_t s) {
    if (s == c->stream) return XB_OK;
    HIPCHK(hipEventRecord(c->io_ev, c->stream));
    HIPCHK(hipStreamWaitEvent(s, c->io_ev, 0));
    return XB_OK;
}

int xb_device_alloc(int device, int64_t bytes, void **out) {
    if (!out || bytes <= 0) return fail(XB_E_ARG, "xb_device_alloc: bad argument");
    HIPCHK(hipSetDevice(device));
    void *p = nullptr;
    HIPCHK(hipMalloc(&p, (size_t)bytes));
    *out = p;
    return XB_OK;
}
int xb_device_free(void *p) {
    if (p) HIPCHK(hipFree(p));   // (waits for the device: work still queued on the buffer, on any stream, ends first)
    return XB_OK;
}

extern "C++" {
// (dst: the resident density, or the weight method's integrand buffer)
template <typename T>
static int io_import_density(xb_ctx *c, const T *src, const int64_t st[3], double *dst) {
    const Grid &g = c->g;
    const long long N = c->N, sx = st[0], sy = st[1], sz = st[2];
    const bool contiguous = sz == 1 && sy == g.nz && sx == g.nyz;
    long long first = 0;
    if (contiguous && sizeof(T) == 8) {
        HIPCHK(hipMemcpyAsync(dst, src, (size_t)N * 8, hipMemcpyDeviceToDevice, c->stream));
        return XB_OK;
    }
    if constexpr (sizeof(T) == 4)
        if (contiguous && (uintptr_t)src % 16 == 0) {
            const long long n4 = N / 4;
            k_io_widen4<<<nblocks(n4), TPB, 0, c->stream>>>(src, dst, n4);
            HIPCHK(hipGetLastError());
            first = 4 * n4;      // (the up to three values behind the last whole group: the gather below)
            if (first == N) return XB_OK;
        }
    if (first == 0 && sz != 1 && (sy == 1 || sx == 1) && c->opt.io_tiled) {
        const bool fy = sy == 1;     // the source's fast axis is y (else x); o is the other one
        const int nf = fy ? g.ny : g.nx, no = fy ? g.nx : g.ny;
        const int tiles_f = (nf + IO_TILE - 1) / IO_TILE, tiles_z = (g.nz + IO_TILE - 1) / IO_TILE;
        const long long blocks = (long long)tiles_f * tiles_z * no;   // < N / 9 + ...: fits the grid's 2^31 - 1
        k_io_tiled<T><<<(unsigned)blocks, TPB, 0, c->stream>>>(src, dst, no, nf, g.nz, fy ? sx : sy, sz, fy ? (long long)g.nyz : g.nz,
                                                              fy ? (long long)g.nz : g.nyz, tiles_f, tiles_z);
        HIPCHK(hipGetLastError());
        return XB_OK;
    }
    k_io_gather<T><<<nblocks(N - first), TPB, 0, c->stream>>>(src, dst, g.ny, g.nz, sx, sy, sz, first, N);
    HIPCHK(hipGetLastError());
    return XB_OK;
}
}  // extern "C++"

int xb_import_density(xb_ctx *c, const void *dev_ptr, int dtype, const int64_t stride[3], void *stream) {
    if (!c || !c->has_grid) return fail(XB_E_ARG, "xb_import_density: call xb_set_grid first");
    const size_t isz = io_float_size(dtype);
    if (!isz) return fail(XB_E_ARG, "xb_import_density: dtype code %d is neither XB_F32 nor XB_F64", dtype);
    if (!stride) return fail(XB_E_ARG, "xb_import_density: null stride");
    if ((uintptr_t)dev_ptr % isz) return fail(XB_E_ARG, "xb_import_density: %p is not aligned to its %zu-byte elements", dev_ptr, isz);
    HIPCHK(hipSetDevice(c->device));
    const int64_t shape[3] = {c->g.nx, c->g.ny, c->g.nz};
    uintptr_t lo, hi;
    if (int rc = io_check(c, "xb_import_density", dev_ptr, isz, shape, stride, &lo, &hi)) return rc;
    if (io_overlaps(lo, hi, c->rho, (size_t)c->N * 8)) return fail(XB_E_ARG, "xb_import_density: the source overlaps the resident density");
    // from here on as xb_upload_density
    vacuum_marks_unproven(*c);
    NEED_GRID_THIN("xb_import_density");
    density_written(*c);
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = io_after_caller(c, s)) return rc;
    if (int rc = dtype == XB_F32 ? io_import_density(c, (const float *)dev_ptr, stride, c->rho) : io_import_density(c, (const double *)dev_ptr, stride, c->rho)) return rc;
    return io_before_caller(c, s);
}

int xb_import_labels(xb_ctx *c, const void *dev_ptr, int dtype, void *stream) {
    if (!c || !c->has_grid) return fail(XB_E_ARG, "xb_import_labels: call xb_set_grid first");
    const size_t sz = dtype_size(dtype);
    if (!sz) return fail(XB_E_ARG, "xb_import_labels: bad dtype code %d", dtype);
    HIPCHK(hipSetDevice(c->device));
    uintptr_t lo, hi;
    if (int rc = io_check_dense(c, "xb_import_labels", dev_ptr, sz, &lo, &hi)) return rc;
    if (io_overlaps(lo, hi, c->labels, (size_t)c->N * 4)) return fail(XB_E_ARG, "xb_import_labels: the source overlaps the resident labels");
    labels_overwritten(*c, sz >= 4 ? 4 : (int)sz, true);   // from here on as xb_upload_labels
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = io_after_caller(c, s)) return rc;
    if (dtype == XB_I32) HIPCHK(hipMemcpyAsync(c->labels, dev_ptr, (size_t)c->N * 4, hipMemcpyDeviceToDevice, c->stream));
    else if (dtype == XB_I8) k_widen<int8_t><<<nblocks(c->N), TPB, 0, c->stream>>>((const int8_t *)dev_ptr, c->labels, c->N);
    else if (dtype == XB_I16) k_widen<int16_t><<<nblocks(c->N), TPB, 0, c->stream>>>((const int16_t *)dev_ptr, c->labels, c->N);
    else k_widen<long long><<<nblocks(c->N), TPB, 0, c->stream>>>((const long long *)dev_ptr, c->labels, c->N);
    HIPCHK(hipGetLastError());
    if (int rc = io_before_caller(c, s)) return rc;
    // vacuum voxels present?  (as xb_upload_labels asks: its one wait, not one more)
    HIPCHK(hipMemsetAsync(c->counters + CT_ANY_EQUAL, 0, sizeof(int), c->stream));
    k_any_equal<<<2048, TPB, 0, c->stream>>>(c->labels, c->N, -1, c->counters + CT_ANY_EQUAL);
    HIPCHK(hipGetLastError());
    int any = 0;
    if (int rc = read_counter(c, CT_ANY_EQUAL, &any)) return rc;
    c->has_vacuum = any != 0;
    return XB_OK;
}

int xb_export_labels(xb_ctx *c, void *dev_ptr, int dtype, void *stream) {
    if (!c || !c->has_grid) return fail(XB_E_ARG, "xb_export_labels: call xb_set_grid first");
    const size_t sz = dtype_size(dtype);
    if (!sz) return fail(XB_E_ARG, "xb_export_labels: bad dtype code %d", dtype);
    HIPCHK(hipSetDevice(c->device));
    uintptr_t lo, hi;
    if (int rc = io_check_dense(c, "xb_export_labels", dev_ptr, sz, &lo, &hi)) return rc;
    if (io_overlaps(lo, hi, c->labels, (size_t)c->N * 4)) return fail(XB_E_ARG, "xb_export_labels: the destination overlaps the resident labels");
    NEED_GRID_THIN("xb_export_labels");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = io_after_caller(c, s)) return rc;
    const long long N = c->N;
    if (dtype == XB_I32) HIPCHK(hipMemcpyAsync(dev_ptr, c->labels, (size_t)N * 4, hipMemcpyDeviceToDevice, c->stream));
    else if (dtype == XB_I64) k_narrow<long long><<<nblocks(N), TPB, 0, c->stream>>>(c->labels, (long long *)dev_ptr, N);
    else {
        // 16 bytes of narrowed labels per thread where the destination allows the 16-byte stores, plain behind them
        const long long per = 16 / (long long)sz, n16 = (uintptr_t)dev_ptr % 16 == 0 ? N / per : 0, done = n16 * per;
        if (dtype == XB_I8) {
            if (n16) k_narrow_vec<int8_t><<<nblocks(n16), TPB, 0, c->stream>>>(c->labels, (int8_t *)dev_ptr, n16);
            if (done < N) k_narrow<int8_t><<<nblocks(N - done), TPB, 0, c->stream>>>(c->labels + done, (int8_t *)dev_ptr + done, N - done);
        } else {
            if (n16) k_narrow_vec<int16_t><<<nblocks(n16), TPB, 0, c->stream>>>(c->labels, (int16_t *)dev_ptr, n16);
            if (done < N) k_narrow<int16_t><<<nblocks(N - done), TPB, 0, c->stream>>>(c->labels + done, (int16_t *)dev_ptr + done, N - done);
        }
    }
    HIPCHK(hipGetLastError());
    return io_before_caller(c, s);
}

int xb_export_volume(xb_ctx *c, int64_t vol_num, void *dev_ptr, int dtype, void *stream) {
    if (!c || !c->has_grid) return fail(XB_E_ARG, "xb_export_volume: call xb_set_grid first");
    const size_t isz = io_float_size(dtype);
    if (!isz) return fail(XB_E_ARG, "xb_export_volume: dtype code %d is neither XB_F32 nor XB_F64", dtype);
    if ((uintptr_t)dev_ptr % isz) return fail(XB_E_ARG, "xb_export_volume: %p is not aligned to its %zu-byte elements", dev_ptr, isz);
    if (vol_num < -XB_INT_MAX || vol_num > XB_INT_MAX) return fail(XB_E_ARG, "xb_export_volume: volume number %lld is no label", (long long)vol_num);
    HIPCHK(hipSetDevice(c->device));
    uintptr_t lo, hi;
    if (int rc = io_check_flat(c, "xb_export_volume", dev_ptr, isz, &lo, &hi)) return rc;
    if (io_overlaps(lo, hi, c->labels, (size_t)c->N * 4) || io_overlaps(lo, hi, c->rho, (size_t)c->N * 8))
        return fail(XB_E_ARG, "xb_export_volume: the destination overlaps the resident density or labels");
    NEED_GRID("xb_export_volume");
    const hipStream_t s = (hipStream_t)stream;
    if (int rc = io_after_caller(c, s)) return rc;
    if (dtype == XB_F64) k_io_volume<double><<<nblocks(c->N), TPB, 0, c->stream>>>(c->rho, c->labels, (int)vol_num, (double *)dev_ptr, c->N);
    else k_io_volume<float><<<nblocks(c->N), TPB, 0, c->stream>>>(c->rho, c->labels, (int)vol_num, (float *)dev_ptr, c->N);
    HIPCHK(hipGetLastError());
    return io_before_caller(c, s);
}

// `bytes` of a device array to host memory, after everything queued on the caller's stream so far (DeviceArray.to_host);
// returns with the data on the host
int xb_device_read(xb_ctx *c, void *dst_host, const void *dev_ptr, int64_t bytes, void *stream) {
    if (!c || !dst_host || bytes <= 0) return fail(XB_E_ARG, "xb_device_read: bad argument");
    HIPCHK(hipSetDevice(c->device));
    const int64_t shape[3] = {bytes, 1, 1}, stride[3] = {1, 0, 0};
    uintptr_t lo, hi;
    if (int rc = io_check(c, "xb_device_read", dev_ptr, 1, shape, stride, &lo, &hi)) return rc;
    if (int rc = io_after_caller(c, (hipStream_t)stream)) return rc;
    return staged_d2h(c, dst_host, dev_ptr, (size_t)bytes);
}
