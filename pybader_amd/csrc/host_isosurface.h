// host_isosurface.h -- host side, part 18: isosurfaces by marching tetrahedra (k_isosurface.h).  xb_isosurface reads the resident
// density or a caller's field (and the resident labels with n >= 1) of the whole grid and writes nothing resident.
//
// Scratch: the per-voxel words (4 N bytes), the runs' bases (16 bytes per ISO_BLOCK voxels) and the chunks' bases live in `stage`
// (N doubles on a whole grid: need_scratch), which is scratch between calls; the per-label sums and the workgroups' sums
// (4 ISO_SLOTS words) in temporary buffers.
// Kept (the blocks BLK_ISO_* of ctx_buffers.h, freed by xb_isosurface_release, discarded by every writer of the density): the mesh
// of the last call -- vertices [3 V] doubles, colours [V] doubles with a colour field, triangles [3 T] and cells [T] 64-bit integers,
// wraps [T] 16-bit integers; every array at least one element long.

static void isosurface_forget(xb_ctx *c) {
    c->iso_v = 0; c->iso_t = 0; c->iso_have = false;
    std::vector<double>().swap(c->iso_vbl);
}
static void isosurface_drop(xb_ctx *c) { isosurface_forget(c); release(c, BLK_ISO_VERT, BLK_ISO_WRAP); }   // the result and its mesh

int xb_isosurface_table(uint8_t *out) {
    if (!out) return fail(XB_E_ARG, "xb_isosurface_table: null argument");
    std::memcpy(out, iso_tab_h.e, XB_ISO_TABLE_SIZE);
    return XB_OK;
}

int xb_isosurface(xb_ctx *c, const void *field_dev, const void *colour_dev, const double lattice[9], double level, int64_t n_labels,
                  int flags, int64_t counts[2]) {
    ANALYSIS_NEED_GRID("xb_isosurface");
    if (!lattice || !counts) return fail(XB_E_ARG, "xb_isosurface: null argument");
    if (flags & ~XB_ISO_GATHER) return fail(XB_E_ARG, "xb_isosurface: unknown flag bits 0x%x", flags & ~XB_ISO_GATHER);
    if (!std::isfinite(level)) return fail(XB_E_ARG, "xb_isosurface: the level (%g) must be finite", level);
    if (n_labels < 0) return fail(XB_E_ARG, "xb_isosurface: %lld labels", (long long)n_labels);
    if (n_labels > XB_INT_MAX) return fail(XB_E_LIMIT, "xb_isosurface: %lld labels exceed %d", (long long)n_labels, XB_INT_MAX);
    if (c->N > INT64_MAX / 7) return fail(XB_E_LIMIT, "xb_isosurface: 7 x %lld edges exceed the 64-bit range", c->N);
    StCoeffs K;
    if (int rc = stencil_ready(c, "xb_isosurface", lattice, n_labels >= 1, &K)) return rc;   // (the whole grid, a density, labels, a sound lattice)
    HIPCHK(hipSetDevice(c->device));
    const Grid &g = c->g;
    const size_t fbytes = (size_t)c->N * sizeof(double);
    const long long nb = (c->N + ISO_BLOCK - 1) / ISO_BLOCK, np = (nb + ISO_CHUNK - 1) / ISO_CHUNK;
    const size_t off_tot = ((size_t)c->N * 4 + 15) / 16 * 16, off_part = off_tot + (size_t)nb * 16, off_grand = off_part + (size_t)np * 16;
    if (c->stage_bytes < fbytes || c->stage_bytes < off_grand + 16) return fail(XB_E_STATE, "xb_isosurface: the scratch buffer holds no whole grid");
    uintptr_t lo[2] = {0, 0}, hi[2] = {0, 0};
    const void *const in[2] = {field_dev, colour_dev};
    for (int k = 0; k < 2; k++) {
        if (!in[k]) continue;
        if (int rc = io_check_dense(c, "xb_isosurface", in[k], sizeof(double), &lo[k], &hi[k])) return rc;
        if (io_overlaps(lo[k], hi[k], c->stage, c->stage_bytes)) return fail(XB_E_ARG, "xb_isosurface: a field overlaps the context's scratch");
    }
    if (field_dev && colour_dev && lo[0] < hi[1] && lo[1] < hi[0] && field_dev != colour_dev)
        return fail(XB_E_ARG, "xb_isosurface: the field and the colour overlap without being the same array");
    if (int rc = settle_labels(c)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    isosurface_drop(c);
    stage_clobbered(*c);
    const double *f = field_dev ? (const double *)field_dev : c->rho;
    const double *gcol = (const double *)colour_dev;
    unsigned int *word = reinterpret_cast<unsigned int *>(c->stage);
    unsigned long long *tot = reinterpret_cast<unsigned long long *>((char *)c->stage + off_tot);
    unsigned long long *part = reinterpret_cast<unsigned long long *>((char *)c->stage + off_part);
    unsigned long long *grand = reinterpret_cast<unsigned long long *>((char *)c->stage + off_grand);
    const unsigned tiles = stencil_tiles(g);   // (the tile of the critical points and the stencil)
    const bool gather = (flags & XB_ISO_GATHER) != 0;
    if (gather) k_iso_count_gather<<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, word);
    else k_iso_count<<<tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, word);
    HIPCHK(hipGetLastError());
    k_iso_offsets<<<(unsigned)nb, TPB, 0, c->stream>>>(c->N, word, tot);
    k_iso_scan_sums<<<(unsigned)np, TPB, 0, c->stream>>>(tot, nb, part);
    k_iso_scan_top<<<1, XB_WAVE, 0, c->stream>>>(part, np, grand);
    k_iso_scan_apply<<<(unsigned)np, TPB, 0, c->stream>>>(tot, nb, part);
    HIPCHK(hipGetLastError());
    unsigned long long want[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(want, grand, sizeof want, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t V = (size_t)want[0], T = (size_t)want[1];
    if (want[0] > 7ull * (unsigned long long)c->N || want[1] > 12ull * (unsigned long long)c->N)
        return fail(XB_E_STATE, "xb_isosurface: the count pass reports %llu vertices and %llu triangles on %lld voxels", want[0], want[1], c->N);
    const size_t v1 = std::max<size_t>(V, 1), t1 = std::max<size_t>(T, 1);
    const BufWant mesh[] = {{BLK_ISO_VERT, v1 * 3 * sizeof(double), 0}, {BLK_ISO_COL, gcol ? v1 * sizeof(double) : 0, 0},
                            {BLK_ISO_TRI, t1 * 3 * sizeof(long long), 0}, {BLK_ISO_CELL, t1 * sizeof(long long), 0},
                            {BLK_ISO_WRAP, t1 * sizeof(unsigned short), 0}};
    if (int rc = reserve(c, mesh)) return rc;   // (all five or none)
    const int n = (int)n_labels;
    DevBuf<double> sums;
    HIPCHK(sums.alloc(3 * (size_t)n));
    double *vol = sums.p, *mag = vol + n;
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(mag + n);
    DevBuf<unsigned long long> slots;
    HIPCHK(slots.alloc(4 * ISO_SLOTS));
    unsigned long long *acc = slots.p;
    if (n) HIPCHK(hipMemsetAsync(vol, 0, 3 * (size_t)n * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(acc, 0, 4 * ISO_SLOTS * sizeof(unsigned long long), c->stream));
    IsoGeom G;
    const double dims[3] = {(double)g.nx, (double)g.ny, (double)g.nz};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G.A[3 * i + j] = lattice[3 * i + j] / dims[i];
    const IsoOut O{c->ptr<double>(BLK_ISO_VERT), c->ptr<double>(BLK_ISO_COL), c->ptr<long long>(BLK_ISO_TRI), c->ptr<unsigned short>(BLK_ISO_WRAP), c->ptr<long long>(BLK_ISO_CELL), (unsigned long long)V, (unsigned long long)T, gcol};
    const bool bins = n >= 1 && n <= ST_BINS;
    if (gather) {
        if (bins) k_iso_emit_gather<true><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, G, word, tot, O, c->labels, n, vol, mag, cnt, acc);
        else k_iso_emit_gather<false><<<nblocks(c->N), TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, G, word, tot, O, c->labels, n, vol, mag, cnt, acc);
    } else {
        if (bins) k_iso_emit<true><<<tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, G, word, tot, O, c->labels, n, vol, mag, cnt, acc);
        else k_iso_emit<false><<<tiles, TPB, 0, c->stream>>>(g.nx, g.ny, g.nz, f, level, G, word, tot, O, c->labels, n, vol, mag, cnt, acc);
    }
    HIPCHK(hipGetLastError());
    unsigned long long per_slot[4 * ISO_SLOTS], got[4] = {0, 0, 0, 0};
    c->iso_vbl.assign((size_t)n, 0.);
    HIPCHK(hipMemcpyAsync(per_slot, acc, sizeof per_slot, hipMemcpyDeviceToHost, c->stream));
    if (n) HIPCHK(hipMemcpyAsync(c->iso_vbl.data(), vol, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double sc[2] = {0., 0.};
    for (int k = 0; k < ISO_SLOTS; k++) {
        double d[2];
        std::memcpy(d, per_slot + 4 * k, sizeof d);
        sc[0] += d[0]; sc[1] += d[1];
        got[2] += per_slot[4 * k + 2]; got[3] += per_slot[4 * k + 3];
    }
    if (got[2] != want[0] || got[3] != want[1]) {
        isosurface_drop(c);
        return fail(XB_E_STATE, "xb_isosurface: %llu vertices and %llu triangles written, %llu and %llu were counted", got[2], got[3], want[0], want[1]);
    }
    // |det A| / 6, the determinant in the order of xb_stencil_coeffs
    const double *A = G.A;
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double tet = std::fabs((A[0] * c00 + A[1] * c01) + A[2] * c02) / 6.;
    c->iso_area = sc[0];
    c->iso_volume = sc[1] * tet;
    for (double &x : c->iso_vbl) x *= tet;
    c->iso_v = V; c->iso_t = T;
    c->iso_have = true;
    counts[0] = (int64_t)V; counts[1] = (int64_t)T;
    return XB_OK;
}

int xb_isosurface_fetch(xb_ctx *c, int on_device, void *vertices, void *colour, void *triangles, void *wrap, void *cell, int64_t cap_vertices,
                        int64_t cap_triangles, double scalars[2], double *volume_by_label, int64_t cap_labels) {
    if (!c || !c->iso_have) return fail(XB_E_STATE, "xb_isosurface_fetch: no result (call xb_isosurface first)");
    if (!vertices || !triangles || !wrap || !cell || !scalars) return fail(XB_E_ARG, "xb_isosurface_fetch: null argument");
    if (colour && !c->bytes(BLK_ISO_COL)) return fail(XB_E_ARG, "xb_isosurface_fetch: the surface was made without a colour field");
    const size_t V = c->iso_v, T = c->iso_t, nl = c->iso_vbl.size();
    if (cap_vertices < (int64_t)V || cap_triangles < (int64_t)T)
        return fail(XB_E_ARG, "xb_isosurface_fetch: capacity (%lld, %lld) below %lld vertices and %lld triangles", (long long)cap_vertices,
                    (long long)cap_triangles, (long long)V, (long long)T);
    if (nl && (!volume_by_label || cap_labels < (int64_t)nl))
        return fail(XB_E_ARG, "xb_isosurface_fetch: room for %lld labels, %lld were summed", (long long)(volume_by_label ? cap_labels : 0), (long long)nl);
    HIPCHK(hipSetDevice(c->device));
    void *const dst[5] = {vertices, colour, triangles, wrap, cell};
    const void *const src[5] = {c->blk[BLK_ISO_VERT].p, c->blk[BLK_ISO_COL].p, c->blk[BLK_ISO_TRI].p, c->blk[BLK_ISO_WRAP].p, c->blk[BLK_ISO_CELL].p};
    const size_t bytes[5] = {V * 24, V * 8, T * 24, T * 2, T * 8}, elem[5] = {8, 8, 8, 2, 8};
    if (on_device) {
        uintptr_t lo[5], hi[5];
        for (int k = 0; k < 5; k++) {
            if (!dst[k] || !bytes[k]) { lo[k] = hi[k] = 0; continue; }
            if ((uintptr_t)dst[k] % elem[k]) return fail(XB_E_ARG, "xb_isosurface_fetch: %p is not aligned to its %zu-byte elements", dst[k], elem[k]);
            const int64_t shape[3] = {(int64_t)(bytes[k] / elem[k]), 1, 1}, stride[3] = {1, 0, 0};
            if (int rc = io_check(c, "xb_isosurface_fetch", dst[k], elem[k], shape, stride, &lo[k], &hi[k])) return rc;
            for (int j = 0; j < k; j++)
                if (lo[j] < hi[k] && lo[k] < hi[j]) return fail(XB_E_ARG, "xb_isosurface_fetch: two destinations overlap");
        }
    }
    for (int k = 0; k < 5; k++)
        if (dst[k] && bytes[k]) HIPCHK(hipMemcpyAsync(dst[k], src[k], bytes[k], on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    scalars[0] = c->iso_area; scalars[1] = c->iso_volume;
    if (nl) std::memcpy(volume_by_label, c->iso_vbl.data(), nl * sizeof(double));
    return XB_OK;
}

int xb_isosurface_nci_mask(xb_ctx *c, void *s_dev, double rho_cut) {
    ANALYSIS_NEED_GRID("xb_isosurface_nci_mask");
    if (int rc = analysis_ready(c, "xb_isosurface_nci_mask", "", NEED_RHO)) return rc;
    if (c->g.x1 - c->g.x0 != c->g.nx) return fail(XB_E_STATE, "xb_isosurface_nci_mask: the context holds a slab");
    if (!(rho_cut == rho_cut)) return fail(XB_E_ARG, "xb_isosurface_nci_mask: rho_cut is NaN");
    if (!s_dev || (uintptr_t)s_dev % sizeof(double)) return fail(XB_E_ARG, "xb_isosurface_nci_mask: %p is null or not aligned to its 8-byte elements", s_dev);
    uintptr_t lo, hi;
    if (int rc = io_check_flat(c, "xb_isosurface_nci_mask", s_dev, sizeof(double), &lo, &hi)) return rc;
    if (io_overlaps(lo, hi, c->rho, (size_t)c->N * sizeof(double))) return fail(XB_E_ARG, "xb_isosurface_nci_mask: the field overlaps the resident density");
    HIPCHK(hipSetDevice(c->device));
    k_iso_nci_mask<<<nblocks(c->N), TPB, 0, c->stream>>>(c->N, c->rho, rho_cut, (double *)s_dev);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    return XB_OK;
}

int xb_stream_wait(xb_ctx *c, void *stream) {
    if (!c) return fail(XB_E_ARG, "xb_stream_wait: null ctx");
    HIPCHK(hipSetDevice(c->device));
    return io_after_caller(c, (hipStream_t)stream);
}

int xb_device_write(xb_ctx *c, void *dev_ptr, const void *src_host, int64_t bytes) {
    if (!c) return fail(XB_E_ARG, "xb_device_write: null ctx");
    if (!dev_ptr || !src_host || bytes < 0) return fail(XB_E_ARG, "xb_device_write: bad argument");
    if (bytes == 0) return XB_OK;
    HIPCHK(hipSetDevice(c->device));
    uintptr_t lo, hi;
    const int64_t shape[3] = {bytes, 1, 1}, stride[3] = {1, 0, 0};
    if (int rc = io_check(c, "xb_device_write", dev_ptr, 1, shape, stride, &lo, &hi)) return rc;
    if (int rc = staged_h2d(c, dev_ptr, src_host, (size_t)bytes)) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));   // (the source may go once this returns)
    return XB_OK;
}
