// host_format.h -- host side of the density text writer (k_format.h, fmt_core.h): values in, text out in chunks of
// whole lines through two pinned buffers, so that the caller writes one chunk to its file while the next one is
// formatted and copied.  Neither side ever holds the whole text (2.4 GB at 512^3).  The state lives in the context
// (c->fmt) between xb_format_begin and xb_format_end; it has its own device buffers and leaves the resident density,
// labels and every other buffer of the context alone.
#pragma once

#define FMT_CHUNK_BYTES ((size_t)64 << 20)   // text per chunk (upper bound)
#define FMT_HOST_CAP (1 << 22)               // values the host may be asked to format

struct FmtState {
    FmtArgs a{};
    double *vals = nullptr, *p10 = nullptr;
    long long *host_idx = nullptr, *host_off = nullptr;
    char *host_txt = nullptr, *text = nullptr;
    int *len = nullptr, *count = nullptr;
    std::vector<long long> host_list;         // sorted indices of the host's values
    long long nlines = 0, next_line = 0, lines_per_chunk = 0;
    size_t text_cap = 0;
    bool ready = false;
    int inflight = -1;                        // slot whose chunk is being formatted / copied
    char *pin[2] = {nullptr, nullptr};
    int *pin_ints = nullptr;
    long long bytes[2] = {0, 0};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};   // ev[slot] before the chunk's kernels, ev[2 + slot] after them
    hipEvent_t done[2] = {nullptr, nullptr};                   // after the chunk's copy into pin[slot]
    double format_ms = 0., copy_ms = 0.;
};

static void fmt_release(xb_ctx *c) {
    if (!c || !c->fmt) return;
    FmtState *s = c->fmt;
    hipStreamSynchronize(c->stream);
    hipFree(s->vals); hipFree(s->p10); hipFree(s->host_idx); hipFree(s->host_off); hipFree(s->host_txt);
    hipFree(s->text); hipFree(s->len); hipFree(s->count);
    for (int k = 0; k < 2; k++) { hipHostFree(s->pin[k]); if (s->done[k]) hipEventDestroy(s->done[k]); }
    for (auto e : s->ev) if (e) hipEventDestroy(e);
    hipHostFree(s->pin_ints);
    delete s;
    c->fmt = nullptr;
}

static int fmt_blocks(long long n) { return (int)std::max<long long>(1, std::min<long long>((n + TPB - 1) / TPB, 1 << 16)); }

int xb_format_begin(xb_ctx *c, const double *values, const int64_t shape[3], int layout, double scale, int style, int prec,
                    const double *pow10, int64_t pow10_lo, int64_t pow10_n, int64_t *n_host) {
    if (!c) return fail(XB_E_ARG, "xb_format_begin: no context");
    HIPCHK(hipSetDevice(c->device));
    fmt_release(c);
    if (!values || !shape || shape[0] <= 0 || shape[1] <= 0 || shape[2] <= 0 || shape[0] > (1 << 20) || shape[1] > (1 << 20) ||
        shape[2] > (1 << 20))
        return fail(XB_E_ARG, "xb_format_begin: bad shape");
    if (layout != XB_TEXT_CHGCAR && layout != XB_TEXT_CUBE) return fail(XB_E_ARG, "xb_format_begin: bad layout %d", layout);
    if (style < FMT_STYLE_E || style > FMT_STYLE_F || prec < 1 || prec > 17) return fail(XB_E_ARG, "xb_format_begin: bad style / precision");
    if (!pow10 || pow10_n <= 0 || pow10_n > 4096 || pow10_lo < -4096 || pow10_lo > 4096) return fail(XB_E_ARG, "xb_format_begin: bad power table");
    const long long N = (long long)shape[0] * shape[1] * shape[2];
    if (N >= (1LL << 40)) return fail(XB_E_LIMIT, "xb_format_begin: %lld values", N);
    FmtState *s = new FmtState;
    c->fmt = s;
    FmtArgs &a = s->a;
    a.n = N;
    a.rec = layout == XB_TEXT_CHGCAR ? N : (long long)shape[2];
    a.per_line = layout == XB_TEXT_CHGCAR ? 5 : 6;
    a.style = style; a.prec = prec;
    a.p10_lo = (int)pow10_lo; a.p10_n = (int)pow10_n;
    double *src = nullptr;
    HIPCHK(hipMalloc(&s->vals, (size_t)N * sizeof(double)));
    HIPCHK(hipMalloc(&src, (size_t)N * sizeof(double)));
    HIPCHK(hipMalloc(&s->p10, (size_t)pow10_n * sizeof(double)));
    HIPCHK(hipMalloc(&s->count, sizeof(int)));
    const int cap = (int)std::min<long long>(N, FMT_HOST_CAP);
    HIPCHK(hipMalloc(&s->host_idx, (size_t)cap * sizeof(long long)));
    HIPCHK(hipMemcpyAsync(s->p10, pow10, (size_t)pow10_n * sizeof(double), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(s->count, 0, sizeof(int), c->stream));
    if (int rc = staged_h2d(c, src, values, (size_t)N * sizeof(double))) { hipStreamSynchronize(c->stream); hipFree(src); return rc; }
    k_fmt_gather<<<fmt_blocks(N), TPB, 0, c->stream>>>(src, N, (int)shape[0], (int)shape[1], (int)shape[2],
                                                       layout == XB_TEXT_CHGCAR ? 0 : 1, scale, s->vals);
    HIPCHK(hipGetLastError());
    a.vals = s->vals; a.p10 = s->p10;
    k_fmt_classify<<<fmt_blocks(N), TPB, 0, c->stream>>>(a, s->host_idx, s->count, cap);
    HIPCHK(hipGetLastError());
    HIPCHK(hipHostMalloc(&s->pin_ints, 64 * sizeof(int)));
    HIPCHK(hipMemcpyAsync(s->pin_ints, s->count, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipFree(src));
    const long long nh = s->pin_ints[0];
    if (nh > cap) return fail(XB_E_LIMIT, "xb_format_begin: %lld values need the host formatter (cap %d)", nh, cap);
    s->host_list.resize(nh);
    if (nh) {
        HIPCHK(hipMemcpy(s->host_list.data(), s->host_idx, nh * sizeof(long long), hipMemcpyDeviceToHost));
        std::sort(s->host_list.begin(), s->host_list.end());
        HIPCHK(hipMemcpy(s->host_idx, s->host_list.data(), nh * sizeof(long long), hipMemcpyHostToDevice));
    }
    a.host_idx = s->host_idx; a.n_host = nh;
    const long long lpr = (a.rec + a.per_line - 1) / a.per_line;
    s->nlines = (N / a.rec) * lpr;
    const long long max_line = (long long)a.per_line * FMT_MAX_VALUE_BYTES(prec) + 1;
    s->lines_per_chunk = std::max<long long>(1, std::min<long long>(s->nlines, (long long)(FMT_CHUNK_BYTES / max_line)));
    s->text_cap = (size_t)(s->lines_per_chunk * max_line);
    const long long L = s->lines_per_chunk;
    HIPCHK(hipMalloc(&s->len, ((size_t)L + L / 1024 + 4096) * sizeof(int)));
    HIPCHK(hipMalloc(&s->text, s->text_cap));
    for (int k = 0; k < 2; k++) {
        HIPCHK(hipHostMalloc(&s->pin[k], s->text_cap));
        HIPCHK(hipEventCreate(&s->done[k]));   // timed: the copy time is done - ev[2 + k]
    }
    for (auto &e : s->ev) HIPCHK(hipEventCreate(&e));
    if (n_host) *n_host = nh;
    return XB_OK;
}

__global__ void k_fmt_take(const double *__restrict__ vals, const long long *__restrict__ idx, long long n, double *__restrict__ out) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n) out[t] = vals[idx[t]];
}

int xb_format_host_values(xb_ctx *c, int64_t *idx, double *vals) {
    if (!c || !c->fmt) return fail(XB_E_STATE, "xb_format_host_values: call xb_format_begin first");
    HIPCHK(hipSetDevice(c->device));
    FmtState *s = c->fmt;
    const long long nh = s->a.n_host;
    if (!nh) return XB_OK;
    if (!idx || !vals) return fail(XB_E_ARG, "xb_format_host_values: null output");
    double *tmp = nullptr;
    HIPCHK(hipMalloc(&tmp, nh * sizeof(double)));
    k_fmt_take<<<(int)((nh + 255) / 256), 256, 0, c->stream>>>(s->vals, s->host_idx, nh, tmp);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(vals, tmp, nh * sizeof(double), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    hipFree(tmp);
    if (e != hipSuccess) return fail(XB_E_HIP, "xb_format_host_values: %s", hipGetErrorString(e));
    memcpy(idx, s->host_list.data(), nh * sizeof(long long));
    return XB_OK;
}

int xb_format_set_host_text(xb_ctx *c, const int64_t *offsets, const char *text) {
    if (!c || !c->fmt) return fail(XB_E_STATE, "xb_format_set_host_text: call xb_format_begin first");
    HIPCHK(hipSetDevice(c->device));
    FmtState *s = c->fmt;
    const long long nh = s->a.n_host;
    if (nh) {
        if (!offsets || !text || offsets[0] != 0) return fail(XB_E_ARG, "xb_format_set_host_text: bad offsets");
        for (long long i = 0; i < nh; i++) {
            const long long w = offsets[i + 1] - offsets[i];
            if (w < 1 || w > FMT_MAX_VALUE_BYTES(s->a.prec))
                return fail(XB_E_ARG, "xb_format_set_host_text: value %lld has %lld bytes of text", (long long)s->host_list[i], w);
        }
        HIPCHK(hipMalloc(&s->host_off, (nh + 1) * sizeof(long long)));
        HIPCHK(hipMalloc(&s->host_txt, (size_t)offsets[nh]));
        HIPCHK(hipMemcpyAsync(s->host_off, offsets, (nh + 1) * sizeof(long long), hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(s->host_txt, text, (size_t)offsets[nh], hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        s->a.host_off = s->host_off; s->a.host_txt = s->host_txt;
    }
    s->ready = true;
    return XB_OK;
}

// the next chunk of lines: kernels + copy into pin[slot], asynchronously (one short wait for the chunk's byte count)
static int fmt_enqueue(xb_ctx *c, int slot) {
    FmtState *s = c->fmt;
    const long long line0 = s->next_line;
    const int L = (int)std::min(s->lines_per_chunk, s->nlines - line0);
    const int nb = (L + TPB - 1) / TPB;
    HIPCHK(hipEventRecord(s->ev[slot], c->stream));
    k_fmt_line_len<<<nb, TPB, 0, c->stream>>>(s->a, line0, L, s->len);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(s->pin_ints, s->len + L - 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (int rc = device_scan(c, s->len, L, s->len + L)) return rc;
    HIPCHK(hipMemcpyAsync(s->pin_ints + 1, s->len + L - 1, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const long long total = (long long)s->pin_ints[0] + s->pin_ints[1];
    if (total <= 0 || (size_t)total > s->text_cap) return fail(XB_E_STATE, "xb_format_next: chunk of %lld bytes (cap %zu)", total, s->text_cap);
    k_fmt_write<<<nb, TPB, 0, c->stream>>>(s->a, line0, L, s->len, s->text);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2 + slot], c->stream));
    HIPCHK(hipMemcpyAsync(s->pin[slot], s->text, (size_t)total, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipEventRecord(s->done[slot], c->stream));
    s->bytes[slot] = total;
    s->next_line = line0 + L;
    s->inflight = slot;
    return XB_OK;
}

int xb_format_next(xb_ctx *c, void **data, int64_t *nbytes) {
    if (!c || !c->fmt || !c->fmt->ready) return fail(XB_E_STATE, "xb_format_next: call xb_format_begin and xb_format_set_host_text first");
    if (!data || !nbytes) return fail(XB_E_ARG, "xb_format_next: null output");
    HIPCHK(hipSetDevice(c->device));
    FmtState *s = c->fmt;
    *data = nullptr; *nbytes = 0;
    if (s->inflight < 0 && s->next_line == 0)
        if (int rc = fmt_enqueue(c, 0)) return rc;
    if (s->inflight < 0) return XB_OK;   // every line delivered
    const int cur = s->inflight;
    HIPCHK(hipEventSynchronize(s->done[cur]));
    float k_ms = 0.f, c_ms = 0.f;
    HIPCHK(hipEventElapsedTime(&k_ms, s->ev[cur], s->ev[2 + cur]));
    HIPCHK(hipEventElapsedTime(&c_ms, s->ev[2 + cur], s->done[cur]));
    s->format_ms += k_ms;
    s->copy_ms += c_ms;
    s->inflight = -1;
    if (s->next_line < s->nlines)
        if (int rc = fmt_enqueue(c, cur ^ 1)) return rc;
    *data = s->pin[cur];
    *nbytes = s->bytes[cur];
    return XB_OK;
}

int xb_format_times(xb_ctx *c, double *format_ms, double *copy_ms) {
    if (!c || !c->fmt) return fail(XB_E_STATE, "xb_format_times: call xb_format_begin first");
    if (format_ms) *format_ms = c->fmt->format_ms;
    if (copy_ms) *copy_ms = c->fmt->copy_ms;
    return XB_OK;
}

int xb_format_end(xb_ctx *c) {
    if (!c) return fail(XB_E_ARG, "xb_format_end: no context");
    HIPCHK(hipSetDevice(c->device));
    fmt_release(c);
    return XB_OK;
}
