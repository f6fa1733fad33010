// k_format.h -- device kernels of libbader_hip.so: a float64 density -> the text block of a CHGCAR or cube file.
// Included by bader_hip.hip (one translation unit); the digits come from fmt_core.h (host and device alike).
#pragma once
#include "fmt_core.h"

// ---------------------------------------------------------------------------------------------
// io/vasp.py:167-250 and io/cube.py:186-240 write the density with utils.python_format / fortran_format (utils.py:40-94),
// one str.format per value: about 2 minutes for a 512^3 block.  Here:
//   k_fmt_gather     values in file order, times the scale (one IEEE multiply, as `density *= lattice_vol`)
//   k_fmt_classify   lists the values the device cannot prove (host fallback, formatted in Python)
//   then per chunk of whole lines:
//   k_fmt_line_len   bytes of every line (values + '\n'); exclusive scan -> byte offsets within the chunk
//   k_fmt_write      the text of every line at its offset
// Layout: a file is records of `rec` values, each record in lines of `per_line` values, the last one partial
// (CHGCAR: one record of N values in lines of 5; cube: nx*ny records of nz values in lines of 6).
// ---------------------------------------------------------------------------------------------
struct FmtArgs {
    const double *vals;       // scaled, in file order
    long long n, rec;
    int per_line, style, prec;
    const double *p10;
    int p10_lo, p10_n;
    const long long *host_idx;   // sorted value indices formatted by the host
    const long long *host_off;   // their text: host_txt[host_off[i] .. host_off[i+1])
    const char *host_txt;
    long long n_host;
};

// file order: 0 = Fortran (x fastest, CHGCAR), 1 = C ([x][y][z], cube)
__global__ __launch_bounds__(TPB) void k_fmt_gather(const double *__restrict__ src, long long n, int nx, int ny, int nz,
                                                    int order, double scale, double *__restrict__ dst) {
    for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < n; t += (long long)gridDim.x * TPB) {
        long long s = t;
        if (order == 0) {
            const long long x = t % nx, r = t / nx;
            s = (x * ny + r % ny) * nz + r / ny;
        }
        dst[t] = src[s] * scale;
    }
}

__global__ __launch_bounds__(TPB) void k_fmt_classify(FmtArgs a, long long *__restrict__ idx, int *count, int cap) {
    for (long long t = (long long)blockIdx.x * TPB + threadIdx.x; t < a.n; t += (long long)gridDim.x * TPB) {
        if (fmt_value(a.vals[t], a.style, a.prec, a.p10, a.p10_lo, a.p10_n, nullptr) < 0) {
            const int k = atomicAdd(count, 1);
            if (k < cap) idx[k] = t;
        }
    }
}

// position of value t in the host list (present by construction)
__device__ __forceinline__ long long fmt_host_slot(const FmtArgs &a, long long t) {
    long long lo = 0, hi = a.n_host - 1;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (a.host_idx[mid] < t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
__device__ __forceinline__ void fmt_line_range(const FmtArgs &a, long long line, long long &first, int &count) {
    const long long lpr = (a.rec + a.per_line - 1) / a.per_line;   // lines per record
    const long long r = line / lpr, w = line - r * lpr;
    first = r * a.rec + w * a.per_line;
    count = (int)min((long long)a.per_line, a.rec - w * a.per_line);
}

__global__ __launch_bounds__(TPB) void k_fmt_line_len(FmtArgs a, long long line0, int nlines, int *__restrict__ len) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= nlines) return;
    long long first;
    int count;
    fmt_line_range(a, line0 + j, first, count);
    int total = 1;   // '\n'
    for (int i = 0; i < count; i++) {
        int b = fmt_value(a.vals[first + i], a.style, a.prec, a.p10, a.p10_lo, a.p10_n, nullptr);
        if (b < 0) {
            const long long s = fmt_host_slot(a, first + i);
            b = (int)(a.host_off[s + 1] - a.host_off[s]);
        }
        total += b;
    }
    len[j] = total;
}

__global__ __launch_bounds__(TPB) void k_fmt_write(FmtArgs a, long long line0, int nlines, const int *__restrict__ off,
                                                   char *__restrict__ text) {
    const int j = blockIdx.x * TPB + threadIdx.x;
    if (j >= nlines) return;
    long long first;
    int count;
    fmt_line_range(a, line0 + j, first, count);
    char *o = text + off[j];
    for (int i = 0; i < count; i++) {
        int b = fmt_value(a.vals[first + i], a.style, a.prec, a.p10, a.p10_lo, a.p10_n, o);
        if (b < 0) {
            const long long s = fmt_host_slot(a, first + i);
            b = (int)(a.host_off[s + 1] - a.host_off[s]);
            for (int k = 0; k < b; k++) o[k] = a.host_txt[a.host_off[s] + k];
        }
        o += b;
    }
    *o = '\n';
}
