// fmt_core.h -- float64 -> text, the digit core shared by the device formatter (k_format.h) and a host build of the
// same code (tests/test_writer_cpu.py compiles this header alone with g++ and checks it against Python's own format).
// Plain C++ only: no HIP intrinsics, no globals, no tables -- every function is __host__ __device__ under hipcc.
//
// Two styles (the reference's writers, utils.py:40-94):
//   E   python_format: ' ' + format(v, '.{p}E') (align ' ': format(v, ' .{p}E')) -- CPython's correctly rounded
//       conversion, round half to even on exact ties.  Here: exact integer arithmetic.  |v| = m 2^e, the digits are
//       round(m 2^e / 10^k) with k = X - p, X = floor(log10 |v|), computed as one 128-bit quotient + remainder.  Values
//       whose numerator or denominator would not fit 127 bits (roughly |v| < 1e-20 or > 1e35), subnormals, nan and inf
//       are left to the host (return -1).
//   F   fortran_format: numpy's float64 steps restated -- exp = floor(log10|a|) + 1, value = int64(0.5 + |a| / 10.0**(exp
//       - p)), the digits str(value)[:p], ' 0.' / ' -.', 'E+' / 'E-', |exp| zero padded to 2 characters or its first 2
//       characters.  10.0**k comes from a table the host filled with np.power(10.0, k).  log10 is not correctly rounded
//       (numpy's may be SVML or libm): a value whose log10 lies within 1e-13 (relative) of an integer goes to the host,
//       every other value has the same floor(log10) under any faithful log10.  The division and the add are single IEEE
//       operations (the library is built with -ffp-contract=off).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIP__) || defined(__CUDACC__)
#define FMT_HD __host__ __device__ inline
#else
#define FMT_HD inline
#endif

enum { FMT_STYLE_E = 0, FMT_STYLE_E_SPACE = 1, FMT_STYLE_F = 2 };
#define FMT_MAX_VALUE_BYTES(prec) ((prec) + 10)   // the widest text of one value, host fallbacks included

typedef unsigned __int128 fmt_u128;

FMT_HD int fmt_bitlen128(fmt_u128 x) {
    const unsigned long long hi = (unsigned long long)(x >> 64), lo = (unsigned long long)x;
    if (hi) return 128 - __builtin_clzll(hi);
    return lo ? 64 - __builtin_clzll(lo) : 0;
}
FMT_HD fmt_u128 fmt_pow5(int j) {   // 5^j, j <= 55
    fmt_u128 r = 1, b = 5;
    for (; j; j >>= 1, b *= b)
        if (j & 1) r *= b;
    return r;
}
FMT_HD unsigned long long fmt_pow10u(int j) {   // 10^j, j <= 19
    unsigned long long r = 1;
    while (j-- > 0) r *= 10ull;
    return r;
}
// upper bound of the bit length of 5^j: floor(j log2 5) + 1 <= j * 2.32193 + 1
FMT_HD int fmt_bitlen_pow5(int j) { return (j * 232193) / 100000 + 1; }

// q = floor(m 2^e / 10^k), rem / den its fraction (0 <= rem < den), exactly.  false: does not fit 127 bits.
FMT_HD bool fmt_scaled(unsigned long long m, int e, int k, unsigned long long &q, fmt_u128 &rem, fmt_u128 &den) {
    const int a2 = e - k, a5 = -k;
    fmt_u128 num = m, d = 1;
    int shift = 0;   // den = d << shift
    if (a5 >= 0) {
        if (a5 > 55 || fmt_bitlen128(num) + fmt_bitlen_pow5(a5) > 127) return false;
        num *= fmt_pow5(a5);
    } else {
        if (-a5 > 55 || fmt_bitlen_pow5(-a5) > 126) return false;
        d = fmt_pow5(-a5);
    }
    if (a2 >= 0) {
        if (fmt_bitlen128(num) + a2 > 127) return false;
        num <<= a2;
    } else {
        if (fmt_bitlen128(d) + (-a2) > 126) return false;
        shift = -a2;
    }
    fmt_u128 qq;
    if (d == 1) {   // a power of two: a shift
        qq = shift >= 128 ? 0 : num >> shift;
        rem = shift >= 128 ? num : num & ((((fmt_u128)1) << shift) - 1);
    } else {
        d <<= shift;
        qq = num / d;
        rem = num - qq * d;
    }
    if (qq >> 63) return false;
    q = (unsigned long long)qq;
    den = d == 1 ? (((fmt_u128)1) << shift) : d;
    return true;
}

// |v| (finite, normal, nonzero) to prec+1 significant decimal digits, round half to even: |v| ~ digits 10^(exp10 - prec)
FMT_HD bool fmt_e_digits(double v, int prec, unsigned long long &digits, int &exp10) {
    unsigned long long bits;
    memcpy(&bits, &v, sizeof bits);
    const int be = (int)((bits >> 52) & 0x7ff);
    if (be == 0 || be == 0x7ff) return false;   // zero / subnormal, inf / nan
    unsigned long long m = (bits & ((1ull << 52) - 1)) | (1ull << 52);
    int e = be - 1075;
    const int p2 = e + 52;                       // 2^p2 <= |v| < 2^(p2+1)
    const int tz = __builtin_ctzll(m);
    m >>= tz;
    e += tz;
    int X = (p2 * 78913) >> 18;                  // floor(p2 log10 2): X or X - 1
    const unsigned long long lo = fmt_pow10u(prec), hi = fmt_pow10u(prec + 1);
    unsigned long long q = 0;
    fmt_u128 rem = 0, den = 1;
    for (int it = 0;; it++) {
        if (it == 3 || !fmt_scaled(m, e, X - prec, q, rem, den)) return false;
        if (q >= hi) X++;
        else if (q < lo) X--;
        else break;
    }
    const fmt_u128 half_up = den - rem;          // rem vs den - rem: rem > den / 2, == on a tie
    if (rem > half_up || (rem == half_up && (q & 1))) q++;
    if (q == hi) { q = lo; X++; }                // 9.99..95 -> 1.00..0E+(X+1)
    digits = q;
    exp10 = X;
    return true;
}

FMT_HD int fmt_put_uint(char *out, unsigned long long x) {   // decimal digits of x; returns their count
    char t[20];
    int n = 0;
    do { t[n++] = (char)('0' + x % 10); x /= 10; } while (x);
    if (out)
        for (int i = 0; i < n; i++) out[i] = t[n - 1 - i];
    return n;
}

// ' ' + format(v, '.{prec}E') (space: format(v, ' .{prec}E')).  Returns the length, -1 when the host must format v.
// out == nullptr: length only.
FMT_HD int fmt_e(double v, int prec, bool space, char *out) {
    const bool neg = std::signbit(v);
    unsigned long long digits = 0;
    int X = 0;
    if (v == 0.) { digits = 0; X = 0; }
    else if (!fmt_e_digits(v, prec, digits, X)) return -1;
    int n = 0;
    char buf[48];
    char *o = out ? out : buf;
    o[n++] = ' ';
    if (neg) o[n++] = '-';
    else if (space) o[n++] = ' ';
    char d[24];
    if (digits == 0)
        for (int i = 0; i <= prec; i++) d[i] = '0';
    else
        fmt_put_uint(d, digits);   // prec + 1 digits
    o[n++] = d[0];
    o[n++] = '.';
    for (int i = 1; i <= prec; i++) o[n++] = d[i];
    o[n++] = 'E';
    o[n++] = X < 0 ? '-' : '+';
    const int ax = X < 0 ? -X : X;
    if (ax < 10) o[n++] = '0';
    n += fmt_put_uint(o + n, (unsigned long long)ax);
    return n;
}

// fortran_format of one value.  p10[k - p10_lo] = np.power(10.0, k) for p10_lo <= k < p10_lo + p10_n.
FMT_HD int fmt_f(double v, int prec, const double *p10, int p10_lo, int p10_n, char *out) {
    char buf[48];
    char *o = out ? out : buf;
    int n = 0;
    if (v == 0.) {                                    // a != 0 false (also -0.0): ' 0.' + '0' * prec + 'E+00'
        o[n++] = ' '; o[n++] = '0'; o[n++] = '.';
        for (int i = 0; i < prec; i++) o[n++] = '0';
        o[n++] = 'E'; o[n++] = '+'; o[n++] = '0'; o[n++] = '0';
        return n;
    }
    const double a = std::fabs(v);
    if (!(a >= 2.2250738585072014e-308) || !(a <= 1.7976931348623157e308)) return -1;   // subnormal, nan, inf
    const double l = std::log10(a);
    const double r = std::rint(l);
    if (std::fabs(l - r) <= 1e-13 * std::fmax(1.0, std::fabs(l))) return -1;          // floor(log10) not certain
    const int ex = (int)std::floor(l) + 1;
    const int k = ex - prec;
    if (k < p10_lo || k >= p10_lo + p10_n) return -1;
    const double q = a / p10[k - p10_lo];
    const double s = 0.5 + q;
    if (!(s < 9.2e18)) return -1;
    const long long value = (long long)s;            // numpy's float64 -> int64 cast: truncation
    o[n++] = ' ';                                    // (nothing is written before the value is known to be ours)
    o[n++] = v < 0 ? '-' : '0';
    o[n++] = '.';
    char d[24];
    const int nd = fmt_put_uint(d, (unsigned long long)value);
    for (int i = 0; i < nd && i < prec; i++) o[n++] = d[i];   // '<U{prec}': the first prec characters
    o[n++] = 'E';
    o[n++] = ex < 0 ? '-' : '+';
    const int ax = ex < 0 ? -ex : ex;
    if (ax < 10) o[n++] = '0';
    char t[8];
    const int nt = fmt_put_uint(t, (unsigned long long)ax);
    for (int i = 0; i < nt && i < 2; i++) o[n++] = t[i];      // '<U2'
    return n;
}

FMT_HD int fmt_value(double v, int style, int prec, const double *p10, int p10_lo, int p10_n, char *out) {
    if (style == FMT_STYLE_F) return fmt_f(v, prec, p10, p10_lo, p10_n, out);
    return fmt_e(v, prec, style == FMT_STYLE_E_SPACE, out);
}
