"""Adversarial vectors for the text readers (xb_parse_density_text / xb_parse_cube_text), shared by
test_text_vectors_cpu.py and test_gpu_text_hard.py.  Deterministic.  The reference for every value is numpy's own
string -> float64, assigned as the reference's readers assign it (`a[:] = tokens`): never the oracle, never the
library.  `on_device` restates the four bounds of the device's exact fast path (txt_parse in csrc/k_text.h)."""
import numpy as np

# the constants the tests aim at; test_text_vectors_cpu.py reads them back from the sources
TXT_BYTES = 16            # bytes of text per thread (k_text.h)
TPB = 256                 # threads per workgroup (k_common.h)
WG_BYTES = TXT_BYTES * TPB   # 4096 bytes of text per workgroup
SCAN_CHUNK = 2048         # workgroup counts per scan block (k_scan_2048, device_scan)
SCAN_BYTES = SCAN_CHUNK * WG_BYTES   # 8 MiB of text per first-level scan chunk
MAX_E10 = 22              # |decimal exponent| of the one-operation path
MAX_DIGITS = 18           # significant digits kept in 64 bits
MAX_EXP_DIGITS = 4        # digits of a written exponent
MANTISSA_LIMIT = 1 << 53  # mantissas below it are exact doubles
TODO_FIRST = 1 << 20      # entries of the first host-token list (host_context.h)

BLANKS = b' \t\n\v\f\r'


def on_device(token):
    """True when the device converts `token` itself: a well-formed decimal with at most MAX_DIGITS significant
    digits, at most MAX_EXP_DIGITS exponent digits, and either a zero mantissa or a mantissa below MANTISSA_LIMIT
    with |e10| <= MAX_E10, e10 = written exponent - digits after the point.  Everything else goes to the host."""
    b = token.encode() if isinstance(token, str) else bytes(token)
    i = 1 if b[:1] in (b'+', b'-') else 0
    m = digits = frac = nd = 0
    point = False
    while i < len(b):
        ch = b[i:i + 1]
        if ch.isdigit():
            digits += 1
            if m or ch != b'0':
                nd += 1
                if nd > MAX_DIGITS:
                    return False
                m = m * 10 + int(ch)
            frac += point
        elif ch == b'.' and not point:
            point = True
        else:
            break
        i += 1
    if not digits:
        return False
    ex = 0
    if b[i:i + 1] in (b'e', b'E'):
        i += 1
        eneg = b[i:i + 1] == b'-'
        i += b[i:i + 1] in (b'+', b'-')
        j = i
        while b[j:j + 1].isdigit():
            j += 1
        if j == i or j - i > MAX_EXP_DIGITS:
            return False
        ex = -int(b[i:j]) if eneg else int(b[i:j])
        i = j
    if i < len(b):
        return False
    return m == 0 or (m < MANTISSA_LIMIT and abs(ex - frac) <= MAX_E10)


def numpy_values(tokens):
    """numpy's string -> float64 as the reference's readers do it; raises ValueError where numpy refuses"""
    a = np.zeros(len(tokens), dtype=np.float64)
    a[:] = list(tokens)
    return a


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_same_values(got, want):
    """finite and infinite values by bit pattern (signed zeros included), NaNs by position only"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    assert got.shape == want.shape
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    bad = np.flatnonzero((bits(got) != bits(want)) & ~nan)
    assert bad.size == 0, (bad.size, bad[:5], got[bad[:5]], want[bad[:5]])


# ---- the fast-path boundary -------------------------------------------------------------------------------------
FIXED_MANTISSAS = [1, (1 << 53) - 2, (1 << 53) - 1, 1 << 53, (1 << 53) + 1, 10 ** 15, 10 ** 16 - 1]
N_SEEDED_MANTISSAS = 2000
E10_RANGE = range(-25, 26)


def _exponent(e, k):
    """`e` written the k-th way: E or e; explicit +, - or no sign; widths E5, E+05, E+0005, E+00005"""
    letter = 'Ee'[k & 1]
    width = (0, 2, 4, 5)[(k >> 1) & 3]
    if e < 0:
        return '%s-%0*d' % (letter, max(width, 1), -e)
    if width == 0 and (k >> 3) & 1:
        return '%s%d' % (letter, e)
    if width == 0:
        return '%s+%d' % (letter, e)
    return '%s+%0*d' % (letter, width, e)


def _by_point(d, e10):
    """the digits `d` times 10**e10 with no exponent: the point moved through the digits, or zeros appended"""
    if e10 >= 0:
        return d + '0' * e10                      # (trailing zeros are significant digits to the parser)
    if -e10 < len(d):
        return d[:e10] + '.' + d[e10:]
    return '0.' + '0' * (-e10 - len(d)) + d


def boundary_tokens():
    rng = np.random.default_rng(20240531)
    seeded = rng.integers(10 ** 15, 1 << 53, N_SEEDED_MANTISSAS)          # 16 digits, below 2^53
    out, k = [], 0
    for m in FIXED_MANTISSAS + [int(x) for x in seeded]:
        d = str(m)
        for e10 in E10_RANGE:
            sign = ('', '-', '+')[k % 3]
            out.append(sign + d + _exponent(e10, k))                     # the exponent alone
            out.append(sign + _by_point(d, e10))                         # the point alone
            s = 1 + k % len(d)                                           # both: point moved s places, exponent e10 + s
            out.append(sign + (d[:-s] + '.' + d[-s:] if s < len(d) else '.' + d) + _exponent(e10 + s, k // 3))
            k += 1
    return out


def digits_18_19_tokens(n_changed=120):
    """19-digit tokens (host: more than MAX_DIGITS) next to their 18-digit heads (host: mantissa >= 2^53).  The first
    2 * n_changed pair a 19-digit token with its head where dropping the last digit changes the double."""
    rng = np.random.default_rng(19)
    changed, same = [], []
    while len(changed) < n_changed:
        d = '%d%018d' % (rng.integers(1, 10), rng.integers(0, 10 ** 18))
        e = int(rng.integers(-40, 40))
        full, head = '%s.%sE%+03d' % (d[0], d[1:], e), '%s.%sE%+03d' % (d[0], d[1:18], e)
        (changed if float(full) != float(head) else same).append((full, head))
    out = [t for pair in changed for t in pair] + [t for pair in same[:n_changed] for t in pair]
    # leading zeros are not significant: 21 of them before an 11-digit number stay on the device
    out += ['0' * 21 + '1.2345678901', '-' + '0' * 21 + '12345678901E-05', '0.' + '0' * 21 + '12345678901',
            '0.' + '0' * 11 + '12345678901', '+' + '0' * 21 + '.12345678901e+10']
    # trailing zeros are: they lift a short number past 18 digits
    out += ['15' + '0' * 16, '15' + '0' * 17, '1.5' + '0' * 16, '1.5' + '0' * 17, '-25' + '0' * 17 + 'E-17',
            '125' + '0' * 15 + '.' + '0' * 5]
    # 20 digits and more wrap 64 bits: 2^64 + 1 must not read as 1, nor 2^64 as 0
    out += ['18446744073709551617', '18446744073709551616', '-18446744073709551621E-3', '36893488147419103233',
            '1.8446744073709551617E+19']
    return out


FORMS = ['.5', '5.', '-.5E+01', '1.e5', '+0', '-0', '-0.0', '0E999', '0.000E-9999', '-0E5000',
         '0', '00', '-.0E5', '+5.E-1', '007', '1E0', '1e-0', '0E99999', '12345678901234567E-17']

HARD = ['9007199254740993', '9007199254740993.0000000000000000001',
        '2.2250738585072011e-308', '4.9e-324', '2.4703282292062327e-324', '2.4703282292062328e-324',
        '1.7976931348623158e308', '1.7976931348623159e308', '1e400', '1e-400', '-1e400', '-1e-400',
        'nan', 'NaN', '-nan', 'inf', '-Inf', 'Infinity', '+infinity', 'INF', '+NAN',
        '1E22', '1E23', '1E-22', '1E-23', '8.5E22', '9007199254740991E22', '9007199254740991E23',
        '9007199254740991E-22', '9007199254740991E-23', '1E9999', '1E-9999', '1E10000', '1E-10000']

REFUSED = ['0x1A', '0X1p3', '0x', 'nan(abc)', 'nan()', '1.0D+00', '1e', '1e+', '.', '-', '+', '.E5', '1.2.3', '1,5',
           '--1', '1e5.0', '1E5E5', 'infinit', '1.0x',
           '-0x1A', '+0x1.8p1', 'NAN(1)', '-nan(abc)', 'in', 'infinityy', 'na', '+-1', '1e--5', 'e5', '1_', '_1',
           '0x1A' * 20]

# numpy accepts these (its converter is Python's float()); the library refuses them on purpose: no writer emits them
DIVERGENT = ['1_0', '1_000.5', '1e1_0', '١٢', '１２', '1٠']


def accepted_classes():
    return {'boundary': boundary_tokens(), 'digits_18_19': digits_18_19_tokens(), 'forms': list(FORMS),
            'hard': list(HARD)}


def all_accepted():
    return [t for c in accepted_classes().values() for t in c]


# ---- texts for the seam tests -------------------------------------------------------------------------------------
def seam_token(i):
    """an 18-byte token, `-1.23456789012E-05` with every digit and both signs depending on i; the device converts it"""
    r = np.random.default_rng(1000 + i)
    t = '%s%d.%011dE%s%02d' % ('+-'[i % 2], r.integers(1, 10), r.integers(0, 10 ** 11), '-+'[(i // 2) % 2],
                               r.integers(0, 12))
    assert len(t) == 18 and on_device(t)
    return t


def place(starts, multiple=9, first=0):
    """A text of seam tokens in which a token starts at every byte offset of `starts` (ascending, at least 19
    apart): the room before each is filled with more tokens a blank apart, the rest is blanks.  The first fillers
    are left out (blanks in their place) until the number of tokens is a multiple of `multiple`, so a grid takes
    them all.  The last token ends at the text's last byte.  Returns (text, tokens)."""
    slots, pos = [], 0                                                   # (offset, placed on purpose)
    for s in starts:
        assert s >= pos, (s, pos)
        while pos + 19 <= s:
            slots.append((pos, False))
            pos += 19
        slots.append((s, True))
        pos = s + 19
    drop = [i for i, (_, seam) in enumerate(slots) if not seam][:len(slots) % multiple]
    assert len(drop) == len(slots) % multiple
    slots = [sl for i, sl in enumerate(slots) if i not in drop]
    buf, toks = bytearray(b' ' * (slots[-1][0] + 18)), []
    for i, (o, _) in enumerate(slots):
        toks.append(seam_token(first + i))
        buf[o:o + 18] = toks[-1].encode()
    assert bytes(buf).decode().split() == toks
    return bytes(buf), toks
