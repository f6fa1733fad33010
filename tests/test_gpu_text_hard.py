"""GPU tests of the text readers at the inputs where they can go wrong (tests/text_vectors.py): the fast-path
boundary from both sides, the tokens numpy refuses, tokens on thread-chunk, workgroup and scan-chunk boundaries, a
text large enough for two scan levels, and more host tokens than the first host list holds.  Every test runs through
xb_parse_density_text and xb_parse_cube_text; the reference for every value is numpy's own string -> float64
(text_vectors.numpy_values), never the oracle and never the library."""
import numpy as np
import pytest

import text_vectors as tv
from pybader_amd import _lib, io_cube

pytestmark = pytest.mark.gpu

DIVISOR = 3.25
SCALE = io_cube.ang_to_bohr ** 3
# (reader, nval, pick): the CHGCAR call, the cube call with one value per voxel and with three, each pick
READERS = [('chgcar', 1, 0), ('cube', 1, 0), ('cube', 3, 0), ('cube', 3, 1), ('cube', 3, 2)]
BOTH = [('chgcar', 1, 0), ('cube', 1, 0)]


def ids(r):
    return '%s-nval%d-pick%d' % r


@pytest.fixture(scope='module')
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def grid_for(n_tokens, nval):
    """the largest (nx, 3, 3) grid that n_tokens fill"""
    nx = n_tokens // (9 * nval)
    assert nx >= 3, n_tokens
    return (nx, 3, 3)


def parse(ctx, reader, text, shape, accumulate=False, scale=SCALE):
    kind, nval, pick = reader
    ctx.set_grid(shape, np.zeros(27), np.zeros(9))
    if kind == 'chgcar':
        return ctx.parse_density_text(text, DIVISOR)
    return ctx.parse_cube_text(text, scale, nval, pick, accumulate=accumulate)


def used(reader, seq, shape):
    """the tokens (or values) of `seq` that the reader takes for a grid of `shape`, in file order"""
    kind, nval, pick = reader
    return seq[:int(np.prod(shape)) * nval][pick::nval]


def expected(reader, vals, shape):
    """numpy's values as the reader stores them: Fortran order over the divisor, or C order times the scale"""
    v = np.asarray(used(reader, vals, shape))
    with np.errstate(over='ignore'):                                     # (the largest double times the scale)
        return v.reshape(shape, order='F') / DIVISOR if reader[0] == 'chgcar' else v.reshape(shape) * SCALE


def check(ctx, reader, text, toks, vals=None, n_host=None):
    """parse `text`, whose tokens are `toks`, and compare the resident density with numpy's conversion of them"""
    shape = grid_for(len(toks), reader[1])
    vals = tv.numpy_values(toks) if vals is None else vals
    n_tokens, got_host = parse(ctx, reader, text, shape)
    assert n_tokens == len(toks)
    wrong = []                                                           # both findings in one report
    try:
        tv.assert_same_values(ctx.download_density(), expected(reader, vals, shape))
    except AssertionError as e:
        wrong.append('values differ from numpy: %s' % e)
    if n_host is not None and got_host != n_host:
        wrong.append('n_host %d, the tokens outside the fast path are %d' % (got_host, n_host))
    assert not wrong, wrong


# ---- values ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def vectors():
    toks = tv.all_accepted()
    toks += toks[:-len(toks) % 27]                                       # a whole grid for nval 1 and nval 3
    text = '\n'.join(' '.join(toks[k:k + 5]) for k in range(0, len(toks), 5)).encode()
    return text, toks, tv.numpy_values(toks), np.array([tv.on_device(t) for t in toks])


@pytest.mark.parametrize('reader', READERS, ids=ids)
def test_values_equal_numpy_and_the_host_takes_exactly_the_rest(ctx, vectors, reader):
    """every accepted vector in one text: bit patterns as numpy's, and n_host == the used tokens outside the four
    fast-path bounds -- a bound moved outwards gives wrong bits and a smaller n_host, moved inwards a larger one"""
    text, toks, vals, dev = vectors
    shape = grid_for(len(toks), reader[1])
    n_host = int((~used(reader, dev, shape)).sum())
    assert 0 < n_host < used(reader, dev, shape).size
    print('tokens', len(toks), 'used', used(reader, dev, shape).size, 'host', n_host)
    check(ctx, reader, text, toks, vals, n_host)


# ---- refusals ---------------------------------------------------------------------------------------------------------
def with_token(toks, at, token):
    return ' '.join(toks[:at] + [token] + toks[at + 1:]).encode()


@pytest.mark.parametrize('reader', [('chgcar', 1, 0), ('cube', 1, 0), ('cube', 3, 1)], ids=ids)
def test_what_numpy_refuses_is_refused(ctx, reader):
    """one text per refused token, at a used index and at the last used one: XB_E_ARG; after the grid's last number
    (and, with nval 3, at an index the pick does not take) it is ignored; a good parse follows every refusal"""
    nval, pick = reader[1:]
    shape = (3, 3, 3)
    toks = [tv.seam_token(i) for i in range(27 * nval)]
    vals = tv.numpy_values(toks)
    good = ' '.join(toks).encode()
    last = 27 * nval - nval + pick
    for token in tv.REFUSED + tv.DIVERGENT:
        for at in (4 * nval + pick, last):
            with pytest.raises(_lib.BaderHipError) as e:
                parse(ctx, reader, with_token(toks, at, token), shape)
            assert e.value.code == _lib.XB_E_ARG, (token, at, str(e.value))
            n_tokens, n_host = parse(ctx, reader, good, shape)
            assert (n_tokens, n_host) == (27 * nval, 0)
            tv.assert_same_values(ctx.download_density(), expected(reader, vals, shape))
        ignored = [good + b' ' + token.encode()]
        if nval > 1:
            ignored.append(with_token(toks, 4 * nval + (pick + 1) % nval, token))
        for text in ignored:
            parse(ctx, reader, b'0 ' * (27 * nval), shape)
            n_tokens, n_host = parse(ctx, reader, text, shape)
            assert n_host == 0 and n_tokens == 27 * nval + (text is ignored[0])
            tv.assert_same_values(ctx.download_density(), expected(reader, vals, shape))


@pytest.mark.parametrize('reader', READERS, ids=ids)
def test_exact_count_one_more_and_one_fewer(ctx, reader):
    """exactly the grid's count of tokens; one more, garbage, which is ignored; one fewer: XB_E_SHORT, and the density
    that was resident downloads bit-unchanged (io_vasp.read retries with a longer text on that code)"""
    nval = reader[1]
    shape = (4, 3, 5)
    n = 60 * nval
    toks = [tv.seam_token(100 + i) for i in range(n)]
    vals = tv.numpy_values(toks)
    for text, count in ((' '.join(toks).encode(), n), ('\n'.join(toks + ['0x1A']).encode(), n + 1),
                        (' '.join(toks + ['augmentation']).encode() + b'\n', n + 1)):
        parse(ctx, reader, b'0 ' * n, shape)
        assert parse(ctx, reader, text, shape) == (count, 0)
        tv.assert_same_values(ctx.download_density(), expected(reader, vals, shape))
    before = ctx.download_density()
    for short in (' '.join(toks[:-1]).encode(), ' '.join(toks[:-1]).encode() + b' \n\t ', b' '):
        with pytest.raises(_lib.BaderHipError) as e:
            parse(ctx, reader, short, shape, accumulate=True)
        assert e.value.code == _lib.XB_E_SHORT
        assert np.array_equal(tv.bits(ctx.download_density()), tv.bits(before))


# ---- seams ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('reader', BOTH + [('cube', 3, 2)], ids=ids)
def test_tokens_on_workgroup_and_thread_chunk_boundaries(ctx, reader):
    """an 18-byte token started at byte B - k for k = 0 .. 19 around workgroup boundaries B = 4096 b, b in {1, 2}, and
    thread-chunk boundaries B = 16 j: the blank the last byte before B, the token's first byte the first after B,
    the token split at every one of its bytes, its last byte the last before B"""
    wg, tb = tv.WG_BYTES, tv.TXT_BYTES
    for k in range(20):
        starts = [tb * 37 - k, wg - k, wg + tb * 9 - k, 2 * wg - k, 2 * wg + tb * 3 - k]
        text, toks = tv.place(starts, multiple=9 * reader[1], first=k)
        for s in starts:
            assert text[s - 1:s] == b' ' and text[s + 18:s + 19] in (b' ', b'') and b' ' not in text[s:s + 18]
        check(ctx, reader, text, toks, n_host=0)


@pytest.mark.parametrize('reader', BOTH, ids=ids)
def test_last_token_ends_at_the_last_byte(ctx, reader):
    """text lengths 16 j - 1, 16 j, 16 j + 1 and exactly one workgroup, no trailing blank"""
    tb = tv.TXT_BYTES
    for length in (tb * 40 - 1, tb * 40, tb * 40 + 1, tv.WG_BYTES - 1, tv.WG_BYTES, tv.WG_BYTES + 1, 2 * tv.WG_BYTES):
        text, toks = tv.place([length - 18], first=length)
        assert len(text) == length and text[-1:] != b' '
        check(ctx, reader, text, toks, n_host=0)


@pytest.mark.parametrize('reader', BOTH, ids=ids)
def test_blank_runs_long_tokens_and_every_separator(ctx, reader):
    toks = [tv.seam_token(300 + i) for i in range(54)]
    vals = tv.numpy_values(toks)
    # 9000 blanks: two workgroups hold no token
    for run in (b' ' * 9000, b'\n' * 9000, b' \t\r\n\v\f' * 1500):
        text = ' '.join(toks[:20]).encode() + run + ' '.join(toks[20:]).encode() + run
        check(ctx, reader, text, toks, vals, n_host=0)
    # a token directly after each separator, and the separators the library knows are the ones Python's split knows
    seps = ['\t', '\r\n', '\v', '\f', '\n', ' ', '\r', ' \t\n\v\f\r ']
    text = ''.join(seps[i % len(seps)] + t for i, t in enumerate(toks))
    assert text.split() == toks and set(text.encode()) - set(''.join(toks).encode()) == set(tv.BLANKS)
    check(ctx, reader, text.encode(), toks, vals, n_host=0)
    # 5000 leading zeros before 1.5: one thread reads across a workgroup boundary; the device converts it itself
    long_toks = toks[:30] + ['0' * 5000 + '1.5'] + toks[31:45] + ['-' + '0' * 5000 + '.25E+01'] + toks[46:]
    assert tv.on_device(long_toks[30]) and tv.numpy_values(long_toks)[30] == 1.5
    check(ctx, reader, ' '.join(long_toks).encode(), long_toks, n_host=0)
    # and one the host converts: 19 significant digits behind the zeros
    long_toks[30] = '0' * 5000 + '1.234567890123456789'
    check(ctx, reader, ' '.join(long_toks).encode(), long_toks, n_host=1)


# ---- two scan levels ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def large_text():
    """18 MB, three first-level scan chunks: 400 dense runs of 300 .. 700 tokens 45 000 bytes apart (a workgroup holds
    up to 215 tokens, most hold none), one token astride byte 8 MiB and one astride byte 16 MiB"""
    pitch, runs = 45000, 400
    groups = [(g * pitch, 300 + g * 37 % 401) for g in range(runs)]
    groups += [(tv.SCAN_BYTES - 7 - 19 * 250, 500), (2 * tv.SCAN_BYTES - 9 - 19 * 250, 500)]
    offsets = np.sort(np.concatenate([o + 19 * np.arange(c) for o, c in groups]))
    assert np.diff(offsets).min() >= 19 and runs * pitch >= 17 << 20
    for seam in (tv.SCAN_BYTES, 2 * tv.SCAN_BYTES):
        assert ((offsets < seam) & (offsets + 18 > seam)).sum() == 1
    rng = np.random.default_rng(8)
    n = offsets.size
    vals = (1 + 9 * rng.random(n)) * 10.0 ** rng.integers(-30, 31, n) * rng.choice([-1.0, 1.0], n)
    toks = ['%+.11E' % v for v in vals]                                  # 18 bytes each; exponents below -11: host
    buf = np.full(runs * pitch, ord(' '), np.uint8)
    buf[offsets[:, None] + np.arange(18)] = np.frombuffer(''.join(toks).encode(), np.uint8).reshape(n, 18)
    assert offsets[-1] > 2 * tv.SCAN_BYTES + tv.WG_BYTES
    return buf, toks, tv.numpy_values(toks), np.array([tv.on_device(t) for t in toks])


@pytest.mark.parametrize('reader', BOTH + [('cube', 3, 1)], ids=ids)
def test_text_of_three_scan_chunks(ctx, large_text, reader):
    text, toks, vals, dev = large_text
    assert text.size >= 17 << 20 and 190000 <= len(toks) <= 210000
    shape = (len(toks) // (81 * reader[1]), 9, 9)
    n_host = int((~used(reader, dev, shape)).sum())
    assert 0 < n_host < len(toks) // reader[1]
    assert parse(ctx, reader, text, shape) == (len(toks), n_host)
    tv.assert_same_values(ctx.download_density(), expected(reader, vals, shape))


# ---- more host tokens than the first list holds ----------------------------------------------------------------------
CAP_SHAPE = (128, 128, 65)


@pytest.fixture(scope='module')
def seventeen_digits():
    """two texts of 128 x 128 x 65 tokens written '%.17E' (18 significant digits: the host converts every one) and a
    third, the first with every 100th token written '%.11E' (the device converts those)"""
    n = int(np.prod(CAP_SHAPE))
    assert n > tv.TODO_FIRST and n - len(range(0, n, 100)) > tv.TODO_FIRST
    rng = np.random.default_rng(17)
    out = []
    for k in range(2):
        v = rng.lognormal(0.0, 4.0, n) * rng.choice([-1.0, 1.0], n)
        toks = ['%.17E' % x for x in v]
        out.append(('\n'.join(toks).encode(), tv.numpy_values(toks)))
        if k == 0:
            short, vals = ['%.11E' % x for x in v[::100]], out[0][1].copy()
            toks[::100], vals[::100] = short, tv.numpy_values(short)
            third = ('\n'.join(toks).encode(), vals)
    return out + [third]


def test_chgcar_of_17_digit_tokens(ctx, seventeen_digits):
    text, vals = seventeen_digits[0]
    n = vals.size
    assert parse(ctx, ('chgcar', 1, 0), text, CAP_SHAPE) == (n, n)
    tv.assert_same_values(ctx.download_density(), vals.reshape(CAP_SHAPE, order='F') / DIVISOR)


def test_cube_chain_of_17_digit_tokens(ctx, seventeen_digits):
    """a store call and an accumulate call: (a + b) * s in float64; then a third, accumulated, of which the device
    converts every 100th value in the pass whose host list overflows: every value is added once"""
    (ta, a), (tb, b), (tc, c) = seventeen_digits
    n, cube = a.size, ('cube', 1, 0)
    assert parse(ctx, cube, ta, CAP_SHAPE, scale=1.0) == (n, n)
    assert parse(ctx, cube, tb, CAP_SHAPE, accumulate=True, scale=SCALE) == (n, n)
    ab = (a + b) * SCALE
    tv.assert_same_values(ctx.download_density(), ab.reshape(CAP_SHAPE))
    assert parse(ctx, cube, tc, CAP_SHAPE, accumulate=True, scale=0.5) == (n, n - len(range(0, n, 100)))
    tv.assert_same_values(ctx.download_density(), ((ab + c) * 0.5).reshape(CAP_SHAPE))
