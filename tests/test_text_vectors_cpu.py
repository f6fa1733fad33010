"""CPU tests of the text readers' adversarial vectors (tests/text_vectors.py): the vectors themselves against numpy,
the oracle's parser against numpy on them, `on_device` against the classes it must split, and the tiling and
fast-path constants the seam tests hard-code against the sources they were read from."""
import os
import re

import numpy as np
import pytest

import oracle
import text_vectors as tv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'pybader_amd', 'csrc')


@pytest.fixture(scope='module')
def classes():
    return tv.accepted_classes()


def test_every_class_is_non_empty(classes):
    for name, toks in classes.items():
        assert len(toks) > 0, name
    assert len(tv.REFUSED) > 0 and len(tv.DIVERGENT) > 0
    assert len(classes['boundary']) == 3 * len(tv.E10_RANGE) * (len(tv.FIXED_MANTISSAS) + tv.N_SEEDED_MANTISSAS)
    assert tv.N_SEEDED_MANTISSAS >= 2000 and list(tv.E10_RANGE) == list(range(-25, 26))
    for t in tv.all_accepted() + tv.REFUSED + tv.DIVERGENT:
        assert t and not any(ch.isspace() for ch in t), t          # one token each


def test_numpy_accepts_and_refuses_as_labelled(classes):
    for name, toks in classes.items():
        tv.numpy_values(toks)                                       # raises if numpy refuses one
    tv.numpy_values(tv.DIVERGENT)
    for t in tv.REFUSED:
        with pytest.raises(ValueError):
            tv.numpy_values([t])
    want = tv.numpy_values(['-0', '-0.0', '-0E5000', '0E999', '1e400', '-1e-400'])
    assert list(np.signbit(want)) == [True, True, True, False, False, True] and np.isinf(want[4])


def test_boundary_reaches_every_e10_three_ways_on_both_sides(classes):
    """the boundary class holds device and host tokens at |e10| = 22 / 23 and at 2^53 - 1 / 2^53, every exponent
    spelling, and its values do not depend on the way e10 is reached"""
    toks = classes['boundary']
    vals = tv.numpy_values(toks)
    assert np.array_equal(tv.bits(np.abs(vals[0::3])), tv.bits(np.abs(vals[1::3])))
    assert np.array_equal(tv.bits(np.abs(vals[0::3])), tv.bits(np.abs(vals[2::3])))
    dev = np.array([tv.on_device(t) for t in toks])
    per = 3 * len(tv.E10_RANGE)
    for k, m in enumerate(tv.FIXED_MANTISSAS):                      # the exponent-alone spelling of the fixed mantissas
        for j, e10 in enumerate(tv.E10_RANGE):
            t = toks[k * per + 3 * j]
            plain = m < tv.MANTISSA_LIMIT and abs(e10) <= tv.MAX_E10
            wide = re.search(r'[eE][+-]?\d{5,}$', t) is not None
            assert dev[k * per + 3 * j] == (plain and not wide), t
    assert 0.3 < dev.mean() < 0.9
    for pat in (r'E\d+$', r'e\d+$', r'E\+\d$', r'E\+\d\d$', r'E\+\d{4}$', r'E\+\d{5}$', r'e-\d{5}$', r'^\+', r'^-', r'^\d'):
        assert any(re.search(pat, t) for t in toks), pat


def test_19_digit_tokens_where_the_last_digit_matters(classes):
    toks = classes['digits_18_19']
    pairs = list(zip(toks[0:240:2], toks[1:240:2]))
    changed = [(a, b) for a, b in pairs if float(a) != float(b)]
    assert len(changed) >= 100
    for a, b in pairs:
        assert len(re.sub(r'\D', '', a.split('E')[0])) == 19 and len(re.sub(r'\D', '', b.split('E')[0])) == 18
        assert not tv.on_device(a) and not tv.on_device(b)
    assert tv.on_device('0' * 21 + '1.2345678901') and not tv.on_device('15' + '0' * 17)
    assert not tv.on_device('18446744073709551617')


def test_on_device_on_the_named_cases():
    for t in ['1', '-0', '0E999', '0.000E-9999', '-0E5000', '.5', '5.', '1.e5', '9007199254740991E22', '1E-22',
              '9007199254740991', '0.' + '0' * 6 + '9007199254740991']:
        assert tv.on_device(t), t
    for t in ['9007199254740992', '9007199254740991E23', '1E23', '1E-23', '1E+00005', '0E99999', 'nan', 'inf',
              '0.' + '0' * 7 + '9007199254740991', '1234567890123456789', '١٢'] + tv.REFUSED + tv.DIVERGENT:
        assert not tv.on_device(t), t


def test_oracle_parser_equals_numpy_and_refuses_what_numpy_refuses(classes):
    toks = tv.all_accepted() + ['0' * 5000 + '1.5']
    want = tv.numpy_values(toks)
    text = '\n'.join(' '.join(toks[k:k + 5]) for k in range(0, len(toks), 5)).encode()
    got = oracle.parse_density_text(text, (len(toks), 1, 1), 1.0)
    tv.assert_same_values(got, want)
    got = oracle.parse_density_text(text, (len(toks), 1, 1), 3.25)
    tv.assert_same_values(got, want / 3.25)
    for t in tv.REFUSED + tv.DIVERGENT:
        with pytest.raises(ValueError):
            oracle.parse_density_text(('1.0 ' + t + ' 2.0').encode(), (3, 1, 1), 1.0)
        a = oracle.parse_density_text(('1.0 2.0 ' + t).encode(), (2, 1, 1), 1.0)     # after the grid's last number
        assert a[0, 0, 0] == 1.0 and a[1, 0, 0] == 2.0


def source(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def one(pattern, text):
    found = re.findall(pattern, text)
    assert len(found) == 1, (pattern, found)
    return found[0]


def test_hard_coded_constants_match_the_sources():
    k_text, k_common, host = source('k_text.h'), source('k_common.h'), source('host_context.h')
    assert int(one(r'#define\s+TXT_BYTES\s+(\d+)', k_text)) == tv.TXT_BYTES == 16
    assert int(one(r'#define\s+TPB\s+(\d+)', k_common)) == tv.TPB == 256
    assert tv.WG_BYTES == 4096 and tv.SCAN_BYTES == 8 << 20
    parse = k_text[k_text.index('bool txt_parse('):k_text.index('struct TxtFortran')]
    assert int(one(r'\+\+nd\s*>\s*(\d+)', parse)) == tv.MAX_DIGITS == 18
    assert int(one(r'\+\+ed\s*>\s*(\d+)', parse)) == tv.MAX_EXP_DIGITS == 4
    assert 1 << int(one(r'm\s*<\s*\(1ull\s*<<\s*(\d+)\)', parse)) == tv.MANTISSA_LIMIT == 1 << 53
    lo, hi = one(r'e10\s*>=\s*(-?\d+)\s*&&\s*e10\s*<=\s*(-?\d+)', parse)
    assert (int(lo), int(hi)) == (-tv.MAX_E10, tv.MAX_E10) == (-22, 22)
    assert int(one(r'P10\[(\d+)\]\s*=', host)) == tv.MAX_E10 + 1
    # the scan: k_scan_2048 takes 8 counts per thread, device_scan cuts its input into as many per block
    scan = k_text[k_text.index('void k_scan_2048('):k_text.index('void k_scan_add(')]
    per_thread = int(one(r'threadIdx\.x\)\s*\*\s*(\d+)', scan))
    assert per_thread * tv.TPB == tv.SCAN_CHUNK == 2048
    dev_scan = host[host.index('static int device_scan('):host.index('enum { TXT_TODO_FIRST')]
    assert one(r'nb\s*=\s*\(n\s*\+\s*(\d+)\)\s*/\s*(\d+)', dev_scan) == ('2047', '2048')
    assert 1 << int(one(r'TXT_TODO_FIRST\s*=\s*1\s*<<\s*(\d+)', host)) == tv.TODO_FIRST
    # the library's blanks are the bytes the texts of the seam tests separate tokens with
    assert one(r"ch == ' ' \|\| \(ch >= (\d+) && ch <= (\d+)\)", k_text) == ('9', '13')
    assert sorted(tv.BLANKS) == [9, 10, 11, 12, 13, 32]
