"""The cached-state flags of a context and the events that drop them (pybader_amd/csrc/ctx_state.h), compiled alone for the
host with g++: every function applied to a state with every flag valid and to one with every flag invalid changes exactly
the fields its table entry below names, to the values it names, and leaves every other field as it was."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'pybader_amd', 'csrc', 'ctx_state.h')

FIELDS = ['grad_valid', 'grad_nb', 'brick_max_valid', 'buni_valid', 'regions_labels', 'list_valid', 'chg_n', 'has_vacuum',
          'vac_by_tol', 'label_wire', 'labels_zero_pending', 'zero_outside0', 'zero_outside1', 'zero_outside2', 'have_rho',
          'have_labels', 'cp_have', 'iso_have', 'rg_have']
FUNCS = ['drop_table', 'drop_table_and_maxima', 'drop_edge_lists', 'stage_clobbered', 'drop_label_marks',
         'drop_density_results', 'vacuum_marks_unproven', 'density_written', 'density_pointer_out', 'labels_overwritten',
         'labels_patched']

SHIM = '#include "ctx_state.h"\n' + r'''
static void load(CtxState &s, const int *v) {
    int k = 0;
    s.grad_valid = v[k++]; s.grad_nb = v[k++]; s.brick_max_valid = v[k++]; s.buni_valid = v[k++]; s.regions_labels = v[k++];
    s.list_valid = v[k++]; s.chg_n = v[k++]; s.has_vacuum = v[k++]; s.vac_by_tol = v[k++]; s.label_wire = v[k++];
    s.labels_zero_pending = v[k++]; s.zero_outside[0] = v[k++]; s.zero_outside[1] = v[k++]; s.zero_outside[2] = v[k++];
    s.have_rho = v[k++]; s.have_labels = v[k++]; s.cp_have = v[k++]; s.iso_have = v[k++]; s.rg_have = v[k++];
}
static void store(const CtxState &s, int *v) {
    int k = 0;
    v[k++] = s.grad_valid; v[k++] = s.grad_nb; v[k++] = s.brick_max_valid; v[k++] = s.buni_valid; v[k++] = s.regions_labels;
    v[k++] = s.list_valid; v[k++] = s.chg_n; v[k++] = s.has_vacuum; v[k++] = s.vac_by_tol; v[k++] = s.label_wire;
    v[k++] = s.labels_zero_pending; v[k++] = s.zero_outside[0]; v[k++] = s.zero_outside[1]; v[k++] = s.zero_outside[2];
    v[k++] = s.have_rho; v[k++] = s.have_labels; v[k++] = s.cp_have; v[k++] = s.iso_have; v[k++] = s.rg_have;
}
extern "C" int n_fields(void) { return 19; }
extern "C" void defaults(int *v) { store(CtxState{}, v); }
extern "C" int apply(int fn, int wire, int has_vacuum, int marks_kept, int owned_only, int *v) {
    CtxState s;
    load(s, v);
    switch (fn) {
    case -1: break;   // (load and store alone)
    case 0: drop_table(s); break;
    case 1: drop_table_and_maxima(s); break;
    case 2: drop_edge_lists(s); break;
    case 3: stage_clobbered(s); break;
    case 4: drop_label_marks(s); break;
    case 5: drop_density_results(s); break;
    case 6: vacuum_marks_unproven(s); break;
    case 7: density_written(s); break;
    case 8: density_pointer_out(s); break;
    case 9: labels_overwritten(s, wire, has_vacuum != 0); break;
    case 10: labels_patched(s, wire, has_vacuum != 0, marks_kept, owned_only != 0); break;
    default: return -1;
    }
    store(s, v);
    return 0;
}
'''

VALID = dict({f: 1 for f in FIELDS}, chg_n=7, label_wire=2, zero_outside0=1, zero_outside1=2, zero_outside2=3)
INVALID = dict({f: 0 for f in FIELDS}, chg_n=-1, label_wire=4, zero_outside0=-1, zero_outside1=-1, zero_outside2=-1)

TABLE = {f: False for f in ('grad_valid', 'grad_nb')}
TABLE_MAXIMA = dict(TABLE, brick_max_valid=False)
EDGE_LISTS = {'list_valid': False, 'chg_n': -1}
LABEL_MARKS = {'buni_valid': False, 'regions_labels': False}
RESULTS = {'cp_have': False, 'iso_have': False, 'rg_have': False}


def expected(fn, wire, has_vacuum, marks_kept=0, owned_only=False, start=None):
    """the stores of each function: field -> new value (labels_patched: `has_vacuum` says that a written label is negative; its
    stores of has_vacuum and label_wire depend on the state it finds, `start`)"""
    if fn == 'labels_patched':
        out = dict(EDGE_LISTS, vac_by_tol=False, have_labels=True, label_wire=max(wire, start['label_wire']))
        if has_vacuum:
            out['has_vacuum'] = True
        if not owned_only:
            out['zero_outside0'] = -1
        if marks_kept < 2:     # LABEL_MARKS_BOTH
            out['buni_valid'] = False
        if marks_kept < 1:     # LABEL_MARKS_REGIONS
            out['regions_labels'] = False
        return out
    return {
        'drop_table': TABLE,
        'drop_table_and_maxima': TABLE_MAXIMA,
        'drop_edge_lists': EDGE_LISTS,
        'stage_clobbered': {'chg_n': -1},
        'drop_label_marks': LABEL_MARKS,
        'drop_density_results': RESULTS,
        'vacuum_marks_unproven': {'vac_by_tol': False},
        'density_written': dict(TABLE_MAXIMA, have_rho=True, **RESULTS),
        'density_pointer_out': dict(RESULTS, have_rho=True),
        'labels_overwritten': dict(EDGE_LISTS, labels_zero_pending=False, zero_outside0=-1, has_vacuum=has_vacuum,
                                   vac_by_tol=False, label_wire=wire, have_labels=True, **LABEL_MARKS),
    }[fn]


@pytest.fixture(scope='module')
def state(tmp_path_factory):
    gxx = shutil.which('g++') or shutil.which('c++')
    if gxx is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('ctx_state')
    src = d / 'shim.cpp'
    src.write_text(SHIM)
    so = d / 'ctx_state.so'
    subprocess.check_call([gxx, '-O1', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC', '-I', os.path.dirname(HEADER),
                           '-o', str(so), str(src)])
    lib = C.CDLL(str(so))
    assert lib.n_fields() == len(FIELDS)

    def run(fn, start, wire=0, has_vacuum=False, marks_kept=0, owned_only=False):
        v = (C.c_int * len(FIELDS))(*[int(start[f]) for f in FIELDS])
        assert lib.apply(-1 if fn is None else FUNCS.index(fn), wire, int(has_vacuum), int(marks_kept), int(owned_only), v) == 0
        return dict(zip(FIELDS, v))
    run.lib = lib
    return run


def test_the_header_is_plain_cxx_and_lists_these_functions():
    text = open(HEADER).read()
    assert '#include' not in text
    import re
    assert sorted(re.findall(r'static inline void (\w+)\(CtxState &', text)) == sorted(FUNCS)


def test_defaults(state):
    v = (C.c_int * len(FIELDS))()
    state.lib.defaults(v)
    assert dict(zip(FIELDS, v)) == dict(INVALID, has_vacuum=1)   # (vacuum until proven otherwise)


def test_the_shim_round_trips_every_field(state):
    for start in (VALID, INVALID):
        assert state(None, start) == start


CASES = [(fn, 0, False) for fn in FUNCS[:-2]] + [('labels_overwritten', w, hv) for w in (1, 2, 4) for hv in (False, True)]


@pytest.mark.parametrize('fn,wire,has_vacuum', CASES)
def test_each_function_changes_exactly_its_fields(state, fn, wire, has_vacuum):
    stores = expected(fn, wire, has_vacuum)
    for start in (VALID, INVALID):
        got = state(fn, start, wire, has_vacuum)
        want = dict(start, **{f: int(x) for f, x in stores.items()})
        assert got == want, {f: (start[f], got[f], want[f]) for f in FIELDS if got[f] != want[f]}
        changed = {f for f in FIELDS if got[f] != start[f]}
        assert changed <= set(stores)
    # between the two fillings every named field does change, so a dropped store cannot hide behind a start that already held its value
    # (has_vacuum and label_wire take the arguments: VALID holds (2, true), INVALID (4, false))
    moved = {f for start in (VALID, INVALID) for f in FIELDS if state(fn, start, wire, has_vacuum)[f] != start[f]}
    assert moved == set(stores)


PATCH_CASES = [(w, neg, marks, owned) for w in (1, 2, 4) for neg in (False, True) for marks in (0, 1, 2) for owned in (False, True)]


@pytest.mark.parametrize('wire,any_negative,marks_kept,owned_only', PATCH_CASES)
def test_labels_patched_changes_exactly_its_fields(state, wire, any_negative, marks_kept, owned_only):
    """some labels written from outside an assignment (xb_scatter_voxels, label planes of xb_copy_planes, xb_walkers_apply): the
    vacuum marks fall, a negative label brings the vacuum back and none takes it away, the wire width only grows, the label
    marks fall unless the writer vouches for them, zero_outside falls unless only owned planes were written"""
    text = open(HEADER).read()
    assert 'LABEL_MARKS_NONE = 0, LABEL_MARKS_REGIONS = 1, LABEL_MARKS_BOTH = 2' in text
    # (VALID: has_vacuum set, wire 2; INVALID: has_vacuum clear, wire 4; the third start has the vacuum proven absent at wire 1)
    for start in (VALID, INVALID, dict(VALID, has_vacuum=0, label_wire=1)):
        got = state('labels_patched', start, wire, any_negative, marks_kept, owned_only)
        stores = expected('labels_patched', wire, any_negative, marks_kept, owned_only, start)
        want = dict(start, **{f: int(x) for f, x in stores.items()})
        assert got == want, {f: (start[f], got[f], want[f]) for f in FIELDS if got[f] != want[f]}
        assert got['vac_by_tol'] == 0 and got['list_valid'] == 0 and got['chg_n'] == -1 and got['have_labels'] == 1
        assert got['has_vacuum'] == int(bool(start['has_vacuum']) or any_negative)
        assert got['label_wire'] == max(wire, start['label_wire'])
    moved = {f for start in (VALID, INVALID, dict(VALID, has_vacuum=0, label_wire=1)) for f in FIELDS
             if state('labels_patched', start, wire, any_negative, marks_kept, owned_only)[f] != start[f]}
    named = {'list_valid', 'chg_n', 'vac_by_tol', 'have_labels'} | ({'has_vacuum'} if any_negative else set()) | \
        ({'label_wire'} if wire > 1 else set()) | (set() if owned_only else {'zero_outside0'}) | \
        ({'buni_valid'} if marks_kept < 2 else set()) | ({'regions_labels'} if marks_kept < 1 else set())
    assert moved == named
