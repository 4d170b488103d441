"""CPU: the entry points of csrc/fit_subjects.hip are declared, exported and bound alike and validate their arguments before any HIP call (no GPU
here): every check returns the error code and names the argument."""
import ctypes as C
import os
import re

import pytest

from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_fit_adam_subjects', 'straps_subject_mean_rows')


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _buf(keep, n=64):
    raw = (C.c_char * (n + 16))()
    keep.append(raw)
    return C.c_void_p((C.addressof(raw) + 15) & ~15)


def test_header_exports_and_prototypes_agree(lib):
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert int(re.search(r'#define STRAPS_ABI_VERSION (\d+)', txt).group(1)) == 12 == hipabi.ABI_VERSION == lib.straps_abi_version()      # no version change
    for n in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % n, plain)
        assert decl, '%s is not declared' % n
        assert hasattr(lib, n), '%s is not exported' % n
        res, args = hipabi.SIGNATURES[n]
        assert len([a for a in decl.group(1).split(',') if a.strip()]) == len(args), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res
    assert 'fit_subjects.hip' in hipabi.SOURCES
    # the block that states the semantics
    for word in ('FIRST row', 'frame_mask', 'fixed order', 'EVERY row', 'first minimum wins', 'An empty', 'Consequence'):
        assert word in txt, word


def test_fit_adam_subjects_checks_its_arguments(lib):
    keep = []
    p = _buf(keep, 157 * 4)
    err = lib.straps_last_error
    o = hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, 256.0)

    def call(est=p, offsets=p, m=p, v=p, sm=p, sv=p, energy=p, ld=1, col=0, sub=p, ld_sub=1, best=p, best_e=p, step=0, update=1, batch=1, n_subjects=1, opts=o):
        return lib.straps_fit_adam_subjects(C.byref(opts) if opts is not None else None, est, offsets, None, p, None, None, None, p, None, 100.0, 100.0, m, v, sm, sv,
                                            energy, ld, col, sub, ld_sub, None, best, best_e, step, 1, update, batch, n_subjects, None)
    assert call(est=None) == 1 and b'est' in err()
    assert call(opts=None) == 1 and b'opts' in err()
    assert call(offsets=None) == 1 and b'offsets' in err()
    assert call(m=None) == 1 and b'exp_avg' in err()
    assert call(v=None) == 1 and b'exp_avg' in err()
    assert call(sm=None) == 1 and b'shape_avg' in err()
    assert call(sv=None) == 1 and b'shape_avg_sq' in err()
    assert call(best=None) == 1 and b'together' in err()
    assert call(best_e=None) == 1 and b'together' in err()
    assert call(col=1) == 1 and b'ld_energy' in err()
    assert call(col=-1) == 1 and b'col' in err()
    assert call(energy=None, ld=0, col=1) == 1 and b'ld_subject' in err()
    assert call(energy=None, ld=0, ld_sub=0) == 1 and b'ld_subject' in err()
    assert call(ld=4, col=2, ld_sub=2) == 1 and b'ld_subject' in err()
    assert call(step=-1) == 1 and b'step' in err()
    assert call(batch=0) == 1 and b'batch' in err()
    assert call(n_subjects=0) == 1 and b'n_subjects' in err()
    assert call(n_subjects=2) == 1 and b'n_subjects' in err()
    assert call(batch=3, n_subjects=4) == 1 and b'n_subjects' in err()
    assert call(opts=hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 1.0, 0.999, 1e-8, 0.0, 1e-3, 1e-3, 256.0)) == 1 and b'beta1' in err()
    assert call(opts=hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 0.9, 0.999, 0.0, 0.0, 1e-3, 1e-3, 256.0)) == 1 and b'eps' in err()


def test_subject_mean_rows_checks_its_arguments(lib):
    keep = []
    p = _buf(keep, 256)
    err = lib.straps_last_error

    def call(rows=p, ld=10, cols=10, offsets=p, out=p, batch=1, n_subjects=1):
        return lib.straps_subject_mean_rows(rows, ld, cols, offsets, None, out, batch, n_subjects, None)
    assert call(rows=None) == 1 and b'rows' in err()
    assert call(out=None) == 1 and b'out' in err()
    assert call(offsets=None) == 1 and b'offsets' in err()
    assert call(cols=0) == 1 and b'cols' in err()
    assert call(cols=65, ld=65) == 1 and b'cols' in err()
    assert call(ld=9) == 1 and b'ld' in err()
    assert call(batch=0) == 1 and b'batch' in err()
    assert call(n_subjects=0) == 1 and b'n_subjects' in err()
    assert call(n_subjects=2) == 1 and b'n_subjects' in err()
