"""CPU: the entry points of csrc/scanfit.hip are declared, exported and bound alike, validate their arguments before any HIP call (no GPU
here) and report the documented workspace size."""
import ctypes as C
import os
import re

import pytest

from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_scan_energy_workspace_bytes', 'straps_scan_energy')
INF, NAN = float('inf'), float('nan')


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
    assert int(re.search(r'#define STRAPS_ABI_VERSION (\d+)', txt).group(1)) == 12 == hipabi.ABI_VERSION == lib.straps_abi_version()
    for n in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % n, plain)
        assert decl, '%s is not declared' % n
        assert hasattr(lib, n), '%s is not exported' % n
        res, args = hipabi.SIGNATURES[n]
        assert len([a for a in decl.group(1).split(',') if a.strip()]) == len(args), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res
    body = re.search(r'typedef struct \{([^}]*)\} straps_scan_opts_t;', plain).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            names = [x.strip() for x in decl.split(',')]
            assert decl.split()[0] == 'float'
            names[0] = names[0].split()[-1]
            fields += names
    assert fields == [f[0] for f in hipabi.ScanOptsStruct._fields_] == ['sigma', 'w_s2m', 'w_m2s']
    assert all(f[1] is C.c_float for f in hipabi.ScanOptsStruct._fields_) and C.sizeof(hipabi.ScanOptsStruct) == 12
    assert 'scanfit.hip' in hipabi.SOURCES and os.path.isfile(os.path.join(hipabi.CSRC, 'scanfit.hip'))


def _energy(lib, keep, **kw):
    p = _buf(keep)
    o = hipabi.ScanOptsStruct(kw.pop('sigma', 0.1), kw.pop('w_s2m', 100.0), kw.pop('w_m2s', 100.0))
    a = dict(verts=p, trans=p, points=p, opts=C.byref(o), energy2=p, dverts=p, dtrans=p, nearest_vertex=p, nearest_point=p, workspace=p, batch=1, nverts=8,
             npoints=8, ld_trans=3)
    a.update(kw)
    return lib.straps_scan_energy(a['verts'], a['trans'], a['ld_trans'], a['points'], a['opts'], a['energy2'], a['dverts'], a['dtrans'], a['nearest_vertex'],
                                  a['nearest_point'], a['workspace'], a['batch'], a['nverts'], a['npoints'], None)


def test_scan_energy_checks_its_arguments(lib):
    keep = []
    err = lib.straps_last_error
    assert _energy(lib, keep, verts=None) == 1 and b'verts' in err()
    assert _energy(lib, keep, points=None) == 1 and b'points' in err()
    assert _energy(lib, keep, trans=None) == 1 and b'trans' in err() and b'ld_trans' not in err()
    assert _energy(lib, keep, opts=None) == 1 and b'opts' in err()
    assert _energy(lib, keep, workspace=None) == 1 and b'workspace' in err()
    assert _energy(lib, keep, energy2=None, dverts=None, dtrans=None, nearest_vertex=None, nearest_point=None) == 1 and b'outputs' in err()
    for bad in (0, (1 << 20) + 1, -3):
        assert _energy(lib, keep, nverts=bad) == 1 and b'nverts' in err()
        assert _energy(lib, keep, npoints=bad) == 1 and b'npoints' in err()
    assert _energy(lib, keep, batch=0) == 1 and b'batch' in err()
    assert _energy(lib, keep, batch=-1) == 1 and b'batch' in err()
    assert _energy(lib, keep, ld_trans=2) == 1 and b'ld_trans' in err()
    for bad in (-1.0, INF, NAN):
        assert _energy(lib, keep, sigma=bad) == 1 and b'sigma' in err()
        assert _energy(lib, keep, w_s2m=bad) == 1 and b'w_s2m' in err()
        assert _energy(lib, keep, w_m2s=bad) == 1 and b'w_m2s' in err()
    assert lib.straps_scan_energy(None, None, 3, None, None, None, None, None, None, None, None, 1, 1, 1, None) == 1 and b'opts' in err()


def test_workspace_bytes_is_the_documented_size(lib):
    f = lib.straps_scan_energy_workspace_bytes
    up = lambda a, b: -(-a // b)
    for B, nv, npts in ((1, 1, 1), (3, 6890, 16384), (64, 6890, 16384), (2, 257, 1025), (1, 65537, 64), (1, 1 << 20, 1 << 20)):
        assert f(B, nv, npts) == B * (24 * nv + 28 * npts + 16 * up(nv, 256) + 4 * up(npts, 256) + 16), (B, nv, npts)
    assert f(0, 8, 8) == 0 and f(-1, 8, 8) == 0 and f(1 << 19, 8, 8) == 0
    assert f(1, 0, 8) == 0 and f(1, (1 << 20) + 1, 8) == 0 and f(1, 8, 0) == 0 and f(1, 8, (1 << 20) + 1) == 0
