"""CPU: the entry points of csrc/silfit.hip are declared, exported and bound alike, validate their arguments before any HIP call (no GPU
here) and report the documented workspace size."""
import ctypes as C
import os
import re

import pytest

from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_distance_field', 'straps_silhouette_energy_workspace_bytes', 'straps_silhouette_energy', 'straps_fit_adam')


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
    body = re.search(r'typedef struct \{([^}]*)\} straps_silfit_opts_t;', plain).group(1)
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            names = [x.strip() for x in decl.split(',')]
            names[0] = names[0].split()[-1]
            fields += names
    assert fields == [f[0] for f in hipabi.SilFitOptsStruct._fields_] and C.sizeof(hipabi.SilFitOptsStruct) == 20
    assert 'silfit.hip' in hipabi.SOURCES


def test_distance_field_checks_its_arguments(lib):
    keep = []
    p = _buf(keep)
    err = lib.straps_last_error
    assert lib.straps_distance_field(None, p, 1, 4, None) == 1 and b'mask' in err()
    assert lib.straps_distance_field(p, None, 1, 4, None) == 1 and b'd2' in err()
    assert lib.straps_distance_field(p, p, 1, 0, None) == 1 and b'wh' in err()
    assert lib.straps_distance_field(p, p, 1, 1025, None) == 1 and b'wh' in err()
    assert lib.straps_distance_field(p, p, 0, 4, None) == 1 and b'batch' in err()


def _energy(lib, keep, **kw):
    p = _buf(keep)
    o = hipabi.SilFitOptsStruct(kw.pop('wh', 16), kw.pop('lattice', 4), kw.pop('tau', 1.5), 100.0, 100.0)
    a = dict(verts=p, cam=p, mask=p, d2=p, energy2=p, dverts=p, dcam=p, nearest=p, workspace=p, batch=1, nverts=8, ld_cam=3)
    a.update(kw)
    return lib.straps_silhouette_energy(a['verts'], a['cam'], a['ld_cam'], a['mask'], a['d2'], C.byref(o), a['energy2'], a['dverts'], a['dcam'], a['nearest'],
                                        a['workspace'], a['batch'], a['nverts'], None)


def test_silhouette_energy_checks_its_arguments(lib):
    keep = []
    err = lib.straps_last_error
    assert _energy(lib, keep, mask=None) == 1 and b'mask' in err()
    assert _energy(lib, keep, d2=None) == 1 and b'd2' in err()
    assert _energy(lib, keep, verts=None) == 1 and b'verts' in err()
    assert _energy(lib, keep, workspace=None) == 1 and b'workspace' in err()
    assert _energy(lib, keep, wh=0) == 1 and b'wh' in err()
    assert _energy(lib, keep, wh=1) == 1 and b'wh' in err()
    assert _energy(lib, keep, wh=1025) == 1 and b'wh' in err()
    assert _energy(lib, keep, lattice=0) == 1 and b'lattice' in err()
    assert _energy(lib, keep, energy2=None, dverts=None, dcam=None, nearest=None) == 1 and b'outputs' in err()
    assert _energy(lib, keep, nverts=0) == 1 and b'nverts' in err()
    assert _energy(lib, keep, batch=0) == 1 and b'batch' in err()
    assert _energy(lib, keep, ld_cam=2) == 1 and b'ld_cam' in err()
    assert _energy(lib, keep, tau=-1.0) == 1 and b'tau' in err()
    assert lib.straps_silhouette_energy(None, None, 3, None, None, None, None, None, None, None, None, 1, 1, None) == 1 and b'opts' in err()


def test_workspace_bytes_is_the_documented_size(lib):
    f = lib.straps_silhouette_energy_workspace_bytes
    for B, nv, wh, lat in ((1, 1, 2, 1), (3, 6890, 256, 4), (64, 6890, 256, 4), (2, 257, 33, 5), (1, 7000, 16, 17), (1024, 6890, 256, 1)):
        nl = -(-wh // lat)
        assert f(B, nv, wh, lat) == B * (16 * (nv + nl * nl + -(-nv // 256)) + 128), (B, nv, wh, lat)
    assert f(0, 8, 16, 4) == 0 and f(1, 0, 16, 4) == 0 and f(1, 8, 1, 4) == 0 and f(1, 8, 1025, 4) == 0 and f(1, 8, 16, 0) == 0


def test_fit_adam_checks_its_arguments(lib):
    keep = []
    p = _buf(keep, 157 * 4)
    err = lib.straps_last_error
    o = hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, 256.0)

    def call(est=p, m=p, v=p, energy=p, ld=1, col=0, best=p, best_e=p, step=0, update=1, batch=1, opts=o):
        return lib.straps_fit_adam(C.byref(opts) if opts is not None else None, est, p, None, None, None, p, None, 100.0, 100.0, m, v, energy, ld, col, None, best,
                                   best_e, step, 1, update, batch, None)
    assert call(est=None) == 1 and b'est' in err()
    assert call(opts=None) == 1 and b'opts' in err()
    assert call(m=None) == 1 and b'exp_avg' in err()
    assert call(v=None) == 1 and b'exp_avg' in err()
    assert call(best=None) == 1 and b'together' in err()
    assert call(best_e=None) == 1 and b'together' in err()
    assert call(col=1) == 1 and b'col' in err()
    assert call(step=-1) == 1 and b'step' in err()
    assert call(batch=0) == 1 and b'batch' in err()
    assert call(opts=hipabi.FitOptsStruct(0, 0, 0.01, 0.01, 0.01, 1.0, 0.999, 1e-8, 0.0, 1e-3, 1e-3, 256.0)) == 1 and b'beta1' in err()
