"""CPU: straps_fit_keypoints validates its arguments before any HIP call (no GPU here), and hipabi mirrors its structs."""
import ctypes as C
import os
import re

import pytest

from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _buf(n, t=C.c_float):
    """host memory with 16-byte alignment: never dereferenced, the call fails at validation"""
    raw = (C.c_char * (n * 4 + 16))()
    addr = (C.addressof(raw) + 15) & ~15
    return raw, C.c_void_p(addr)


def _call(lib, keep, **kw):
    m = hipabi.FitModelStruct()
    for f in ('j_template', 'j_shapedirs', 'parents', 'vert_dirs', 'vert_w', 'kp_src'):
        raw, p = _buf(16 * 3 * 224)
        keep.append(raw)
        setattr(m, f, p)
    m.n_verts, m.n_kp = kw.pop('n_verts', 5), kw.pop('n_kp', 17)
    o = hipabi.FitOptsStruct(kw.pop('iters', 10), kw.pop('step0', 0), 0.01, 0.01, 0.01, 0.9, 0.999, 1e-8, 0.0, 1e-3, 1e-3, kw.pop('img_wh', 256.0))
    args = {}
    for name in ('est', 'targets', 'exp_avg', 'exp_avg_sq'):
        raw, p = _buf(157 * 4)
        keep.append(raw)
        args[name] = p
    args.update(kw)
    return lib.straps_fit_keypoints(C.byref(m), C.byref(o), args['est'], None, args['targets'], None, args['exp_avg'], args['exp_avg_sq'],
                                    None, None, None, None, None, kw.get('batch', 1), None)


def test_arguments_are_checked_before_any_hip_call(lib):
    keep = []
    assert _call(lib, keep, est=None) == 1 and b'null pointer' in lib.straps_last_error()
    assert _call(lib, keep, targets=None) == 1
    assert _call(lib, keep, iters=-1) == 1 and b'iters' in lib.straps_last_error()
    assert _call(lib, keep, iters=10001) == 1 and b'iters' in lib.straps_last_error()
    assert _call(lib, keep, n_kp=0) == 1 and b'n_kp' in lib.straps_last_error()
    assert _call(lib, keep, n_kp=33) == 1 and b'n_kp' in lib.straps_last_error()
    assert _call(lib, keep, n_verts=17) == 1 and b'n_verts' in lib.straps_last_error()
    assert _call(lib, keep, n_verts=-1) == 1
    assert _call(lib, keep, exp_avg=None) == 1 and b'together' in lib.straps_last_error()
    assert _call(lib, keep, exp_avg_sq=None) == 1 and b'together' in lib.straps_last_error()
    assert _call(lib, keep, batch=0) == 1
    assert _call(lib, keep, step0=-1) == 1
    assert _call(lib, keep, img_wh=0.0) == 1
    assert lib.straps_fit_keypoints(None, None, None, None, None, None, None, None, None, None, None, None, None, 1, None) == 1


def test_structs_mirror_the_header_and_the_version_stays(lib):
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    assert int(re.search(r'#define STRAPS_ABI_VERSION (\d+)', txt).group(1)) == 12 == hipabi.ABI_VERSION == lib.straps_abi_version()
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    for cls, name in ((hipabi.FitModelStruct, 'straps_fit_model_t'), (hipabi.FitOptsStruct, 'straps_fit_opts_t')):
        body = re.search(r'typedef struct \{([^}]*)\} %s;' % name, plain).group(1)
        fields = []
        for decl in body.split(';'):
            decl = decl.strip()
            if decl:
                names = [n.strip().lstrip('*') for n in decl.split(',')]
                names[0] = names[0].split()[-1].lstrip('*')
                fields += names
        assert fields == [f[0] for f in cls._fields_], name
    assert C.sizeof(hipabi.FitModelStruct) == 6 * 8 + 8 and C.sizeof(hipabi.FitOptsStruct) == 12 * 4
    assert 'fit.hip' in hipabi.SOURCES
