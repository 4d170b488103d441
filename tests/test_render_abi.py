"""CPU: the entry points of csrc/render.hip are declared, exported and bound alike, the options struct equals its ctypes mirror, every
argument check answers before any HIP call (no GPU here) and names the argument, and the workspace size is the documented one."""
import ctypes as C
import os
import re

import pytest

import straps_amd
from straps_amd import hipabi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_render_mesh_workspace_bytes', 'straps_render_mesh')
EINVAL = 1


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


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
    assert len(hipabi.SIGNATURES['straps_render_mesh'][1]) == 20 and hipabi.SIGNATURES['straps_render_mesh'][0] is C.c_int
    assert hipabi.SIGNATURES['straps_render_mesh_workspace_bytes'] == (C.c_size_t, [C.c_longlong, C.c_int, C.c_int])
    assert 'render.hip' in hipabi.SOURCES
    assert all(hasattr(straps_amd, n) for n in ('WeakPerspectiveMeshRenderer', 'vertex_face_table', 'Predictor'))
    assert hasattr(straps_amd.Predictor, 'render')
    from straps_amd import weak_perspective_pyrender_renderer
    assert hasattr(weak_perspective_pyrender_renderer, 'Renderer')


def test_options_struct_equals_its_mirror():
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} straps_render_opts_t;', plain).group(1)
    ctype = {'float': C.c_float, 'int32_t': C.c_int32, 'int': C.c_int}
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            typ, name = decl.split()
            m = re.match(r'(\w+)\[(\d+)\]$', name)
            fields.append((m.group(1), ctype[typ] * int(m.group(2))) if m else (name, ctype[typ]))
    assert [f[0] for f in fields] == ['colour', 'ambient', 'background', 'n_lights', 'light_dir', 'light_intensity']
    mirror = hipabi.RenderOptsStruct._fields_
    assert [f[0] for f in mirror] == [f[0] for f in fields]
    for (name, want), (_, got) in zip(fields, mirror):
        assert C.sizeof(want) == C.sizeof(got) and getattr(want, '_length_', 1) == getattr(got, '_length_', 1), name
        assert getattr(want, '_type_', want) == getattr(got, '_type_', got), name
    assert C.sizeof(hipabi.RenderOptsStruct) == 24 * 4 == sum(C.sizeof(t) for _, t in fields)      # no padding
    S = hipabi.RenderOptsStruct
    assert (S.colour.offset, S.ambient.offset, S.background.offset, S.n_lights.offset, S.light_dir.offset, S.light_intensity.offset) == (0, 12, 16, 28, 32, 80)


def test_workspace_formula(lib):
    ws = lib.straps_render_mesh_workspace_bytes
    for B, N, wh in ((1, 1, 1), (1, 3, 16), (3, 257, 20), (64, 6890, 256), (2, 110, 4096), (1 << 20, 6890, 256)):
        assert ws(B, N, wh) == B * (8 * wh * wh + 32 * N), (B, N, wh)
    assert ws(0, 6890, 256) == 0 and ws(-1, 6890, 256) == 0 and ws(4, 0, 256) == 0 and ws(4, -7, 256) == 0
    assert ws(4, 6890, 0) == 0 and ws(4, 6890, -1) == 0 and ws(4, 6890, 4097) == 0


def _opts(n_lights=2, ambient=0.3):
    o = hipabi.RenderOptsStruct()
    o.colour[:] = (0.8, 0.3, 0.3)
    o.ambient, o.n_lights = ambient, n_lights
    return o


def test_argument_validation_without_gpu(lib):
    """every failure returns STRAPS_EINVAL before any HIP call (the pointers are never dereferenced) and names the argument"""
    err = lambda: lib.straps_last_error().decode()
    p = lambda v: C.c_void_p(v)
    A = 8192
    good = _opts()

    def call(verts=A, faces=A, vf_offsets=A, vf_faces=A, cam=A, ld_cam=3, rotation=None, per_body=0, opts=good, background=None, rgb=A, mask=A, depth=A,
             face_ids=A, ws=A, batch=2, nv=6890, nf=13776, wh=256):
        return lib.straps_render_mesh(p(verts), p(faces), p(vf_offsets), p(vf_faces), p(cam), ld_cam, p(rotation), per_body,
                                      C.byref(opts) if opts is not None else None, p(background), p(rgb), p(mask), p(depth), p(face_ids), p(ws), batch, nv, nf,
                                      wh, None)
    for name, text in (('verts', 'verts'), ('faces', 'faces'), ('vf_offsets', 'vf_offsets'), ('vf_faces', 'vf_faces'), ('cam', 'cam_wp'), ('opts', 'opts'),
                       ('rgb', 'rgb'), ('ws', 'workspace')):
        assert call(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err() and 'straps_render_mesh' in err(), name
    for off in (1, 2, 4, 6):
        assert call(ws=A + off) == EINVAL and '`workspace`' in err() and '8-byte aligned' in err(), off
    for ld in (2, 0, -3):
        assert call(ld_cam=ld) == EINVAL and '`ld_cam`' in err() and str(ld) in err(), ld
    for wh in (0, -1, 4097):
        assert call(wh=wh) == EINVAL and '`wh`' in err(), wh
    for kw in ({'batch': 0}, {'nv': 0}, {'nf': 0}, {'batch': -2}, {'nv': -1}, {'nf': -5}):
        assert call(**kw) == EINVAL and '`batch`' in err() and '`nverts`' in err() and '`nfaces`' in err(), kw
    assert call(batch=1, nf=0x7fffffff // 3 + 1) == EINVAL and '`nfaces`' in err() and '715827882' in err()
    for n in (-1, 5, 1 << 20):
        assert call(opts=_opts(n_lights=n)) == EINVAL and '`n_lights`' in err(), n
    for a in (-0.01, float('nan'), float('inf'), -float('inf')):
        assert call(opts=_opts(ambient=a)) == EINVAL and '`ambient`' in err(), a
    assert call(batch=1 << 36) == EINVAL and 'too large' in err()
    assert call(batch=1 << 24, wh=4096) == EINVAL and 'too large' in err()            # the pixel launch
    assert call(batch=1 << 17, nv=1, nf=0x7fffffff // 3) == EINVAL and 'too large' in err()      # the face launch


def test_python_surface_checks_without_gpu():
    """the host side of the module: table buffers, light normalisation, refusals -- and NMRRenderer's RGB mode still raises"""
    import numpy as np
    faces = np.array([[0, 1, 2], [2, 1, 3]], np.int32)
    r = straps_amd.WeakPerspectiveMeshRenderer(faces, img_wh=20)
    assert set(dict(r.named_buffers())) == {'faces', 'vf_offsets', 'vf_faces'} and r.img_wh == 20 and r.num_vertices == 4
    assert r.vf_offsets.tolist() == [0, 1, 3, 5, 6] and r.vf_faces.tolist() == [0, 0, 1, 0, 1, 1]
    o = r.render_opts()
    assert o.n_lights == 2 and abs(o.ambient - 0.3) < 1e-7 and [round(c, 6) for c in o.colour] == [0.8, 0.3, 0.3]
    s = 2.0 ** -0.5
    assert np.allclose(list(o.light_dir)[:6], [0, s, -s, 0, -s, -s], atol=1e-7) and list(o.light_intensity)[:2] == [1.0, 1.0]
    assert [round(c, 6) for c in r.render_opts(colour=(0.1, 0.2, 0.3)).colour] == [0.1, 0.2, 0.3]
    with pytest.raises(RuntimeError):
        straps_amd.WeakPerspectiveMeshRenderer(faces, lights=(((0, 0, 0), 1.0),))
    with pytest.raises(RuntimeError):
        straps_amd.WeakPerspectiveMeshRenderer(faces, lights=(((0, 0, -1), 1.0),) * 5)
    with pytest.raises(RuntimeError):
        straps_amd.WeakPerspectiveMeshRenderer(faces, img_wh=4097)
    with pytest.raises(RuntimeError):
        straps_amd.WeakPerspectiveMeshRenderer(faces.reshape(-1))
    with pytest.raises(RuntimeError):
        straps_amd.NMRRenderer(1, np.eye(3), np.eye(3), rend_parts_seg=False)
    from straps_amd.weak_perspective_pyrender_renderer import rotation_matrix
    assert np.allclose(rotation_matrix(180, [1, 0, 0]), np.diag([1.0, -1.0, -1.0]), atol=1e-15)
    assert np.allclose(rotation_matrix(90, [0, 0, 2]).dot([1.0, 0.0, 0.0]), [0.0, 1.0, 0.0], atol=1e-15)
