"""CPU: the entry points of csrc/measure.hip are declared, exported and bound alike, the measurement struct equals its ctypes mirror, every
argument check answers before any HIP call (no GPU here) and names the argument, and the workspace size is the documented one."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import straps_amd
from straps_amd import hipabi, measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_measure_workspace_bytes', 'straps_measure_mesh')
EINVAL = 1
FPB, VPB = hipabi.MEASURE_FACES_PER_BLOCK, hipabi.MEASURE_VERTS_PER_BLOCK


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
    assert len(hipabi.SIGNATURES['straps_measure_mesh'][1]) == 13 and hipabi.SIGNATURES['straps_measure_mesh'][0] is C.c_int
    assert hipabi.SIGNATURES['straps_measure_workspace_bytes'] == (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_int])
    assert 'measure.hip' in hipabi.SOURCES
    kinds = re.search(r'enum \{([^}]*STRAPS_MEASURE_VOLUME[^}]*)\}', plain).group(1)
    assert dict((k.strip(), int(v)) for k, v in (e.split('=') for e in kinds.split(','))) == {
        'STRAPS_MEASURE_VOLUME': hipabi.MEASURE_VOLUME, 'STRAPS_MEASURE_AREA': hipabi.MEASURE_AREA, 'STRAPS_MEASURE_EXTENT': hipabi.MEASURE_EXTENT,
        'STRAPS_MEASURE_GIRTH': hipabi.MEASURE_GIRTH, 'STRAPS_MEASURE_PATH': hipabi.MEASURE_PATH}
    assert (hipabi.MEASURE_VOLUME, hipabi.MEASURE_AREA, hipabi.MEASURE_EXTENT, hipabi.MEASURE_GIRTH, hipabi.MEASURE_PATH) == (0, 1, 2, 3, 4)
    assert all(hasattr(straps_amd, n) for n in ('BodyMeasurer', 'default_measurements', 'measure', 'Predictor'))
    assert hasattr(straps_amd.Predictor, 'measure') and hasattr(straps_amd.BodyMeasurer, 'from_smpl')
    # the block sizes the workspace formula is written with stand in the kernel source as well
    src = open(os.path.join(hipabi.CSRC, 'measure.hip')).read()
    assert int(re.search(r'MS_FACES_PER_BLOCK = (\d+);', src).group(1)) == FPB and int(re.search(r'MS_VERTS_PER_BLOCK = (\d+);', src).group(1)) == VPB


def test_struct_equals_its_mirror():
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} straps_measure_t;', plain).group(1)
    ctype = {'float': C.c_float, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32}
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            typ, name = decl.split()
            m = re.match(r'(\w+)\[(\d+)\]$', name)
            fields.append((m.group(1), ctype[typ] * int(m.group(2))) if m else (name, ctype[typ]))
    assert [f[0] for f in fields] == ['kind', 'anchor', 'dir', 'part_mask']
    mirror = hipabi.MeasureStruct._fields_
    assert [f[0] for f in mirror] == [f[0] for f in fields]
    for (name, want), (_, got) in zip(fields, mirror):
        assert C.sizeof(want) == C.sizeof(got) and getattr(want, '_length_', 1) == getattr(got, '_length_', 1), name
        assert getattr(want, '_type_', want) == getattr(got, '_type_', got), name
    S = hipabi.MeasureStruct
    assert C.sizeof(S) == 36 == 9 * 4 == sum(C.sizeof(t) for _, t in fields)      # nine words, no padding
    assert (S.kind.offset, S.anchor.offset, S.dir.offset, S.part_mask.offset) == (0, 4, 20, 32)
    assert C.sizeof(S * 32) == 32 * 36


def test_workspace_formula(lib):
    ws = lib.straps_measure_workspace_bytes
    cdiv = lambda a, b: (a + b - 1) // b
    for B, N, F, M in ((1, 1, 0, 1), (1, 3, 1, 1), (3, 64, 65, 32), (64, 6890, 13776, 15), (2, VPB, FPB, 5), (2, VPB + 1, FPB + 1, 5), (7, VPB - 1, 2 * FPB + 1, 32),
                       (1, 1 << 20, 0x7fffffff // 3, 32), (1 << 20, 6890, 13776, 15)):
        assert ws(B, N, F, M) == B * M * 8 * (cdiv(F, FPB) + 2 * cdiv(N, VPB)), (B, N, F, M)
    assert ws(64, 6890, 13776, 15) == 64 * 15 * 8 * (27 + 2 * 4)
    for bad in ((0, 6890, 13776, 15), (-1, 6890, 13776, 15), (4, 0, 13776, 15), (4, -7, 13776, 15), (4, (1 << 20) + 1, 13776, 15), (4, 6890, -1, 15),
                (4, 6890, 0x7fffffff // 3 + 1, 15), (4, 6890, 13776, 0), (4, 6890, 13776, 33), (4, 6890, 13776, -2), (1 << 31, 6890, 13776, 15)):
        assert ws(*bad) == 0, bad


def _meas(*items):
    arr = (hipabi.MeasureStruct * len(items))()
    for q, (kind, anchor, direction, mask) in zip(arr, items):
        q.kind = kind
        q.anchor[:] = list(anchor) + [-1] * (4 - len(anchor))
        q.dir[:] = direction
        q.part_mask = mask
    return arr


Y = (0.0, 1.0, 0.0)
GOOD = ((hipabi.MEASURE_VOLUME, (), Y, 0), (hipabi.MEASURE_AREA, (), Y, 0), (hipabi.MEASURE_EXTENT, (), Y, 0), (hipabi.MEASURE_GIRTH, (6890 + 3,), Y, 1 << 6),
        (hipabi.MEASURE_PATH, (0, 6890 + 23), Y, 0))


def test_argument_validation_without_gpu(lib):
    """every failure returns STRAPS_EINVAL before any HIP call (the device pointers are never dereferenced) and names the argument"""
    err = lambda: lib.straps_last_error().decode()
    p = lambda v: C.c_void_p(v)
    A = 8192

    def call(verts=A, points=A, faces=A, face_parts=A, meas=GOOD, out=A, ws=A, batch=2, nv=6890, n_points=24, nf=13776, n_meas=None, meas_null=False):
        arr = _meas(*meas) if meas else None
        return lib.straps_measure_mesh(p(verts), p(points), p(faces), p(face_parts), None if meas_null else arr, p(out), p(ws), batch, nv, n_points, nf,
                                       len(meas) if n_meas is None else n_meas, None)
    for name, text in (('verts', 'verts'), ('faces', 'faces'), ('out', 'out'), ('ws', 'workspace')):
        assert call(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err() and 'straps_measure_mesh' in err(), name
    assert call(meas_null=True) == EINVAL and '`meas`' in err() and 'null pointer' in err()
    for off in (1, 2, 4, 6):
        assert call(ws=A + off) == EINVAL and '`workspace`' in err() and '8-byte aligned' in err(), off
    for n in (0, 33, -1):
        assert call(n_meas=n) == EINVAL and '`n_meas`' in err() and str(n) in err(), n
    for b in (0, -2, 1 << 31):
        assert call(batch=b) == EINVAL and '`batch`' in err(), b
    for nv in (0, -1, (1 << 20) + 1):
        assert call(nv=nv) == EINVAL and '`nverts`' in err(), nv
    for npts in (-1, 65):
        assert call(n_points=npts) == EINVAL and '`n_points`' in err(), npts
    for nf in (-1, 0x7fffffff // 3 + 1):
        assert call(nf=nf) == EINVAL and '`nfaces`' in err(), nf
    for kind in (5, -1, 1 << 20):
        assert call(meas=GOOD[:2] + ((kind, (), Y, 0),)) == EINVAL and '`meas[2].kind`' in err() and 'unknown' in err(), kind
    assert call(meas=((hipabi.MEASURE_GIRTH, (), Y, 0),)) == EINVAL and '`meas[0]`' in err() and 'GIRTH' in err() and '`anchor[0]`' in err()
    assert call(meas=GOOD[:1] + ((hipabi.MEASURE_PATH, (5,), Y, 0),)) == EINVAL and '`meas[1]`' in err() and 'PATH' in err() and '`anchor`' in err()
    assert call(meas=((hipabi.MEASURE_PATH, (), Y, 0),)) == EINVAL and 'PATH' in err()
    assert call(meas=((hipabi.MEASURE_PATH, (-1, 4, 5), Y, 0),)) == EINVAL and 'PATH' in err()                      # the LEADING entries count
    for kind, anchor, where in ((hipabi.MEASURE_GIRTH, (6890 + 24,), 'anchor[0]'), (hipabi.MEASURE_VOLUME, (6890 + 24,), 'anchor[0]'),
                                (hipabi.MEASURE_PATH, (0, 1, 6890 + 24), 'anchor[2]'), (hipabi.MEASURE_PATH, (0, 1, 2, 1 << 30), 'anchor[3]'),
                                (hipabi.MEASURE_VOLUME, (-2,), 'anchor[0]'), (hipabi.MEASURE_GIRTH, (-5,), 'anchor[0]')):
        assert call(meas=((kind, anchor, Y, 0),)) == EINVAL and '`meas[0].%s`' % where in err() and str(anchor[-1]) in err(), (kind, anchor)
    assert call(meas=((hipabi.MEASURE_GIRTH, (6890,), Y, 0),), n_points=0, points=None) == EINVAL and '`meas[0].anchor[0]`' in err()      # no points: vertices only
    for kind in (hipabi.MEASURE_VOLUME, hipabi.MEASURE_AREA, hipabi.MEASURE_GIRTH):
        assert call(meas=GOOD[:1] + ((kind, (3,), Y, 1 << 4),), face_parts=None) == EINVAL and '`meas[1].part_mask`' in err() and '`face_parts`' in err(), kind
    assert call(points=None) == EINVAL and '`points`' in err() and 'n_points' in err()
    for kind in (hipabi.MEASURE_VOLUME, hipabi.MEASURE_AREA, hipabi.MEASURE_GIRTH):
        assert call(meas=((kind, (3,), Y, 0),), nf=0) == EINVAL and '`nfaces`' in err() and '`meas[0]`' in err(), kind
    assert call(batch=(1 << 31) - 1) == EINVAL and 'too large' in err()


def test_python_surface_checks_without_gpu():
    """the host side of the module: spec helpers, table buffers, anchor resolution, refusals"""
    import torch
    model = straps_amd.synthetic_smpl_model(0)
    d = measure.default_measurements()
    assert list(d) == ['height', 'volume', 'surface_area', 'chest_girth', 'waist_girth', 'hip_girth', 'thigh_girth_l', 'thigh_girth_r', 'upper_arm_girth_l',
                       'upper_arm_girth_r', 'arm_length_l', 'arm_length_r', 'leg_length_l', 'leg_length_r', 'shoulder_breadth']
    assert d['height'] == measure.extent((0, 1, 0)) and d['volume'] == measure.volume() and d['surface_area'] == measure.area()
    assert d['chest_girth'] == measure.girth(('joint', 9), (0, 1, 0), parts=[6]) and d['waist_girth'].anchors == (('joint', 3),) and d['hip_girth'].anchors == (('joint', 0),)
    assert d['thigh_girth_l'].anchors[0] in (('joint', 1), ('joint', 4)) and d['thigh_girth_r'].anchors[0] in (('joint', 2), ('joint', 5))
    assert d['thigh_girth_l'].parts == (4,) and d['thigh_girth_r'].parts == (5,) and d['thigh_girth_l'].direction == (0.0, 1.0, 0.0)
    assert d['upper_arm_girth_l'] == measure.girth(('joint', 18), (1, 0, 0), parts=(1,)) and d['upper_arm_girth_r'] == measure.girth(('joint', 19), (1, 0, 0), parts=(2,))
    assert d['arm_length_l'] == measure.path(('joint', 16), ('joint', 18), ('joint', 20)) and d['arm_length_r'] == measure.path(('joint', 17), ('joint', 19), ('joint', 21))
    assert d['leg_length_l'] == measure.path(('joint', 1), ('joint', 4), ('joint', 7)) and d['leg_length_r'] == measure.path(('joint', 2), ('joint', 5), ('joint', 8))
    assert d['shoulder_breadth'] == measure.path(('joint', 16), ('joint', 17))
    assert 'untuned' in measure.default_measurements.__doc__.lower()
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts'])
    assert set(dict(m.named_buffers())) == {'faces', 'face_parts'} and m.faces.dtype == torch.int32 and m.face_parts.dtype == torch.uint8
    assert m.names == tuple(d) and m.needs_joints == 22
    arr, n_points = measure.measure_structs(m.specs, 6890)
    assert n_points == 22 and len(arr) == 15
    assert (arr[0].kind, list(arr[0].anchor), list(arr[0].dir), arr[0].part_mask) == (hipabi.MEASURE_EXTENT, [-1] * 4, [0.0, 1.0, 0.0], 0)
    assert (arr[3].kind, list(arr[3].anchor), arr[3].part_mask) == (hipabi.MEASURE_GIRTH, [6890 + 9, -1, -1, -1], 1 << 6)
    assert (arr[10].kind, list(arr[10].anchor)) == (hipabi.MEASURE_PATH, [6890 + 16, 6890 + 18, 6890 + 20, -1])
    assert measure.volume(parts=[6, 1, 6], about=7) == measure.Spec(hipabi.MEASURE_VOLUME, (7,), (0.0, 0.0, 0.0), (1, 6))

    class FakeSmpl:
        faces, face_parts = model['faces'], model['face_parts']
    fs = straps_amd.BodyMeasurer.from_smpl(FakeSmpl, {'waist': measure.girth(100, (0, 1, 0), parts=(6,))})
    assert fs.names == ('waist',) and fs.needs_joints == 0 and torch.equal(fs.faces, m.faces) and torch.equal(fs.face_parts, m.face_parts)
    for bad in (lambda: measure.path(1), lambda: measure.path(1, 2, 3, 4, 5), lambda: measure.girth(-1, (0, 1, 0)), lambda: measure.girth(('bone', 1), (0, 1, 0)),
                lambda: measure.girth(3, (0, 0, 0)), lambda: measure.extent((1, 2)), lambda: measure.area(parts=[32]), lambda: measure.area(parts=[]),
                lambda: measure.girth(('joint', 64), (0, 1, 0)), lambda: measure.extent((0, float('nan'), 0))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(RuntimeError, match='face_parts'):
        straps_amd.BodyMeasurer(model['faces'], None)                                      # the defaults select parts
    assert straps_amd.BodyMeasurer(model['faces'], None, {'v': measure.volume()}).face_parts is None
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'][:-1])
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'].reshape(-1), model['face_parts'])
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], {})
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], [('m%d' % i, measure.area()) for i in range(33)])
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], [('a', measure.area()), ('a', measure.volume())])
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], {'values': measure.area()})
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], {'a': (1, 2, 3)})
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m(torch.zeros(2, 6890, 3), torch.zeros(2, 24, 3))                                  # CPU tensors: no fallback
