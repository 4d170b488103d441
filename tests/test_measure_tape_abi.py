"""CPU: the entry points of csrc/measure_tape.hip are declared, exported and bound alike, the tape struct equals its ctypes mirror, every
argument check answers before any HIP call (no GPU here) and names the argument, the workspace size is the documented one, the Python
surface refuses what it must -- and straps_measure_mesh is what it was: five kinds, kind 5 unknown."""
import ctypes as C
import os
import re

import pytest

import straps_amd
from straps_amd import hipabi, measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_measure_tape_workspace_bytes', 'straps_measure_tape')
EINVAL = 1
MAXF = 0x7fffffff // 3


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def _header():
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    return txt, re.sub(r'/\*.*?\*/', '', txt, flags=re.S)


def test_header_exports_and_prototypes_agree(lib):
    txt, plain = _header()
    assert int(re.search(r'#define STRAPS_ABI_VERSION (\d+)', txt).group(1)) == 12 == hipabi.ABI_VERSION == lib.straps_abi_version()      # added without a version change
    for n in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % n, plain)
        assert decl, '%s is not declared' % n
        assert hasattr(lib, n), '%s is not exported' % n
        res, args = hipabi.SIGNATURES[n]
        assert len([a for a in decl.group(1).split(',') if a.strip()]) == len(args), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res
    assert len(hipabi.SIGNATURES['straps_measure_tape'][1]) == 15 and hipabi.SIGNATURES['straps_measure_tape'][0] is C.c_int
    assert hipabi.SIGNATURES['straps_measure_tape'][1][4] == C.POINTER(hipabi.TapeStruct)
    assert hipabi.SIGNATURES['straps_measure_tape_workspace_bytes'] == (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_int])
    assert 'measure_tape.hip' in hipabi.SOURCES and 'measure.hip' in hipabi.SOURCES
    kinds = re.search(r'enum \{([^}]*STRAPS_TAPE_HULL[^}]*)\}', plain).group(1)
    assert dict((k.strip(), int(v)) for k, v in (e.split('=') for e in kinds.split(','))) == {'STRAPS_TAPE_HULL': hipabi.TAPE_HULL, 'STRAPS_TAPE_SECTION': hipabi.TAPE_SECTION}
    assert (hipabi.TAPE_HULL, hipabi.TAPE_SECTION) == (0, 1)
    assert all(hasattr(straps_amd, n) for n in ('BodyMeasurer', 'default_measurements', 'tape_measurements', 'posed_measurements', 'measure', 'Predictor'))
    assert all(hasattr(measure, n) for n in ('tape_girth', 'section_girth', 'tape_structs')) and hasattr(straps_amd.BodyMeasurer, 'measure_counts')
    src = open(os.path.join(hipabi.CSRC, 'measure_tape.hip')).read()
    assert int(re.search(r'MT_FACES_PER_BLOCK = (\d+);', src).group(1)) == hipabi.MEASURE_TAPE_FACES_PER_BLOCK
    assert 'STRAPS_NO_PACKED_FP32' in src and src.count('__global__') == 2 == src.count('STRAPS_NO_PACKED_FP32 void')


def test_the_mesh_entry_point_is_unchanged(lib):
    """five kinds and no sixth; the workspace formula of straps_measure_mesh"""
    _, plain = _header()
    kinds = re.search(r'enum \{([^}]*STRAPS_MEASURE_VOLUME[^}]*)\}', plain).group(1)
    assert [e.split('=')[0].strip() for e in kinds.split(',')] == ['STRAPS_MEASURE_VOLUME', 'STRAPS_MEASURE_AREA', 'STRAPS_MEASURE_EXTENT', 'STRAPS_MEASURE_GIRTH',
                                                                   'STRAPS_MEASURE_PATH']
    arr = (hipabi.MeasureStruct * 1)()
    p = lambda v: C.c_void_p(v)
    for kind in (5, 6, measure.TAPE_KINDS[0], measure.TAPE_KINDS[1]):
        arr[0].kind = kind
        arr[0].anchor[:] = [0, -1, -1, -1]
        arr[0].dir[:] = (0.0, 1.0, 0.0)
        assert lib.straps_measure_mesh(p(8192), p(8192), p(8192), p(8192), arr, p(8192), p(8192), 2, 6890, 24, 13776, 1, None) == EINVAL
        assert '`meas[0].kind`' in lib.straps_last_error().decode() and 'unknown' in lib.straps_last_error().decode()
    assert lib.straps_measure_workspace_bytes(64, 6890, 13776, 15) == 64 * 15 * 8 * (27 + 2 * 4)
    assert C.sizeof(hipabi.MeasureStruct) == 36


def test_struct_equals_its_mirror():
    _, plain = _header()
    body = re.search(r'typedef struct \{([^}]*)\} straps_tape_t;', plain).group(1)
    ctype = {'float': C.c_float, 'int32_t': C.c_int32, 'uint32_t': C.c_uint32}
    fields = []
    for decl in body.split(';'):
        if decl.strip():
            typ, name = decl.split()
            m = re.match(r'(\w+)\[(\d+)\]$', name)
            fields.append((m.group(1), ctype[typ] * int(m.group(2))) if m else (name, ctype[typ]))
    assert [f[0] for f in fields] == ['kind', 'anchor', 'dir', 'part_mask']
    mirror = hipabi.TapeStruct._fields_
    assert [f[0] for f in mirror] == [f[0] for f in fields]
    for (name, want), (_, got) in zip(fields, mirror):
        assert C.sizeof(want) == C.sizeof(got) and getattr(want, '_length_', 1) == getattr(got, '_length_', 1), name
        assert getattr(want, '_type_', want) == getattr(got, '_type_', got), name
    S = hipabi.TapeStruct
    assert C.sizeof(S) == 28 == 7 * 4 == sum(C.sizeof(t) for _, t in fields)      # seven words, no padding
    assert (S.kind.offset, S.anchor.offset, S.dir.offset, S.part_mask.offset) == (0, 4, 12, 24)
    assert C.sizeof(S * 32) == 32 * 28


def test_workspace_formula(lib):
    ws = lib.straps_measure_tape_workspace_bytes
    for B, F, M, cap in ((1, 1, 1, 0), (1, 1, 1, 2), (3, 65, 32, 0), (3, 65, 32, 130), (3, 65, 32, 2), (3, 65, 32, 7), (64, 13776, 7, 0), (64, 13776, 7, 4096),
                         (1, MAXF, 1, 0), (1 << 20, 13776, 32, 2), ((1 << 26) - 1, 12, 32, 0)):
        assert ws(B, F, M, cap) == B * M * 8 * (2 + 2 * (cap if cap else 2 * F)), (B, F, M, cap)
    assert ws(64, 13776, 7, 0) == 64 * 7 * 8 * (2 + 2 * 27552)
    for bad in ((0, 13776, 7, 0), (-1, 13776, 7, 0), (1 << 31, 13776, 7, 0), (4, 0, 7, 0), (4, -3, 7, 0), (4, MAXF + 1, 7, 0), (4, 13776, 0, 0), (4, 13776, 33, 0),
                (4, 13776, -1, 0), (4, 13776, 7, 1), (4, 13776, 7, -2), (4, 13776, 7, 2 * 13776 + 1), (1 << 26, 12, 32, 0), (1 << 30, MAXF, 32, 0)):
        assert ws(*bad) == 0, bad


def _meas(*items):
    arr = (hipabi.TapeStruct * len(items))()
    for q, (kind, anchor, direction, mask) in zip(arr, items):
        q.kind = kind
        q.anchor[:] = list(anchor) + [-1] * (2 - len(anchor))
        q.dir[:] = direction
        q.part_mask = mask
    return arr


Y = (0.0, 1.0, 0.0)
GOOD = ((hipabi.TAPE_HULL, (6890 + 3,), Y, 1 << 6), (hipabi.TAPE_SECTION, (17,), Y, 0), (hipabi.TAPE_HULL, (6890 + 4, 6890 + 1), (0.0, 0.0, 0.0), 0))


def test_argument_validation_without_gpu(lib):
    """every failure returns STRAPS_EINVAL before any HIP call (the device pointers are never dereferenced) and names the argument"""
    err = lambda: lib.straps_last_error().decode()
    p = lambda v: C.c_void_p(v)
    A = 8192

    def call(verts=A, points=A, faces=A, face_parts=A, meas=GOOD, out=A, counts=A, ws=A, batch=2, nv=6890, n_points=24, nf=13776, n_meas=None, cap=0, meas_null=False):
        arr = _meas(*meas) if meas else None
        return lib.straps_measure_tape(p(verts), p(points), p(faces), p(face_parts), None if meas_null else arr, p(out), p(counts), p(ws), batch, nv, n_points, nf,
                                       len(meas) if n_meas is None else n_meas, cap, None)
    for name, text in (('verts', 'verts'), ('faces', 'faces'), ('out', 'out'), ('ws', 'workspace')):
        assert call(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err() and 'straps_measure_tape' in err(), name
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
    for nf in (-1, 0, MAXF + 1):
        assert call(nf=nf) == EINVAL and '`nfaces`' in err(), nf
    for cap in (1, -1, 2 * 13776 + 1, 1 << 30):
        assert call(cap=cap) == EINVAL and '`capacity`' in err() and str(cap) in err(), cap
    for kind in (2, 5, -1, measure.TAPE_KINDS[0], 1 << 20):
        assert call(meas=GOOD[:2] + ((kind, (3,), Y, 0),)) == EINVAL and '`meas[2].kind`' in err() and 'unknown' in err(), kind
    assert call(meas=((hipabi.TAPE_HULL, (), Y, 0),)) == EINVAL and '`meas[0]`' in err() and '`anchor[0]`' in err()
    for kind in (hipabi.TAPE_HULL, hipabi.TAPE_SECTION):
        for anchor, where in (((6890 + 24,), 'anchor[0]'), ((-5,), 'anchor[0]'), ((1 << 30,), 'anchor[0]'), ((0, 6890 + 24), 'anchor[1]'), ((0, -2), 'anchor[1]'),
                              ((6890 + 23, 1 << 30), 'anchor[1]')):
            assert call(meas=GOOD[:1] + ((kind, anchor, Y, 0),)) == EINVAL and '`meas[1].%s`' % where in err() and str(anchor[-1]) in err(), (kind, anchor)
        assert call(meas=((kind, (6890,), Y, 0),), n_points=0, points=None) == EINVAL and '`meas[0].anchor[0]`' in err()      # no points: vertices only
        assert call(meas=((kind, (3, 6890), Y, 0),), n_points=0, points=None) == EINVAL and '`meas[0].anchor[1]`' in err()
        assert call(meas=GOOD[1:2] + ((kind, (3,), Y, 1 << 4),), face_parts=None) == EINVAL and '`meas[1].part_mask`' in err() and '`face_parts`' in err(), kind
    assert call(points=None) == EINVAL and '`points`' in err() and 'n_points' in err()
    assert call(batch=(1 << 31) - 1) == EINVAL and 'too large' in err()
    assert call(batch=1 << 26, meas=GOOD * 10 + GOOD[:2]) == EINVAL and 'too large' in err()              # batch * n_meas == 2^31


def test_python_surface_checks_without_gpu():
    import torch
    model = straps_amd.synthetic_smpl_model(0)
    j = lambda k: ('joint', k)
    # spec helpers
    t = measure.tape_girth(j(9), (0, 1, 0), parts=[6])
    assert t == measure.Spec(measure.TAPE_KIND_BASE + hipabi.TAPE_HULL, (j(9),), (0.0, 1.0, 0.0), (6,))
    s = measure.section_girth(100, toward=j(3), parts=(4, 5))
    assert s == measure.Spec(measure.TAPE_KIND_BASE + hipabi.TAPE_SECTION, (100, j(3)), (0.0, 0.0, 0.0), (4, 5))
    assert not set(measure.TAPE_KINDS) & set(range(5)) and len(set(measure.TAPE_KINDS)) == 2
    for helper in (measure.tape_girth, measure.section_girth):
        for bad in (lambda: helper(3), lambda: helper(3, (0, 1, 0), toward=4), lambda: helper(3, (0, 0, 0)), lambda: helper(3, (0, float('inf'), 0)),
                    lambda: helper(-1, (0, 1, 0)), lambda: helper(3, toward=('bone', 1)), lambda: helper(3, toward=j(64)), lambda: helper(3, (0, 1, 0), parts=[32]),
                    lambda: helper(3, toward=-2)):
            with pytest.raises(ValueError):
                bad()
    # the two sets
    d, tm, pm = measure.default_measurements(), measure.tape_measurements(), measure.posed_measurements()
    girths = [n for n, q in d.items() if q.kind == hipabi.MEASURE_GIRTH]
    assert list(tm) == [n.replace('_girth', '_tape_girth') for n in girths] and len(tm) == 7
    for n in girths:
        q, g = tm[n.replace('_girth', '_tape_girth')], d[n]
        assert q.kind == measure.TAPE_KINDS[0] and q.anchors == g.anchors and q.direction == g.direction
        assert q.parts == ((4, 5, 6) if n == 'hip_girth' else g.parts)
    assert all(q.kind == measure.TAPE_KINDS[0] and len(q.anchors) == 2 and q.direction == (0.0, 0.0, 0.0) and q.parts for q in pm.values()) and len(pm) == 8
    assert pm['posed_thigh_girth_l'] == measure.tape_girth(j(4), toward=j(1), parts=(4,)) and pm['posed_forearm_girth_r'] == measure.tape_girth(j(21), toward=j(19), parts=(2,))
    assert 'untuned' in measure.tape_measurements.__doc__.lower() and 'untuned' in measure.posed_measurements.__doc__.lower()
    assert list(d) == list(straps_amd.default_measurements()) and len(d) == 15
    # structs: a tape spec never reaches straps_measure_mesh's struct, and the other way round
    arr, n_points = measure.tape_structs([t, s], 6890)
    assert n_points == 10 and (arr[0].kind, list(arr[0].anchor), list(arr[0].dir), arr[0].part_mask) == (hipabi.TAPE_HULL, [6890 + 9, -1], [0.0, 1.0, 0.0], 1 << 6)
    assert (arr[1].kind, list(arr[1].anchor), arr[1].part_mask) == (hipabi.TAPE_SECTION, [100, 6890 + 3], (1 << 4) | (1 << 5))
    with pytest.raises(ValueError):
        measure.measure_structs([t], 6890)
    with pytest.raises(ValueError):
        measure.tape_structs([measure.girth(3, (0, 1, 0))], 6890)
    # the module: a mix of old and new specs, split by the call that serves them
    mix = [('h', measure.extent((0, 1, 0))), ('tape', t), ('g', measure.girth(j(9), (0, 1, 0), parts=(6,))), ('sec', s), ('vol', measure.volume())]
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts'], mix)
    assert m.names == ('h', 'tape', 'g', 'sec', 'vol') and m.tape_columns == (1, 3) and m.mesh_columns == (0, 2, 4) and m.tape_names == ('tape', 'sec')
    assert m.needs_joints == 10 and m.tape_capacity is None
    assert straps_amd.BodyMeasurer(model['faces'], model['face_parts'], tm, tape_capacity=4096).tape_capacity == 4096
    both = list(d.items()) + list(tm.items()) + list(pm.items())
    assert len(both) == 30 and all(n.startswith('posed_') for n in pm) and len(straps_amd.BodyMeasurer(model['faces'], model['face_parts'], both).tape_columns) == 15
    with pytest.raises(RuntimeError):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], [('m%d' % i, t) for i in range(33)])
    with pytest.raises(RuntimeError, match='face_parts'):
        straps_amd.BodyMeasurer(model['faces'], None, {'t': t})
    with pytest.raises(RuntimeError, match='faces'):
        straps_amd.BodyMeasurer(model['faces'][:0], None, {'t': measure.tape_girth(3, (0, 1, 0))})
    with pytest.raises(RuntimeError, match='unknown kind'):
        straps_amd.BodyMeasurer(model['faces'], model['face_parts'], {'t': t._replace(kind=5)})
    for cap in (1, 0, -4, 2 * 13776 + 1, 2.5, True):
        with pytest.raises(RuntimeError, match='tape_capacity'):
            straps_amd.BodyMeasurer(model['faces'], model['face_parts'], tm, tape_capacity=cap)

    class FakeSmpl:
        faces, face_parts = model['faces'], model['face_parts']
    fs = straps_amd.BodyMeasurer.from_smpl(FakeSmpl, pm, tape_capacity=64)
    assert fs.names == tuple(pm) and fs.needs_joints == 22 and fs.tape_capacity == 64 and fs.mesh_columns == ()
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m(torch.zeros(2, 6890, 3), torch.zeros(2, 24, 3))                                  # CPU tensors: no fallback
    with pytest.raises(RuntimeError, match='GPU tensor'):
        m.measure_counts(torch.zeros(2, 6890, 3), torch.zeros(2, 24, 3))
    import inspect
    assert list(inspect.signature(straps_amd.Predictor.measure).parameters) == ['self', 'out', 'measurer', 'posed']
    assert inspect.signature(straps_amd.Predictor.measure).parameters['posed'].default is False
    assert list(inspect.signature(straps_amd.BodyMeasurer.measure_arrays).parameters) == ['self', 'vertices', 'joints']
