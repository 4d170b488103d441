"""CPU: the entry points of csrc/measure_tape_bwd.hip are declared, exported and bound alike, every argument check answers before any HIP call
(no GPU here) and names the argument, the workspace size is the documented one, and the Python surface is opt-in: without tape_gradients=True
every refusal is the one it was."""
import ctypes as C
import os
import re

import pytest

import straps_amd
from straps_amd import hipabi, measure

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('straps_measure_tape_bwd_workspace_bytes', 'straps_measure_tape_bwd')
EINVAL = 1
MAXF = 0x7fffffff // 3


@pytest.fixture(scope='module')
def lib():
    hipabi.build()
    return hipabi.load()


def formula(B, M, cap):
    """the header's: per (body, measurement) ten doubles, cap (u, v) pairs, cap (g_u, g_v) pairs and ceil(cap / 2) int32 padded to a double"""
    return B * M * 8 * (10 + 4 * cap + ((cap + 1) // 2 + 1) // 2)


def test_header_exports_and_prototypes_agree(lib):
    txt = open(os.path.join(ROOT, 'include', 'straps_hip.h')).read()
    plain = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    assert int(re.search(r'#define STRAPS_ABI_VERSION (\d+)', txt).group(1)) == 12 == hipabi.ABI_VERSION == lib.straps_abi_version()      # added without a version change
    for n in NAMES:
        decl = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % n, plain)
        assert decl, '%s is not declared' % n
        assert hasattr(lib, n), '%s is not exported' % n
        res, args = hipabi.SIGNATURES[n]
        assert len([a for a in decl.group(1).split(',') if a.strip()]) == len(args), n
        assert getattr(lib, n).argtypes == args and getattr(lib, n).restype == res
    assert len(hipabi.SIGNATURES['straps_measure_tape_bwd'][1]) == 22 and hipabi.SIGNATURES['straps_measure_tape_bwd'][1][6] == C.POINTER(hipabi.TapeStruct)
    assert hipabi.SIGNATURES['straps_measure_tape_bwd_workspace_bytes'] == (C.c_size_t, [C.c_longlong, C.c_int, C.c_int, C.c_int, C.c_int])
    assert 'measure_tape_bwd.hip' in hipabi.SOURCES
    src = open(os.path.join(hipabi.CSRC, 'measure_tape_bwd.hip')).read()
    assert int(re.search(r'TB_FACES_PER_BLOCK = (\d+);', src).group(1)) == hipabi.MEASURE_TAPE_FACES_PER_BLOCK
    assert src.count('__global__') == 3 == src.count('STRAPS_NO_PACKED_FP32 void')
    assert 'straps_measure_tape_bwd' in txt and 'have no gradient' not in txt


def test_workspace_formula(lib):
    ws = lib.straps_measure_tape_bwd_workspace_bytes
    for B, N, F, M, cap in ((1, 1, 1, 1, 0), (1, 3, 1, 1, 2), (3, 97, 65, 32, 0), (3, 97, 65, 32, 130), (3, 97, 65, 32, 2), (3, 97, 65, 32, 7), (64, 6890, 13776, 7, 0),
                            (64, 6890, 13776, 7, 4096), (1, 1 << 20, MAXF, 1, 0), (1 << 20, 6890, 13776, 32, 2), ((1 << 26) - 1, 8, 12, 32, 0)):
        assert ws(B, N, F, M, cap) == formula(B, M, cap if cap else 2 * F), (B, N, F, M, cap)
    assert ws(64, 6890, 13776, 7, 0) == 64 * 7 * 8 * (10 + 4 * 27552 + 6888)
    for bad in ((0, 6890, 13776, 7, 0), (-1, 6890, 13776, 7, 0), (1 << 31, 6890, 13776, 7, 0), (4, 0, 13776, 7, 0), (4, (1 << 20) + 1, 13776, 7, 0), (4, 6890, 0, 7, 0),
                (4, 6890, -3, 7, 0), (4, 6890, MAXF + 1, 7, 0), (4, 6890, 13776, 0, 0), (4, 6890, 13776, 33, 0), (4, 6890, 13776, 7, 1), (4, 6890, 13776, 7, -2),
                (4, 6890, 13776, 7, 2 * 13776 + 1), (1 << 26, 8, 12, 32, 0), (1 << 30, 6890, MAXF, 32, 0)):
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

    def call(verts=A, points=A, faces=A, face_parts=A, off=A, vf=A, meas=GOOD, dout=A, dverts=A, dpoints=A, values=A, counts=A, ws=A, batch=2, nv=6890, n_points=24,
             rows=90, nf=13776, n_meas=None, cap=0, acc=0, meas_null=False):
        arr = _meas(*meas) if meas else None
        return lib.straps_measure_tape_bwd(p(verts), p(points), p(faces), p(face_parts), p(off), p(vf), None if meas_null else arr, p(dout), p(dverts), p(dpoints),
                                           p(values), p(counts), p(ws), batch, nv, n_points, rows, nf, len(meas) if n_meas is None else n_meas, cap, acc, None)
    for name, text in (('verts', 'verts'), ('faces', 'faces'), ('off', 'vf_offsets'), ('vf', 'vf_faces'), ('dout', 'dout'), ('dverts', 'dverts'), ('ws', 'workspace')):
        assert call(**{name: None}) == EINVAL and '`%s`' % text in err() and 'null pointer' in err() and 'straps_measure_tape_bwd' in err(), name
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
        assert call(n_points=npts, rows=90) == EINVAL and '`n_points`' in err(), npts
    for rows in (23, 0, -1):
        assert call(rows=rows) == EINVAL and '`dpoints_rows`' in err(), rows
    for nf in (-1, 0, MAXF + 1):
        assert call(nf=nf) == EINVAL and '`nfaces`' in err(), nf
    for cap in (1, -1, 2 * 13776 + 1, 1 << 30):
        assert call(cap=cap) == EINVAL and '`capacity`' in err() and str(cap) in err(), cap
    for acc in (2, -1):
        assert call(acc=acc) == EINVAL and '`accumulate`' in err() and str(acc) in err(), acc
    for kind in (2, 5, -1, measure.TAPE_KINDS[0], 1 << 20):
        assert call(meas=GOOD[:2] + ((kind, (3,), Y, 0),)) == EINVAL and '`meas[2].kind`' in err() and 'unknown' in err(), kind
    assert call(meas=((hipabi.TAPE_HULL, (), Y, 0),)) == EINVAL and '`meas[0]`' in err() and '`anchor[0]`' in err()
    for kind in (hipabi.TAPE_HULL, hipabi.TAPE_SECTION):
        for anchor, where in (((6890 + 24,), 'anchor[0]'), ((-5,), 'anchor[0]'), ((1 << 30,), 'anchor[0]'), ((0, 6890 + 24), 'anchor[1]'), ((0, -2), 'anchor[1]'),
                              ((6890 + 23, 1 << 30), 'anchor[1]')):
            assert call(meas=GOOD[:1] + ((kind, anchor, Y, 0),)) == EINVAL and '`meas[1].%s`' % where in err() and str(anchor[-1]) in err(), (kind, anchor)
        assert call(meas=((kind, (6890,), Y, 0),), n_points=0, points=None) == EINVAL and '`meas[0].anchor[0]`' in err()      # no points: vertices only
        assert call(meas=GOOD[1:2] + ((kind, (3,), Y, 1 << 4),), face_parts=None) == EINVAL and '`meas[1].part_mask`' in err() and '`face_parts`' in err(), kind
    assert call(points=None) == EINVAL and '`points`' in err() and 'n_points' in err()
    assert call(dpoints=None) == EINVAL and '`dpoints`' in err()                                           # an anchor that is read is a point
    assert call(meas=((hipabi.TAPE_HULL, (3, 6890 + 2), Y, 0),), dpoints=None) == EINVAL and '`dpoints`' in err()      # anchor[1] as well
    assert call(batch=(1 << 31) - 1) == EINVAL and 'too large' in err()
    assert call(batch=1 << 26, meas=GOOD * 10 + GOOD[:2]) == EINVAL and 'too large' in err()              # batch * n_meas == 2^31


def test_python_surface_is_opt_in():
    import inspect
    model = straps_amd.synthetic_smpl_model(0)
    tm = measure.tape_measurements()
    m = straps_amd.BodyMeasurer(model['faces'], model['face_parts'], tm)
    assert m.tape_gradients is False and straps_amd.BodyMeasurer(model['faces'], model['face_parts'], tm, tape_gradients=True).tape_gradients is True
    assert inspect.signature(straps_amd.BodyMeasurer.__init__).parameters['tape_gradients'].default is False
    assert inspect.signature(straps_amd.BodyMeasurer.from_smpl).parameters['tape_gradients'].default is False
    assert list(inspect.signature(straps_amd.BodyMeasurer.__init__).parameters)[:6] == ['self', 'faces', 'face_parts', 'measurements', 'tape_capacity', 'num_vertices']

    class FakeSmpl:
        faces, face_parts = model['faces'], model['face_parts']
    assert straps_amd.BodyMeasurer.from_smpl(FakeSmpl, tm, tape_gradients=True).tape_gradients is True and straps_amd.BodyMeasurer.from_smpl(FakeSmpl, tm).tape_gradients is False
    assert all(hasattr(straps_amd.BodyMeasurer, n) for n in ('measure_tape_raw', 'measure_tape_grad_raw', 'tape_workspace_bytes', 'tape_grad_workspace_bytes'))
    import torch
    with pytest.raises(RuntimeError, match='tape'):      # as before: refused before anything touches a device
        m(torch.zeros(2, 6890, 3), torch.zeros(2, 24, 3), differentiable=True)
    with pytest.raises(RuntimeError, match='tape'):
        m.measure_grad(torch.zeros(2, 6890, 3), torch.zeros(2, 24, 3), torch.zeros(2, 7))
    assert list(inspect.signature(straps_amd.Predictor.refine_shape).parameters) == ['self', 'out', 'mfitter', 'targets', 'weights']
