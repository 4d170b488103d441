"""Body measurements of a batch of meshes on the device: height, volume, surface area, girths and limb lengths (csrc/measure.hip,
straps_measure_mesh), and tape-measure girths with the plane's normal given once or taken per body (csrc/measure_tape.hip,
straps_measure_tape); include/straps_hip.h states the definitions.

    measurer = BodyMeasurer.from_smpl(smpl).to(device)            # the tables of the model, default_measurements()
    m = measurer(vertices, joints)                                # {'values': [B,M] float32, 'height': [B], 'volume': [B], ...}
    m = predictor.measure(out, measurer)                          # the predicted body in the T-pose
    tape = BodyMeasurer.from_smpl(smpl, tape_measurements()).to(device)      # what a tape reads: convex hull of the plane section
    posed = BodyMeasurer.from_smpl(smpl, posed_measurements()).to(device)    # limb girths, planes perpendicular to the bone of EACH body
    m = predictor.measure(out, posed, posed=True)                 # the predicted body as posed

A measurement is a spec made by one of the helpers below; `measurements` is a dict name -> spec (or a sequence of (name, spec)), at most 32,
old and new kinds in any mix.  An anchor is an int (a vertex id) or ('joint', j): row j of the `joints` given to the call.  `parts` is an
iterable of part labels (0..31) of the per-face table `face_parts` (this package's labels, synthetic_smpl.JOINT_TO_PART: 1 / 2 left / right
arm, 3 head, 4 / 5 left / right leg, 6 torso); None: every face.

`girth` is the length of the plane section, which follows concavities; `tape_girth` is the perimeter of the section's convex hull, which spans
them as a tape does (the two agree on a convex section); `section_girth` is `girth` with the new plane options.  The plane of the two new
helpers has either a `normal` shared by the batch or `toward`: a second anchor, the normal being that anchor minus the first one on each
body -- a plane perpendicular to a bone, wherever the pose has put it.

All arithmetic is double on fp32 vertices, rounded to float once; results are bit-reproducible and a body's row depends on that body alone.

Gradients (csrc/measure_bwd.hip, straps_measure_mesh_bwd): `measurer(vertices, joints, differentiable=True)` gives the same values with a
gradient to vertices and joints, `measurer.measure_grad(vertices, joints, dvalues)` the gradient itself; fit.MeasurementFitter fits the shape
to known measurements with them.  Tape girths (`tape_girth`, `section_girth`) have one with `BodyMeasurer(..., tape_gradients=True)`
(csrc/measure_tape_bwd.hip, straps_measure_tape_bwd); without it a measurer refuses to differentiate them, as it always did.
"""
import collections
import ctypes as C
import os

import numpy as np
import torch
import torch.nn as nn

from . import config, hipabi

Spec = collections.namedtuple('Spec', ('kind', 'anchors', 'direction', 'parts'))
KIND_NAMES = ('volume', 'area', 'extent', 'girth', 'path')
# Spec.kind of the specs that go to straps_measure_tape: TAPE_KIND_BASE + hipabi.TAPE_*; never a kind of straps_measure_mesh
TAPE_KIND_BASE = 100
TAPE_KINDS = (TAPE_KIND_BASE + hipabi.TAPE_HULL, TAPE_KIND_BASE + hipabi.TAPE_SECTION)


def _anchor(a, what):
    if isinstance(a, (tuple, list)):
        if len(a) != 2 or a[0] != 'joint' or int(a[1]) < 0:
            raise ValueError("%s: an anchor is a vertex id or ('joint', j) (got %r)" % (what, a))
        if int(a[1]) >= hipabi.MEASURE_MAX_POINTS:
            raise ValueError('%s: joint anchors are limited to the first %d joints (got %r)' % (what, hipabi.MEASURE_MAX_POINTS, a))
        return ('joint', int(a[1]))
    if isinstance(a, (bool, float)) or int(a) != a or int(a) < 0:
        raise ValueError("%s: an anchor is a vertex id or ('joint', j) (got %r)" % (what, a))
    return int(a)


def _direction(d, what):
    d = tuple(float(x) for x in np.asarray(d, np.float64).reshape(-1))
    if len(d) != 3 or not np.isfinite(d).all() or not any(d):
        raise ValueError('%s: a direction is three finite numbers, not all zero (got %r)' % (what, d))
    return d


def _parts(parts, what):
    if parts is None:
        return None
    parts = tuple(sorted(set(int(p) for p in parts)))
    if not parts or parts[0] < 0 or parts[-1] > 31:
        raise ValueError('%s: part labels are 0..31, at least one (got %r)' % (what, parts))
    return parts


def volume(parts=None, about=None):
    """signed volume (1/6) sum q0 . (q1 x q2) of the selected faces, corners relative to the anchor `about` (None: the origin).  The choice of
    `about` does not matter for a closed surface; for an open part it closes the part with a cone to that point."""
    return Spec(hipabi.MEASURE_VOLUME, () if about is None else (_anchor(about, 'measure.volume'),), (0.0, 0.0, 0.0), _parts(parts, 'measure.volume'))


def area(parts=None):
    """surface area of the selected faces"""
    return Spec(hipabi.MEASURE_AREA, (), (0.0, 0.0, 0.0), _parts(parts, 'measure.area'))


def extent(axis):
    """max - min of axis . p over all vertices (axis is not normalised)"""
    return Spec(hipabi.MEASURE_EXTENT, (), _direction(axis, 'measure.extent'), None)


def girth(anchor, normal, parts=None):
    """length of the section of the selected faces with the plane through `anchor` with normal `normal`"""
    return Spec(hipabi.MEASURE_GIRTH, (_anchor(anchor, 'measure.girth'),), _direction(normal, 'measure.girth'), _parts(parts, 'measure.girth'))


def path(*anchors):
    """length of the polyline through two to four anchors"""
    if not 2 <= len(anchors) <= 4:
        raise ValueError('measure.path: two to four anchors (got %d)' % len(anchors))
    return Spec(hipabi.MEASURE_PATH, tuple(_anchor(a, 'measure.path') for a in anchors), (0.0, 0.0, 0.0), None)


def _tape_spec(what, kind, anchor, normal, parts, toward):
    if (normal is None) == (toward is None):
        raise ValueError('%s: give exactly one of normal= (shared by the batch) and toward= (a second anchor: the normal per body)' % what)
    if toward is None:
        return Spec(TAPE_KIND_BASE + kind, (_anchor(anchor, what),), _direction(normal, what), _parts(parts, what))
    return Spec(TAPE_KIND_BASE + kind, (_anchor(anchor, what), _anchor(toward, what)), (0.0, 0.0, 0.0), _parts(parts, what))


def tape_girth(anchor, normal=None, parts=None, toward=None):
    """what a tape reads: the perimeter of the convex hull of the section of the selected faces with the plane through `anchor`; its normal
    is `normal`, or on each body the anchor `toward` minus `anchor`"""
    return _tape_spec('measure.tape_girth', hipabi.TAPE_HULL, anchor, normal, parts, toward)


def section_girth(anchor, normal=None, parts=None, toward=None):
    """length of the section (what `girth` gives) with the plane of `tape_girth`: `normal`, or `toward` for a normal per body"""
    return _tape_spec('measure.section_girth', hipabi.TAPE_SECTION, anchor, normal, parts, toward)


def default_measurements():
    """The default set, anchored at SMPL's public joint numbering (0 pelvis, 1 / 2 hips, 3 spine1, 4 / 5 knees, 7 / 8 ankles, 9 spine3, 16 / 17
    shoulders, 18 / 19 elbows, 20 / 21 wrists) and this package's part labels, for T-pose bodies (y up, arms along x):

        height               extent along y
        volume, surface_area the whole mesh
        chest_girth          plane through joint 9, normal y, torso          waist_girth   joint 3          hip_girth   joint 0
        thigh_girth_l / _r   plane with normal y through the KNEE joint (4 / 5), leg parts: the leg's section at the knee's height.  Joints 1 / 2
                             (the hip joints) lie at the top of the leg part, where the section runs into the torso boundary; the knee is the
                             joint that lies inside the leg part on every body, so the section is a closed loop of leg faces
        upper_arm_girth_l/_r plane with normal x through the elbow joint (18 / 19), arm parts
        arm_length_l / _r    paths 16-18-20 and 17-19-21            leg_length_l / _r   paths 1-4-7 and 2-5-8
        shoulder_breadth     path 16-17

    These positions are UNTUNED on the real model: no SMPL file was available when they were chosen, only the synthetic stand-in, whose
    triangle soup is not a body surface.  Check them on your model (and move a plane along a limb with your own specs) before relying on
    absolute numbers.  The fit defaults carry the same warning."""
    j = lambda k: ('joint', k)
    y, x = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    return collections.OrderedDict([
        ('height', extent(y)), ('volume', volume()), ('surface_area', area()),
        ('chest_girth', girth(j(9), y, parts=(6,))), ('waist_girth', girth(j(3), y, parts=(6,))), ('hip_girth', girth(j(0), y, parts=(6,))),
        ('thigh_girth_l', girth(j(4), y, parts=(4,))), ('thigh_girth_r', girth(j(5), y, parts=(5,))),
        ('upper_arm_girth_l', girth(j(18), x, parts=(1,))), ('upper_arm_girth_r', girth(j(19), x, parts=(2,))),
        ('arm_length_l', path(j(16), j(18), j(20))), ('arm_length_r', path(j(17), j(19), j(21))),
        ('leg_length_l', path(j(1), j(4), j(7))), ('leg_length_r', path(j(2), j(5), j(8))),
        ('shoulder_breadth', path(j(16), j(17)))])


def tape_measurements():
    """The seven girths of default_measurements() as tape girths, for T-pose bodies (y up, arms along x):

        chest_tape_girth, waist_tape_girth       planes through joints 9 and 3, normal y, torso
        hip_tape_girth                           plane through joint 0, normal y, torso AND both leg parts: the tape spans the two thighs
        thigh_tape_girth_l / _r                  normal y through the knee joint (4 / 5), the leg part of that side
        upper_arm_tape_girth_l / _r              normal x through the elbow joint (18 / 19), the arm part of that side

    These positions are UNTUNED on the real model, as those of default_measurements() are and for the same reason: only the synthetic
    stand-in was available, whose triangle soup is not a body surface.  Check them on your model before relying on absolute numbers."""
    j = lambda k: ('joint', k)
    y, x = (0.0, 1.0, 0.0), (1.0, 0.0, 0.0)
    return collections.OrderedDict([
        ('chest_tape_girth', tape_girth(j(9), y, parts=(6,))), ('waist_tape_girth', tape_girth(j(3), y, parts=(6,))),
        ('hip_tape_girth', tape_girth(j(0), y, parts=(4, 5, 6))),
        ('thigh_tape_girth_l', tape_girth(j(4), y, parts=(4,))), ('thigh_tape_girth_r', tape_girth(j(5), y, parts=(5,))),
        ('upper_arm_tape_girth_l', tape_girth(j(18), x, parts=(1,))), ('upper_arm_tape_girth_r', tape_girth(j(19), x, parts=(2,)))])


def posed_measurements():
    """Limb tape girths for bodies in ANY pose: every plane passes through a joint and is perpendicular to the bone towards the neighbouring
    joint of that body (`toward=`), so it turns with the limb:

        posed_thigh_girth_l / _r         through the knee (4 / 5) toward the hip joint (1 / 2), leg part
        posed_calf_girth_l / _r          through the ankle (7 / 8) toward the knee (4 / 5), leg part
        posed_upper_arm_girth_l / _r     through the elbow (18 / 19) toward the shoulder (16 / 17), arm part
        posed_forearm_girth_l / _r       through the wrist (20 / 21) toward the elbow (18 / 19), arm part

    Give the call the posed joints (Predictor.measure(out, measurer, posed=True) does).  These positions are UNTUNED on the real model, as
    those of default_measurements() are: a plane through a joint is where the part ends or bends, and a plane further along the bone needs a
    vertex anchor of your model."""
    j = lambda k: ('joint', k)
    return collections.OrderedDict([
        ('posed_thigh_girth_l', tape_girth(j(4), toward=j(1), parts=(4,))), ('posed_thigh_girth_r', tape_girth(j(5), toward=j(2), parts=(5,))),
        ('posed_calf_girth_l', tape_girth(j(7), toward=j(4), parts=(4,))), ('posed_calf_girth_r', tape_girth(j(8), toward=j(5), parts=(5,))),
        ('posed_upper_arm_girth_l', tape_girth(j(18), toward=j(16), parts=(1,))), ('posed_upper_arm_girth_r', tape_girth(j(19), toward=j(17), parts=(2,))),
        ('posed_forearm_girth_l', tape_girth(j(20), toward=j(18), parts=(1,))), ('posed_forearm_girth_r', tape_girth(j(21), toward=j(19), parts=(2,)))])


def tape_structs(specs, nverts):
    """-> (hipabi.TapeStruct array, number of points the specs read) for specs of tape_girth / section_girth"""
    arr = (hipabi.TapeStruct * len(specs))()
    n_points = 0
    for q, s in zip(arr, specs):
        if s.kind not in TAPE_KINDS:
            raise ValueError('measure.tape_structs: %r is not a spec of measure.tape_girth / section_girth' % (s,))
        q.kind = s.kind - TAPE_KIND_BASE
        q.anchor[:] = [-1, -1]
        for i, a in enumerate(s.anchors):
            if isinstance(a, tuple):
                q.anchor[i] = nverts + a[1]
                n_points = max(n_points, a[1] + 1)
            else:
                q.anchor[i] = a
        q.dir[:] = s.direction
        q.part_mask = sum(1 << p for p in s.parts) if s.parts else 0
    return arr, n_points


def measure_structs(specs, nverts):
    """-> (hipabi.MeasureStruct array, number of points the specs read): ('joint', j) anchors resolve to nverts + j"""
    arr = (hipabi.MeasureStruct * len(specs))()
    n_points = 0
    for q, s in zip(arr, specs):
        if s.kind not in range(len(KIND_NAMES)):      # (a tape spec goes to straps_measure_tape: tape_structs)
            raise ValueError('measure.measure_structs: %r is not a spec of measure.volume / area / extent / girth / path' % (s,))
        q.kind = s.kind
        q.anchor[:] = [-1, -1, -1, -1]
        for i, a in enumerate(s.anchors):
            if isinstance(a, tuple):
                q.anchor[i] = nverts + a[1]
                n_points = max(n_points, a[1] + 1)
            else:
                q.anchor[i] = a
        q.dir[:] = s.direction
        q.part_mask = sum(1 << p for p in s.parts) if s.parts else 0
    return arr, n_points


class BodyMeasurer(nn.Module):
    """Measures a batch of meshes of one topology (see the module docstring).  faces [F,3] and face_parts [F] (None: no spec may name parts) are
    held as buffers; faces=None loads config.SMPL_FACES_PATH, and then the part table from the reference's texture files, as NMRRenderer does.
    measurements=None: default_measurements().  Specs of tape_girth / section_girth go to straps_measure_tape, the others to
    straps_measure_mesh (a call without specs of one sort is not made); `values` holds the columns in the order of `names`.  tape_capacity:
    the section points per (body, tape measurement) that the workspace holds, None: the worst case, 2 * faces.  A tape girth of a body
    that cuts more is NaN; measure_counts tells how many there were.  num_vertices: the vertex count of the meshes that measure_grad will get,
    for the vertex-to-face table of the gradient's gather (`vf_offsets` / `vf_faces`, nmr_renderer.vertex_face_table, built here once and moved
    with the module);
    None: the highest index in `faces` + 1, which is wrong only when the last vertices are in no face (from_smpl passes the model's count).
    tape_gradients=True: measure_grad, forward(differentiable=True) and fit.MeasurementFitter also serve the tape specs
    (straps_measure_tape_bwd); the default refuses them, as it always did."""

    def __init__(self, faces=None, face_parts=None, measurements=None, tape_capacity=None, num_vertices=None, tape_gradients=False):
        super().__init__()
        name = 'BodyMeasurer'
        if faces is None:
            if not os.path.isfile(config.SMPL_FACES_PATH):
                raise RuntimeError('%s: %s not found; pass faces= (e.g. from synthetic_smpl_model()) or use from_smpl' % (name, config.SMPL_FACES_PATH))
            faces = np.load(config.SMPL_FACES_PATH)
            if face_parts is None and os.path.isfile(config.VERTEX_TEXTURE_PATH) and os.path.isfile(config.CUBE_PARTS_PATH):
                from .nmr_renderer import face_parts_from_texture
                face_parts = face_parts_from_texture(np.load(config.VERTEX_TEXTURE_PATH), np.load(config.CUBE_PARTS_PATH))
        as_numpy = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        faces = np.ascontiguousarray(as_numpy(faces).astype(np.int32))
        if faces.ndim != 2 or faces.shape[1] != 3:
            raise RuntimeError('%s: faces must be [F,3] (got %s)' % (name, faces.shape))
        self.register_buffer('faces', torch.from_numpy(faces))
        if face_parts is not None:
            face_parts = np.ascontiguousarray(as_numpy(face_parts).astype(np.uint8))
            if face_parts.shape != (faces.shape[0],):
                raise RuntimeError('%s: face_parts must be [%d] (got %s)' % (name, faces.shape[0], face_parts.shape))
            face_parts = torch.from_numpy(face_parts)
        self.register_buffer('face_parts', face_parts)
        measurements = default_measurements() if measurements is None else measurements
        items = list(measurements.items()) if hasattr(measurements, 'items') else [tuple(m) for m in measurements]
        if not 1 <= len(items) <= hipabi.MEASURE_MAX:
            raise RuntimeError('%s: 1 to %d measurements (got %d)' % (name, hipabi.MEASURE_MAX, len(items)))
        self.names = tuple(str(n) for n, _ in items)
        self.specs = tuple(s for _, s in items)
        if len(set(self.names)) != len(self.names) or 'values' in self.names:
            raise RuntimeError("%s: measurement names must be distinct and none may be 'values' (got %r)" % (name, self.names))
        for n, s in items:
            if not isinstance(s, Spec):
                raise RuntimeError('%s: measurement %r is not a spec of measure.volume / area / extent / girth / path / tape_girth / section_girth (got %r)'
                                   % (name, n, s))
            if s.parts and face_parts is None:
                raise RuntimeError('%s: measurement %r selects parts %r but no face_parts table was given' % (name, n, s.parts))
            if s.kind not in range(len(KIND_NAMES)) and s.kind not in TAPE_KINDS:
                raise RuntimeError('%s: measurement %r has the unknown kind %r' % (name, n, s.kind))
            if s.kind in (hipabi.MEASURE_VOLUME, hipabi.MEASURE_AREA, hipabi.MEASURE_GIRTH) + TAPE_KINDS and faces.shape[0] == 0:
                raise RuntimeError('%s: measurement %r reads faces but the face table is empty' % (name, n))
        self.needs_joints = max([a[1] + 1 for s in self.specs for a in s.anchors if isinstance(a, tuple)] or [0])
        # columns of `values` that each library call fills, in the order of `names`
        self.tape_columns = tuple(i for i, s in enumerate(self.specs) if s.kind in TAPE_KINDS)
        self.mesh_columns = tuple(i for i, s in enumerate(self.specs) if s.kind not in TAPE_KINDS)
        self.tape_names = tuple(self.names[i] for i in self.tape_columns)
        if tape_capacity is not None:
            if isinstance(tape_capacity, (bool, float)) or int(tape_capacity) != tape_capacity or not 2 <= int(tape_capacity) <= 2 * max(1, faces.shape[0]):
                raise RuntimeError('%s: tape_capacity is None (the worst case) or a number of section points in 2..2 * faces = %d (got %r)'
                                   % (name, 2 * faces.shape[0], tape_capacity))
            tape_capacity = int(tape_capacity)
        self.tape_capacity = tape_capacity
        self.tape_gradients = bool(tape_gradients)
        # the CSR vertex-to-face table of the gradient's gather (straps_measure_mesh_bwd), built once.  Derived from `faces`, so neither in the
        # state dict nor among named_buffers(): plain tensors that _apply moves with the module
        from .nmr_renderer import vertex_face_table
        self.num_vertices = int(num_vertices) if num_vertices is not None else max(1, int(faces.max()) + 1 if faces.size else 1)
        vf_offsets, vf_faces = vertex_face_table(faces, self.num_vertices)
        self.vf_offsets, self.vf_faces = torch.from_numpy(vf_offsets), torch.from_numpy(vf_faces)
        self._structs = {}
        self._tape_structs = {}

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        self.vf_offsets, self.vf_faces = fn(self.vf_offsets), fn(self.vf_faces)
        return self

    @classmethod
    def from_smpl(cls, smpl, measurements=None, tape_capacity=None, tape_gradients=False):
        """the face and part tables of an SMPL module (its `.faces` / `.face_parts`: the model file's, or the synthetic model's)"""
        if getattr(smpl, 'faces', None) is None:
            raise RuntimeError('BodyMeasurer.from_smpl: the SMPL model carries no faces; pass faces= (and face_parts=) to BodyMeasurer')
        nv = getattr(smpl, 'v_template', None)
        return cls(smpl.faces, getattr(smpl, 'face_parts', None), measurements, tape_capacity, None if nv is None else nv.shape[0], tape_gradients)

    @hipabi.on_tensor_device
    def measure_arrays(self, vertices, joints=None):
        """vertices [B,N,3], joints None or [B,J,3] (fp32 GPU) -> values [B,M] float32.  Never synchronises; runs on the current stream;
        capturable."""
        return self._measure(vertices, joints, False)

    @hipabi.on_tensor_device
    def measure_counts(self, vertices, joints=None):
        """-> int32 [B, n_tape]: the section points (2 x the cut faces) of every tape_girth / section_girth, in the order of `tape_names`,
        whatever tape_capacity is: a count above it is a NaN tape girth.  Runs the tape call alone; never synchronises."""
        return self._measure(vertices, joints, True)

    def _checked_inputs(self, vertices, joints):
        """the checks every call makes -> (vertices detached and contiguous, points [B,needs_joints,3] or None, B, N)"""
        name = 'BodyMeasurer'
        hipabi.require_gpu_tensor(vertices, 'vertices', torch.float32)
        hipabi.require_gpu_tensor(self.faces, name + ' buffers (call .to(device))', torch.int32)
        if vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[0] < 1 or vertices.shape[1] < 1:
            raise RuntimeError('%s: expected vertices [B,N,3], got %s' % (name, tuple(vertices.shape)))
        B, N = vertices.shape[0], vertices.shape[1]
        points = None
        if self.needs_joints:
            if joints is None:
                raise RuntimeError("%s: the measurements %r are anchored at joints: pass joints [B,J,3] with J >= %d"
                                   % (name, [n for n, s in zip(self.names, self.specs) if any(isinstance(a, tuple) for a in s.anchors)], self.needs_joints))
            hipabi.require_gpu_tensor(joints, 'joints', torch.float32)
            if joints.dim() != 3 or joints.shape[0] != B or joints.shape[2] != 3 or joints.shape[1] < self.needs_joints:
                raise RuntimeError('%s: joints must be [%d,J,3] with J >= %d, got %s' % (name, B, self.needs_joints, tuple(joints.shape)))
            points = joints.detach()[:, :self.needs_joints].contiguous()           # (the library takes at most 64 points: the leading joints that are read)
        for n, s in zip(self.names, self.specs):
            for a in s.anchors:
                if not isinstance(a, tuple) and a >= N:
                    raise RuntimeError('%s: measurement %r is anchored at vertex %d, the mesh has %d' % (name, n, a, N))
        return vertices.detach().contiguous(), points, B, N

    def _measure(self, vertices, joints, want_counts):
        name = 'BodyMeasurer'
        vertices, points, B, N = self._checked_inputs(vertices, joints)
        L = hipabi.lib()
        F = self.faces.shape[0]
        # both calls get the SAME points tensor, [B, needs_joints, 3]: its row count is the stride by which they find a body's points, whatever the
        # highest joint that the specs of one call alone read
        n_points = self.needs_joints
        out = tape_out = counts = None
        if self.mesh_columns and not want_counts:
            if N not in self._structs:
                self._structs[N] = measure_structs([self.specs[i] for i in self.mesh_columns], N)
            arr = self._structs[N][0]
            M = len(self.mesh_columns)
            out = torch.empty(B, M, device=vertices.device, dtype=torch.float32)
            ws = torch.empty(L.straps_measure_workspace_bytes(B, N, F, M) // 8, device=vertices.device, dtype=torch.float64)
            hipabi.check(L.straps_measure_mesh(hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces) if F else None, hipabi.ptr(self.face_parts), arr,
                                               hipabi.ptr(out), hipabi.ptr(ws), B, N, n_points, F, M, hipabi.stream_ptr()), 'straps_measure_mesh')
        if self.tape_columns:
            if N not in self._tape_structs:
                self._tape_structs[N] = tape_structs([self.specs[i] for i in self.tape_columns], N)
            arr = self._tape_structs[N][0]
            T, cap = len(self.tape_columns), self.tape_capacity or 0
            ws_bytes = L.straps_measure_tape_workspace_bytes(B, F, T, cap)
            if not ws_bytes:
                raise RuntimeError('%s: no tape workspace for batch %d, %d faces, %d tape measurements, capacity %d' % (name, B, F, T, cap))
            tape_out = torch.empty(B, T, device=vertices.device, dtype=torch.float32)
            if want_counts:
                counts = torch.empty(B, T, device=vertices.device, dtype=torch.int32)
            ws = torch.empty(ws_bytes // 8, device=vertices.device, dtype=torch.float64)
            hipabi.check(L.straps_measure_tape(hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces), hipabi.ptr(self.face_parts), arr,
                                               hipabi.ptr(tape_out), hipabi.ptr(counts), hipabi.ptr(ws), B, N, n_points, F, T, cap, hipabi.stream_ptr()),
                         'straps_measure_tape')
        if want_counts:
            return counts if counts is not None else torch.empty(B, 0, device=vertices.device, dtype=torch.int32)
        if tape_out is None:
            return out
        if out is None:
            return tape_out
        src = {i: out[:, k] for k, i in enumerate(self.mesh_columns)}
        src.update({i: tape_out[:, k] for k, i in enumerate(self.tape_columns)})
        return torch.stack([src[i] for i in range(len(self.specs))], 1)

    @hipabi.on_tensor_device
    def measure_grad(self, vertices, joints, dvalues):
        """the gradient of sum(dvalues * values) w.r.t. the inputs of measure_arrays (straps_measure_mesh_bwd; include/straps_hip.h defines it at
        ties and degenerate terms): vertices [B,N,3], joints None or [B,J,3], dvalues [B,M] in the order of `names`
        -> (dvertices [B,N,3], djoints [B,J,3] or None without joints; rows of joints that no spec reads are zero).  Tape girths have a
        gradient with tape_gradients=True (straps_measure_tape_bwd, added onto the other kinds' in the same buffers; a call without specs
        of one sort is not made).  Without it a non-zero dvalues column of a tape spec raises (that check reads the device, and is made
        only when there are tape specs).  Otherwise never synchronises; capturable."""
        name = 'BodyMeasurer.measure_grad'
        if not self.mesh_columns and not self.tape_gradients:
            raise RuntimeError('%s: every measurement is a tape girth: straps_measure_tape has no gradient without tape_gradients=True' % name)
        vertices, points, B, N = self._checked_inputs(vertices, joints)
        hipabi.require_gpu_tensor(dvalues, 'dvalues', torch.float32)
        if tuple(dvalues.shape) != (B, len(self.specs)):
            raise RuntimeError('%s: dvalues must be [%d,%d], got %s' % (name, B, len(self.specs), tuple(dvalues.shape)))
        if N != self.num_vertices:
            raise RuntimeError('%s: the vertex-to-face table was built for %d vertices, the mesh has %d (BodyMeasurer(..., num_vertices=))' % (name, self.num_vertices, N))
        dvalues = dvalues.detach()
        tape_dvalues = None
        if self.tape_columns:
            if self.tape_gradients:
                tape_dvalues = dvalues[:, list(self.tape_columns)].contiguous()
            elif bool((dvalues[:, list(self.tape_columns)] != 0).any()):
                raise RuntimeError('%s: dvalues is non-zero in a column of %r: tape girths (straps_measure_tape) have no gradient without tape_gradients=True'
                                   % (name, list(self.tape_names)))
            dvalues = dvalues[:, list(self.mesh_columns)]
        dvalues = dvalues.contiguous()
        dverts = torch.empty(B, N, 3, device=vertices.device, dtype=torch.float32)
        djoints = None if joints is None else torch.zeros(B, joints.shape[1], 3, device=vertices.device, dtype=torch.float32)
        if self.mesh_columns:
            ws = torch.empty(hipabi.lib().straps_measure_bwd_workspace_bytes(B, N, self.faces.shape[0], len(self.mesh_columns)) // 8, device=vertices.device,
                             dtype=torch.float64)
            self.measure_grad_raw(vertices, points, dvalues, dverts, djoints, ws)
        if tape_dvalues is not None:
            ws = torch.empty(self.tape_grad_workspace_bytes(B, N) // 8, device=vertices.device, dtype=torch.float64)
            self.measure_tape_grad_raw(vertices, points, tape_dvalues, dverts, djoints, ws, accumulate=bool(self.mesh_columns))
        return dverts, djoints

    def _mesh_structs(self, N):
        """the straps_measure_t array of the non-tape specs for meshes of N vertices (joint anchors resolve to N + j), built once per N"""
        if N not in self._structs:
            self._structs[N] = measure_structs([self.specs[i] for i in self.mesh_columns], N)
        return self._structs[N][0]

    def measure_raw(self, vertices, points, out, workspace):
        """one straps_measure_mesh call for the non-tape specs on contiguous GPU tensors: points None or [B,needs_joints,3], out
        [B,len(mesh_columns)]; what measure_arrays launches, on the caller's buffers"""
        B, N, F = vertices.shape[0], vertices.shape[1], self.faces.shape[0]
        hipabi.check(hipabi.lib().straps_measure_mesh(hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces) if F else None, hipabi.ptr(self.face_parts),
                                                      self._mesh_structs(N), hipabi.ptr(out), hipabi.ptr(workspace), B, N, self.needs_joints, F, len(self.mesh_columns),
                                                      hipabi.stream_ptr()), 'straps_measure_mesh')

    def measure_grad_raw(self, vertices, points, dvalues, dverts, dpoints, workspace):
        """one straps_measure_mesh_bwd call for the non-tape specs on contiguous GPU tensors: points None or [B,needs_joints,3], dvalues
        [B,len(mesh_columns)], dpoints None or [B,rows >= needs_joints,3] (rows the specs do not read are left as they are)"""
        B, N, F = vertices.shape[0], vertices.shape[1], self.faces.shape[0]
        hipabi.check(hipabi.lib().straps_measure_mesh_bwd(
            hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces) if F else None, hipabi.ptr(self.face_parts), hipabi.ptr(self.vf_offsets),
            hipabi.ptr(self.vf_faces) if self.vf_faces.numel() else None, self._mesh_structs(N), hipabi.ptr(dvalues), hipabi.ptr(dverts), hipabi.ptr(dpoints),
            hipabi.ptr(workspace), B, N, self.needs_joints, 0 if dpoints is None else dpoints.shape[1], F, len(self.mesh_columns), hipabi.stream_ptr()),
            'straps_measure_mesh_bwd')

    def _tape_structs_for(self, N):
        """the straps_tape_t array of the tape specs for meshes of N vertices, built once per N"""
        if N not in self._tape_structs:
            self._tape_structs[N] = tape_structs([self.specs[i] for i in self.tape_columns], N)
        return self._tape_structs[N][0]

    def tape_workspace_bytes(self, B):
        """bytes of the workspace of measure_tape_raw for a batch of B"""
        return hipabi.lib().straps_measure_tape_workspace_bytes(B, self.faces.shape[0], len(self.tape_columns), self.tape_capacity or 0)

    def tape_grad_workspace_bytes(self, B, N):
        """bytes of the workspace of measure_tape_grad_raw for a batch of B meshes of N vertices"""
        n = hipabi.lib().straps_measure_tape_bwd_workspace_bytes(B, N, self.faces.shape[0], len(self.tape_columns), self.tape_capacity or 0)
        if not n:
            raise RuntimeError('BodyMeasurer: no tape gradient workspace for batch %d, %d vertices, %d faces, %d tape measurements, capacity %d'
                               % (B, N, self.faces.shape[0], len(self.tape_columns), self.tape_capacity or 0))
        return n

    def measure_tape_raw(self, vertices, points, out, workspace, counts=None):
        """one straps_measure_tape call for the tape specs on contiguous GPU tensors: points None or [B,needs_joints,3], out
        [B,len(tape_columns)], counts None or int32 of that shape; what measure_arrays launches, on the caller's buffers"""
        B, N, F = vertices.shape[0], vertices.shape[1], self.faces.shape[0]
        hipabi.check(hipabi.lib().straps_measure_tape(hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces), hipabi.ptr(self.face_parts),
                                                      self._tape_structs_for(N), hipabi.ptr(out), hipabi.ptr(counts), hipabi.ptr(workspace), B, N, self.needs_joints, F,
                                                      len(self.tape_columns), self.tape_capacity or 0, hipabi.stream_ptr()), 'straps_measure_tape')

    def measure_tape_grad_raw(self, vertices, points, dvalues, dverts, dpoints, workspace, accumulate=False, values=None, counts=None):
        """one straps_measure_tape_bwd call for the tape specs on contiguous GPU tensors: points None or [B,needs_joints,3], dvalues
        [B,len(tape_columns)], dpoints None or [B,rows >= needs_joints,3] (rows the specs do not read are left as they are); accumulate: add
        to what dverts / dpoints hold (straps_measure_mesh_bwd's output, say) instead of overwriting it; values / counts: None or
        [B,len(tape_columns)] float32 / int32, filled with what straps_measure_tape gives"""
        B, N, F = vertices.shape[0], vertices.shape[1], self.faces.shape[0]
        hipabi.check(hipabi.lib().straps_measure_tape_bwd(
            hipabi.ptr(vertices), hipabi.ptr(points), hipabi.ptr(self.faces), hipabi.ptr(self.face_parts), hipabi.ptr(self.vf_offsets), hipabi.ptr(self.vf_faces),
            self._tape_structs_for(N), hipabi.ptr(dvalues), hipabi.ptr(dverts), hipabi.ptr(dpoints), hipabi.ptr(values), hipabi.ptr(counts), hipabi.ptr(workspace), B, N,
            self.needs_joints, 0 if dpoints is None else dpoints.shape[1], F, len(self.tape_columns), self.tape_capacity or 0, 1 if accumulate else 0,
            hipabi.stream_ptr()), 'straps_measure_tape_bwd')

    def forward(self, vertices, joints=None, differentiable=False):
        """-> {'values': [B,M] float32, name: [B] (a view of its column), ...} in the order of `self.names`.  differentiable=True: the values
        carry a gradient to `vertices` and `joints` (autograd_ops.measure_autograd: straps_measure_mesh forward, straps_measure_mesh_bwd
        backward); a measurer with tape specs raises unless it was made with tape_gradients=True (then straps_measure_tape_bwd serves
        them).  The default computes exactly what it always did."""
        if differentiable:
            if self.tape_columns and not self.tape_gradients:
                raise RuntimeError('BodyMeasurer: differentiable=True with the tape specs %r: tape girths (straps_measure_tape) have no gradient without '
                                   'tape_gradients=True' % (list(self.tape_names),))
            from .autograd_ops import measure_autograd
            values = measure_autograd(self, vertices, joints)
        else:
            values = self.measure_arrays(vertices, joints)
        res = {'values': values}
        for i, n in enumerate(self.names):
            res[n] = values[:, i]
        return res
