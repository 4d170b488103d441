#!/usr/bin/env python3
"""tools/smpl_bwd_parent_ab.py -- the axis-angle gradient change (ABI 10) measured against the library of the commit before it.

GPU mode (default):  python tools/smpl_bwd_parent_ab.py --parent-lib PATH [--out FILE.json]
    PATH = libstraps_hip.so built from the parent commit (ABI 9), e.g.
        git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -c "import __graft_entry__ as g; g.build()")
        -> /tmp/parent/straps-3dhumanshapepose_amd/csrc/libstraps_hip.so
    For B = 64 / 1100 / 4096 bodies (det_uniform inputs): straps_smpl_bwd of this tree == the parent's, bit for bit (dbetas, drotmats; raises
    otherwise), and event-timed means over 20 calls of: straps_smpl_bwd (parent, this tree), straps_rodrigues_bwd, straps_smpl_bwd_aa (fused).
ISA mode (host only): python tools/smpl_bwd_parent_ab.py --isa PARENT_SMPL_BWD_HIP [--out FILE.txt]
    compiles the parent's csrc/smpl_bwd.hip and this tree's to gfx950 assembly and lists the opcode counts of smpl_pose_bwd_kernel that differ
    (the parent's plain kernel against this tree's <false> / <true> instantiations)."""
import argparse
import collections
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]


def gpu_mode(parent_lib):
    import torch
    import straps_amd
    from straps_amd import hipabi
    from detgen import det_uniform
    dev = torch.device('cuda:0')
    new = hipabi.load()
    old = C.CDLL(parent_lib)
    old.straps_abi_version.restype = C.c_int
    assert old.straps_abi_version() == 9, 'expected the parent library (ABI 9)'
    P, L_, I_ = C.c_void_p, C.c_longlong, C.c_int
    old.straps_smpl_bwd.argtypes = [C.POINTER(hipabi.SmplModelStruct), P, P, P, P, P, P, P, L_, I_, P]
    old.straps_smpl_bwd.restype = C.c_int
    old.straps_smpl_bwd_workspace_bytes.argtypes = [L_, I_]
    old.straps_smpl_bwd_workspace_bytes.restype = C.c_size_t
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1).to(dev)
    ms = C.byref(smpl._model_struct())
    st = hipabi.stream_ptr()
    p = hipabi.ptr

    def timeit(fn, reps=20):
        for _ in range(3):
            hipabi.check(fn(), 'warm-up')
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return round(e0.elapsed_time(e1) / reps * 1000.0, 1)      # us

    res = {'device': torch.cuda.get_device_name(0), 'reps': 20, 'unit': 'us per call (event-timed mean)'}
    for B in (64, 1100, 4096):
        b = torch.from_numpy(det_uniform((B, 10), 1, -2, 2)).to(dev)
        aa = torch.from_numpy(det_uniform((B, 72), 2, -2, 2)).to(dev)
        r = straps_amd.batch_rodrigues(aa.view(-1, 3)).view(B, 24, 3, 3)
        dv = torch.from_numpy(det_uniform((B, 6890, 3), 3, -1, 1)).to(dev)
        dj = torch.from_numpy(det_uniform((B, 90, 3), 4, -1, 1)).to(dev)
        assert old.straps_smpl_bwd_workspace_bytes(B, 0) == new.straps_smpl_bwd_workspace_bytes(B, 0)
        ws = torch.empty(new.straps_smpl_bwd_workspace_bytes(B, 0) // 4, device=dev)
        outs = {}
        for name, lib in (('parent', old), ('this', new)):
            db, dr = torch.empty_like(b), torch.empty_like(r)
            hipabi.check(lib.straps_smpl_bwd(ms, p(b), p(r), p(dv), p(dj), p(db), p(dr), p(ws), B, 0, st), name)
            outs[name] = (db, dr)
        same = torch.equal(outs['parent'][0], outs['this'][0]) and torch.equal(outs['parent'][1], outs['this'][1])
        db, dr, daa = torch.empty_like(b), torch.empty_like(r), torch.empty_like(aa)
        res[str(B)] = dict(
            smpl_bwd_bitwise_equal_to_parent=same,
            smpl_bwd_parent=timeit(lambda: old.straps_smpl_bwd(ms, p(b), p(r), p(dv), p(dj), p(db), p(dr), p(ws), B, 0, st)),
            smpl_bwd_this=timeit(lambda: new.straps_smpl_bwd(ms, p(b), p(r), p(dv), p(dj), p(db), p(dr), p(ws), B, 0, st)),
            rodrigues_bwd=timeit(lambda: new.straps_rodrigues_bwd(p(aa), p(dr), p(daa), B * 24, st)),
            smpl_bwd_aa_fused=timeit(lambda: new.straps_smpl_bwd_aa(ms, p(b), p(r), p(aa), p(dv), p(dj), p(db), p(daa), None, p(ws), B, 0, st)))
        print(B, res[str(B)], flush=True)
        assert same, 'straps_smpl_bwd differs from the parent library at B=%d' % B
    return json.dumps(res, indent=1) + '\n'


def _kernels(asm):
    s = open(asm).read()
    out = {}
    for m in re.finditer(r'^(\S*smpl_pose_bwd_kernel\S*):\s*;', s, re.M):
        body = s[m.end():s.index('.Lfunc_end', m.end())]
        ins = [ln.split(';')[0].strip() for ln in body.splitlines()]
        out[m.group(1)] = collections.Counter(i.split()[0] for i in ins if i and not i.startswith('.') and not i.endswith(':'))
    return out


def isa_mode(parent_src):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    csrc = os.path.join(ROOT, 'straps-3dhumanshapepose_amd', 'csrc')
    tmp = tempfile.mkdtemp()
    try:
        old_src = os.path.join(csrc, '_parent_smpl_bwd.hip')         # beside the headers it includes; removed below
        shutil.copy(parent_src, old_src)
        asm = {}
        try:
            for tag, src in (('parent', old_src), ('this', os.path.join(csrc, 'smpl_bwd.hip'))):
                asm[tag] = os.path.join(tmp, tag + '.s')
                subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S', src, '-o', asm[tag]],
                               check=True, stderr=subprocess.DEVNULL)
        finally:
            os.remove(old_src)
        (pname, pc), = _kernels(asm['parent']).items()
        lines = ['smpl_pose_bwd_kernel opcode counts that differ from the parent (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S)',
                 'parent: %s (%d instructions)' % (pname, sum(pc.values()))]
        for name, c in _kernels(asm['this']).items():
            lines.append('this tree: %s (%d instructions)' % (name, sum(c.values())))
            for op in sorted(set(pc) | set(c)):
                if pc[op] != c[op] and not op.startswith('@'):
                    lines.append('    %-24s %5d -> %5d' % (op, pc[op], c[op]))
        return '\n'.join(lines) + '\n'
    finally:
        shutil.rmtree(tmp)


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib')
    ap.add_argument('--isa', metavar='PARENT_SMPL_BWD_HIP')
    ap.add_argument('--out')
    a = ap.parse_args()
    text = isa_mode(a.isa) if a.isa else gpu_mode(a.parent_lib)
    print(text, end='')
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
