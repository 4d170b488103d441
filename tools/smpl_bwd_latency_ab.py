#!/usr/bin/env python3
"""tools/smpl_bwd_latency_ab.py -- the look-ahead form of csrc/smpl_bwd.hip against the library of the commit before it: the same bits.

    python tools/smpl_bwd_latency_ab.py --parent-lib PATH [--out FILE.json]
    PATH = libstraps_hip.so built from the parent commit, e.g.
        git worktree add /tmp/parent <parent commit> && (cd /tmp/parent && python -c "import __graft_entry__ as g; g.build()")
        -> /tmp/parent/straps-3dhumanshapepose_amd/csrc/libstraps_hip.so

For B in {1, 31, 32, 33, 64, 65, 1100} x chunks in {0, 1, 7, 53, 54} x upstream gradient in {dverts only, djoints only, both} (det_uniform inputs,
NaN-filled outputs and workspace) it calls straps_smpl_bwd and straps_smpl_bwd_aa of both libraries and raises unless every output -- dbetas,
drotmats, dfull_pose_aa -- of this tree equals the parent's bit for bit and is finite.  The change moves loads, never a sum: one differing bit is a
failure, not a tolerance question.  Then, at B = 64 and at B = 1100, event-timed means of straps_smpl_bwd for both libraries (back to back, and with a 1 GiB fill
between calls so that the tables come from beyond the caches, as they do inside a training step)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'oracle')]

BATCHES = (1, 31, 32, 33, 64, 65, 1100)
CHUNKS = (0, 1, 7, 53, 54)
KINDS = ('verts', 'joints', 'both')


def main(parent_lib):
    import torch
    import straps_amd
    from straps_amd import hipabi
    from detgen import det_uniform
    dev = torch.device('cuda:0')
    new = hipabi.load()
    old = C.CDLL(parent_lib)
    P, L_, I_ = C.c_void_p, C.c_longlong, C.c_int
    M = C.POINTER(hipabi.SmplModelStruct)
    old.straps_abi_version.restype = C.c_int
    assert old.straps_abi_version() == hipabi.ABI_VERSION, 'the parent library has another ABI version'
    old.straps_smpl_bwd.argtypes = [M, P, P, P, P, P, P, P, L_, I_, P]
    old.straps_smpl_bwd_aa.argtypes = [M, P, P, P, P, P, P, P, P, P, L_, I_, P]
    old.straps_smpl_bwd.restype = old.straps_smpl_bwd_aa.restype = C.c_int
    old.straps_smpl_bwd_workspace_bytes.argtypes = [L_, I_]
    old.straps_smpl_bwd_workspace_bytes.restype = C.c_size_t
    smpl = straps_amd.SMPL(straps_amd.synthetic_smpl_model(0), batch_size=1).to(dev)
    ms = C.byref(smpl._model_struct())
    st = hipabi.stream_ptr()
    p = hipabi.ptr
    nan = float('nan')

    def call(lib, entry, x, chunks, ws):
        B = x['b'].shape[0]
        db, dr, da = torch.full_like(x['b'], nan), torch.full_like(x['r'], nan), torch.full_like(x['aa'], nan)
        ws.fill_(nan)
        if entry == 'rot':
            rc = lib.straps_smpl_bwd(ms, p(x['b']), p(x['r']), p(x['dv']), p(x['dj']), p(db), p(dr), p(ws), B, chunks, st)
            outs = (db, dr)
        else:
            rc = lib.straps_smpl_bwd_aa(ms, p(x['b']), p(x['r']), p(x['aa']), p(x['dv']), p(x['dj']), p(db), p(da), p(dr), p(ws), B, chunks, st)
            outs = (db, dr, da)
        assert rc == 0, '%s failed (code %d)' % (entry, rc)
        torch.cuda.synchronize()
        return outs

    res = {'device': torch.cuda.get_device_name(0), 'batches': BATCHES, 'chunks': CHUNKS, 'kinds': KINDS, 'entries': ['straps_smpl_bwd', 'straps_smpl_bwd_aa'],
           'cases': 0, 'outputs_compared': 0, 'differing': []}
    for B in BATCHES:
        b = torch.from_numpy(det_uniform((B, 10), 1, -2, 2)).to(dev)
        aa = torch.from_numpy(det_uniform((B, 72), 2, -2, 2)).to(dev)
        r = straps_amd.batch_rodrigues(aa.view(-1, 3)).view(B, 24, 3, 3).contiguous()
        dv = torch.from_numpy(det_uniform((B, 6890, 3), 3, -1, 1)).to(dev)
        dj = torch.from_numpy(det_uniform((B, 90, 3), 4, -1, 1)).to(dev)
        for chunks in CHUNKS:
            assert old.straps_smpl_bwd_workspace_bytes(B, chunks) == new.straps_smpl_bwd_workspace_bytes(B, chunks)
            ws = torch.empty(new.straps_smpl_bwd_workspace_bytes(B, chunks) // 4, device=dev)
            for kind in KINDS:
                x = dict(b=b, aa=aa, r=r, dv=dv if kind != 'joints' else None, dj=dj if kind != 'verts' else None)
                for entry in ('rot', 'aa'):
                    want, got = call(old, entry, x, chunks, ws), call(new, entry, x, chunks, ws)
                    res['cases'] += 1
                    for name, w, g in zip(('dbetas', 'drotmats', 'dfull_pose_aa'), want, got):
                        res['outputs_compared'] += 1
                        if not (torch.equal(w, g) and bool(torch.isfinite(g).all())):
                            res['differing'].append('B=%d chunks=%d %s %s %s: %d elements' % (B, chunks, kind, entry, name, int((w != g).sum())))
        print('B = %d: %d cases so far, %d differing outputs' % (B, res['cases'], len(res['differing'])), flush=True)
    res['bitwise_equal_to_parent'] = not res['differing']

    # timing at the training step's batch and at a large one (8 chunks, several rounds per wave, the pose pass on every CU)
    res['us_per_call'] = {'unit': 'us per straps_smpl_bwd call (pose forward + vertex pass + pose pass), device events, alternating libraries'}
    flush = torch.empty(1 << 28, device=dev)
    for B in (64, 1100):
        b = torch.from_numpy(det_uniform((B, 10), 1, -2, 2)).to(dev)
        r = straps_amd.batch_rodrigues(torch.from_numpy(det_uniform((B, 72), 2, -2, 2)).to(dev).view(-1, 3)).view(B, 24, 3, 3).contiguous()
        dv = torch.from_numpy(det_uniform((B, 6890, 3), 3, -1, 1)).to(dev)
        dj = torch.from_numpy(det_uniform((B, 90, 3), 4, -1, 1)).to(dev)
        ws = torch.empty(new.straps_smpl_bwd_workspace_bytes(B, 0) // 4, device=dev)
        db, dr = torch.empty_like(b), torch.empty_like(r)
        libs = {'parent': old, 'this': new}
        run = lambda lib: lib.straps_smpl_bwd(ms, p(b), p(r), p(dv), p(dj), p(db), p(dr), p(ws), B, 0, st)
        for lib in libs.values():
            for _ in range(5):
                run(lib)
        warm, cold = {n: [] for n in libs}, {n: [] for n in libs}
        for rnd in range(7):
            for name, lib in libs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    run(lib)
                e1.record()
                torch.cuda.synchronize()
                warm[name].append(e0.elapsed_time(e1) / 20 * 1000.0)
        for rnd in range(9):
            for name, lib in libs.items():
                flush.fill_(float(rnd))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run(lib)
                e1.record()
                torch.cuda.synchronize()
                cold[name].append(e0.elapsed_time(e1) * 1000.0)
        res['us_per_call']['B=%d' % B] = {'back_to_back_median_of_7x20': {n: round(statistics.median(v), 1) for n, v in warm.items()},
                                          'after_1GiB_fill_median_of_9': {n: round(statistics.median(v), 1) for n, v in cold.items()}}
    text = json.dumps(res, indent=1) + '\n'
    print(text, end='')
    return text, res['differing']


if __name__ == '__main__':
    ap = argparse.ArgumentParser()
    ap.add_argument('--parent-lib', required=True)
    ap.add_argument('--out')
    a = ap.parse_args()
    text, differing = main(a.parent_lib)
    if a.out:
        with open(a.out, 'w') as f:
            f.write(text)
    if differing:
        raise SystemExit('straps_smpl_bwd differs from the parent library:\n  ' + '\n  '.join(differing))
