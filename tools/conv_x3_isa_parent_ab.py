"""Instruction-stream A/B of the forward / data-gradient convolution kernels against a parent revision: a change of the host side (the launch plan,
the dispatchers, the launchers) must leave every kernel's instructions as they were, and the set of instantiations too.  conv.hip, conv_x3.hip,
conv_x3_lean.hip, conv_x3f.hip and conv_bf16.hip of the working tree and of REV (git archive) are compiled with
`hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S`; directives, comments and labels other than basic blocks are dropped, the function's number in the
translation unit is taken out of the basic-block labels (.LBB<n>_<k>: it follows the order of instantiation, which a host-side change moves; likewise .Lpost_getpc<n>), and what
remains is diffed per kernel under its mangled name as it stands.  CPU only.

    python tools/conv_x3_isa_parent_ab.py [--rev HEAD] [--out profiles/conv_plan_isa_parent_diff.txt]
"""
import argparse
import difflib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = 'straps-3dhumanshapepose_amd'
SOURCES = ('conv.hip', 'conv_x3.hip', 'conv_x3_lean.hip', 'conv_x3f.hip', 'conv_bf16.hip')


def asm(csrc, src, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S', src, '-o', out], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text):
    """kernel name -> instruction lines"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^(_Z\S+):', line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        s = line.split(';')[0].rstrip()
        if not s.strip() or s.lstrip().startswith('.') or re.match(r'^\s*\S+:$', s) and 'BB' not in s:
            if s.strip().startswith(('.Lfunc_end', '.size')):
                cur = None
            continue
        out[cur].append(re.sub(r'\.Lpost_getpc\d+', '.Lpost_getpc', re.sub(r'\.LBB\d+_', '.LBB_', s)))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rev', default='HEAD', help='parent revision (before the change is committed: HEAD; afterwards: HEAD~1)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_plan_isa_parent_diff.txt'))
    a = ap.parse_args()
    rev = subprocess.run(['git', 'rev-parse', '--short=12', a.rev], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    lines = ['forward / data-gradient convolution kernels: instruction streams of the working tree against %s (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S)' % rev]
    total = moved = 0
    with tempfile.TemporaryDirectory() as tmp:
        arch = subprocess.run(['git', 'archive', a.rev, PKG + '/csrc', 'include'], cwd=ROOT, capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', tmp], input=arch, check=True)
        for src in SOURCES:
            old = kernels(asm(os.path.join(tmp, PKG, 'csrc'), src, os.path.join(tmp, 'old_' + src + '.s')))
            new = kernels(asm(os.path.join(ROOT, PKG, 'csrc'), src, os.path.join(tmp, 'new_' + src + '.s')))
            for k in sorted(set(old) | set(new)):
                if k not in old or k not in new:
                    moved += 1
                    lines.append('%s  %-100s %6d instructions  only in the %s' % (src, k, len(old.get(k, new.get(k))), 'parent' if k in old else 'working tree'))
                    continue
                d = list(difflib.unified_diff(old[k], new[k], lineterm='', n=0))
                total += len(d)
                lines.append('%s  %-100s %6d instructions  %s' % (src, k, len(old[k]), 'identical' if not d else '%d diff lines' % len(d)))
                lines += d[:40]
    lines.append('TOTAL diff lines: %d; instantiations only on one side: %d' % (total, moved))
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-3:]))
    sys.exit(1 if total or moved else 0)


if __name__ == '__main__':
    main()
