"""Instruction-stream A/B of the bf16x3 plane kernels against a parent revision: conv_x3_kernels.h is templated on a plane count (PL, last template
parameter; PL = 0 = the bf16x3 kernels) for the single-product bf16 route, and the shared epilogue on its output plane count -- the existing
instantiations must compile to the SAME instructions.  conv_x3.hip and conv_x3_lean.hip of the working tree and of REV (git archive) are compiled with
`hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S`; directives, comments, labels' translation-unit ids and the trailing template argument of
the new parameter (ELi0E in the mangled names) are normalised away, and what remains is diffed per kernel.  CPU only.

    python tools/conv_x3_isa_parent_ab.py [--rev HEAD] [--out profiles/conv_x3_isa_parent_diff.txt]
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
SOURCES = ('conv_x3.hip', 'conv_x3_lean.hip')


def asm(csrc, src, out):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '--cuda-device-only', '-S', src, '-o', out], cwd=csrc, check=True,
                   stderr=subprocess.DEVNULL)
    return open(out).read()


def kernels(text, strip_pl):
    """kernel name -> normalised instruction lines (strip_pl: drop the trailing PL = 0 argument of the working tree's names)"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^(_Z\S+):', line)
        if m:
            cur = re.sub(r'ELi0EEEvNS_5ConvPE$', 'EEEvNS_5ConvPE', m.group(1)) if strip_pl else m.group(1)
            out[cur] = []
            continue
        if cur is None:
            continue
        s = line.split(';')[0].rstrip()
        if not s.strip() or s.lstrip().startswith('.') or re.match(r'^\s*\S+:$', s) and 'BB' not in s:
            if s.strip().startswith('.Lfunc_end'):
                cur = None
            continue
        out[cur].append(s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rev', default='HEAD', help='parent revision (before the change is committed: HEAD; afterwards: HEAD~1)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'conv_x3_isa_parent_diff.txt'))
    a = ap.parse_args()
    rev = subprocess.run(['git', 'rev-parse', '--short=12', a.rev], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    lines = ['bf16x3 plane kernels: instruction streams of the working tree against %s (hipcc --offload-arch=gfx950 -O3 --cuda-device-only -S)' % rev]
    total = 0
    with tempfile.TemporaryDirectory() as tmp:
        arch = subprocess.run(['git', 'archive', a.rev, PKG + '/csrc', 'include'], cwd=ROOT, capture_output=True, check=True).stdout
        subprocess.run(['tar', '-x', '-C', tmp], input=arch, check=True)
        for src in SOURCES:
            old = kernels(asm(os.path.join(tmp, PKG, 'csrc'), src, os.path.join(tmp, 'old_' + src + '.s')), False)
            new = kernels(asm(os.path.join(ROOT, PKG, 'csrc'), src, os.path.join(tmp, 'new_' + src + '.s')), True)
            assert set(old) == set(new), (src, sorted(set(old) ^ set(new)))
            for k in sorted(old):
                d = list(difflib.unified_diff(old[k], new[k], lineterm='', n=0))
                total += len(d)
                lines.append('%s  %-90s %6d instructions  %s' % (src, k, len(old[k]), 'identical' if not d else '%d diff lines' % len(d)))
                lines += d[:40]
    lines.append('TOTAL diff lines: %d' % total)
    open(a.out, 'w').write('\n'.join(lines) + '\n')
    print('\n'.join(lines[-3:]))
    sys.exit(1 if total else 0)


if __name__ == '__main__':
    main()
