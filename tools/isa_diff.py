#!/usr/bin/env python
"""Per-kernel comparison of the gfx950 instruction text of two source trees (the check behind "existing kernels keep their text"):
    python tools/isa_diff.py <other csrc dir> env.hip dien.hip step.hip
compiles each unit of <other> and of this tree with the flags of rl4rs_amd/build.py (hipcc -S --offload-device-only), strips comments,
directives and local label numbers, and prints one row per kernel: same / CHANGED / NEW / GONE, instruction lines, VGPRs, scratch.
ISA_DIFF_FLAGS="-DRL4RS_X_USPLIT=0 ..." adds flags to THIS tree's compile only (a switch set back to what the other tree has)."""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rl4rs_amd.build import CSRC, NO_SLP  # noqa: E402


def asm(csrc, unit, out, extra=()):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    cmd = [hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-Wno-unused-function', '-ffp-contract=off', '-mllvm',
           '-pragma-unroll-threshold=200000', '-S', '--offload-device-only', os.path.join(csrc, unit), '-o', out]
    subprocess.check_call(cmd + (['-fno-slp-vectorize'] if unit in NO_SLP else []) + list(extra))
    return open(out).read()


def kernels(text):
    """{mangled name: (normalised instruction lines, vgprs, scratch bytes)} of every .amdhsa_kernel of an assembly file"""
    names = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    out = {}
    for name in names:
        m = re.search(r'^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata' % re.escape(name), text, re.M | re.S)
        if not m:
            continue
        lines = []
        for ln in m.group(1).splitlines():
            ln = ln.split(';')[0].strip()
            if not ln or ln.startswith('.') or ln.endswith(':'):
                continue
            lines.append(re.sub(r'\.LBB\d+_\d+', '.L', ln))
        blk = re.search(r'\.amdhsa_kernel\s+%s\n(.*?)\.end_amdhsa_kernel' % re.escape(name), text, re.S).group(1)
        vg = re.search(r'\.amdhsa_next_free_vgpr\s+(\d+)', blk)
        sc = re.search(r'\.amdhsa_private_segment_fixed_size\s+(\d+)', blk)
        out[name] = (lines, int(vg.group(1)) if vg else -1, int(sc.group(1)) if sc else -1)
    return out


def main():
    other, units = sys.argv[1], sys.argv[2:]
    with tempfile.TemporaryDirectory() as d:
        for u in units:
            a = kernels(asm(other, u, os.path.join(d, 'a.s')))
            b = kernels(asm(CSRC, u, os.path.join(d, 'b.s'), os.environ.get('ISA_DIFF_FLAGS', '').split()))
            print('## %s' % u)
            names = sorted(set(a) | set(b))
            dem = subprocess.run(['c++filt'], input='\n'.join(names) + '\n', capture_output=True, text=True).stdout.splitlines()
            for n, dn in zip(names, dem):
                if n in a and n in b:
                    tag = 'same' if a[n][0] == b[n][0] else 'CHANGED'
                else:
                    tag = 'NEW' if n in b else 'GONE'
                e = b.get(n) or a[n]
                extra = '' if tag != 'CHANGED' else '   (was %d lines, %d VGPR)' % (len(a[n][0]), a[n][1])
                print('%-8s %6d  %-110s %3d VGPR, scratch %d%s' % (tag, len(e[0]), dn[:110], e[1], e[2], extra))


if __name__ == '__main__':
    main()
