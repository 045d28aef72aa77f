#!/usr/bin/env python3
"""Emitted-code comparison of two source trees of the library (no GPU: compiles and reads assembly only).

    python tools/isa_compare.py PARENT_CSRC BRANCH_CSRC [--out TABLE] [--jobs N] [--keep DIR]

Compiles every *.hip of both csrc directories to gfx950 assembly with the Makefile's flags (FLAGS and the per-file FLAGS_<name>,
read from each tree's own Makefile by `make -pn`) plus `--cuda-device-only -S`, and compares each kernel: the sequence of
instruction mnemonics, .vgpr_count, .agpr_count, .sgpr_count, .private_segment_fixed_size, .group_segment_fixed_size and the code
length (instructions). Operands and register numbers may differ. Prints one line per kernel; exit status 1 if any kernel differs."""
import argparse
import concurrent.futures
import difflib
import os
import re
import subprocess
import sys
import tempfile

META = ('.vgpr_count', '.agpr_count', '.sgpr_count', '.private_segment_fixed_size', '.group_segment_fixed_size')


def make_vars(csrc):
    """HIPCC, FLAGS and FLAGS_<file> of the tree's Makefile, expanded by make itself"""
    db = subprocess.run(['make', '-C', csrc, '-pn', '--no-print-directory'], capture_output=True, text=True).stdout
    raw = {}
    for m in re.finditer(r'^([A-Za-z_][A-Za-z0-9_]*) *[:?]?= *(.*)$', db, re.M):
        raw.setdefault(m.group(1), m.group(2))

    def expand(v, depth=0):
        return re.sub(r'\$\((\w+)\)', lambda m: expand(raw.get(m.group(1), ''), depth + 1) if depth < 8 else '', v)

    return {k: expand(v) for k, v in raw.items() if k in ('HIPCC', 'FLAGS', 'SRCS') or k.startswith('FLAGS_')}


def compile_tree(csrc, out, jobs):
    v = make_vars(csrc)
    os.makedirs(out, exist_ok=True)

    def one(src):
        base = src[:-4]
        cmd = [v['HIPCC']] + v['FLAGS'].split() + v.get('FLAGS_' + base, '').split() + ['--cuda-device-only', '-S', src, '-o',
                                                                                         os.path.join(out, base + '.s')]
        r = subprocess.run(cmd, cwd=csrc, capture_output=True, text=True)
        if r.returncode:
            raise RuntimeError('%s: %s' % (src, r.stderr[-2000:]))

    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        list(ex.map(one, v['SRCS'].split()))


INSTR = re.compile(r'^\t([a-z][a-z0-9_]*)(\s|$)')


def parse(path):
    """{kernel: (mnemonics, {meta})} of one assembly file"""
    text = open(path).read()
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    code = {}
    cur = None
    for line in text.split('\n'):
        m = re.match(r'^([A-Za-z_$][\w$.]*):', line)
        if m and not m.group(1).startswith('.L'):
            cur = m.group(1) if m.group(1) in kernels else None
            if cur:
                code[cur] = []
            continue
        if cur is None:
            continue
        if line.startswith('\t.size') or line.startswith('\t.section') or line.startswith('.Lfunc_end'):
            cur = None
            continue
        m = INSTR.match(line)
        if m:
            code[cur].append(m.group(1))
    meta = {}
    for blk in re.split(r'^  - \.agpr_count:', text, flags=re.M)[1:]:
        blk = '  - .agpr_count:' + blk
        name = re.search(r'^\s+\.name:\s+(\S+)', blk, re.M).group(1)
        meta[name] = {k: int(re.search(r'%s:\s+(\d+)' % re.escape(k), blk).group(1)) for k in META}
    return {k: (code[k], meta[k]) for k in kernels}


def demangle(names):
    if not names:
        return {}
    out = subprocess.run(['c++filt'] + list(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, out))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('parent')
    ap.add_argument('branch')
    ap.add_argument('--out', help='write the table here as well')
    ap.add_argument('--jobs', type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument('--keep', help='keep the assembly under DIR/parent and DIR/branch (reused if present)')
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix='isa_compare_')
    dirs = {}
    for side, csrc in (('parent', a.parent), ('branch', a.branch)):
        dirs[side] = os.path.join(tmp, side)
        if not (a.keep and os.path.isdir(dirs[side]) and os.listdir(dirs[side])):
            compile_tree(csrc, dirs[side], a.jobs)
    lines = ['# file  kernel  instructions  vgpr agpr sgpr scratch lds  verdict', '#   verdict: same = identical mnemonic sequence and resources']
    bad = 0
    tot_k = tot_i = 0
    files = sorted(set(os.listdir(dirs['parent'])) | set(os.listdir(dirs['branch'])))
    for f in files:
        pp, pb = os.path.join(dirs['parent'], f), os.path.join(dirs['branch'], f)
        if not (os.path.exists(pp) and os.path.exists(pb)):
            lines.append('%s  ONLY IN %s' % (f, 'parent' if os.path.exists(pp) else 'branch'))
            bad += 1
            continue
        P, B = parse(pp), parse(pb)
        names = demangle(sorted(set(P) | set(B)))
        for k in sorted(set(P) | set(B)):
            short = re.sub(r'\([^()]*\)$', '', names.get(k, k)).replace('void ', '').replace('lvae::', '').replace(', ', ',')
            if k not in P or k not in B:
                lines.append('%s  %s  ONLY IN %s' % (f[:-2], short, 'parent' if k in P else 'branch'))
                bad += 1
                continue
            (cp, mp), (cb, mb) = P[k], B[k]
            tot_k += 1
            tot_i += len(cb)
            res = ' '.join(str(mb[x]) for x in META)
            if cp == cb and mp == mb:
                verdict = 'same'
            else:
                bad += 1
                why = []
                if len(cp) != len(cb):
                    why.append('instructions %d -> %d' % (len(cp), len(cb)))
                elif cp != cb:
                    sm = difflib.SequenceMatcher(None, cp, cb, autojunk=False)
                    why.append('%d mnemonics moved or changed' % sum(max(i2 - i1, j2 - j1) for t, i1, i2, j1, j2 in sm.get_opcodes() if t != 'equal'))
                why += ['%s %d -> %d' % (x, mp[x], mb[x]) for x in META if mp[x] != mb[x]]
                verdict = 'DIFFERS: ' + ', '.join(why)
            lines.append('%s  %s  %d  %s  %s' % (f[:-2], short, len(cb), res, verdict))
    lines.append('# %d kernels, %d instructions on the branch side, %d differ' % (tot_k, tot_i, bad))
    text = '\n'.join(lines) + '\n'
    sys.stdout.write(text)
    if a.out:
        open(a.out, 'w').write(text)
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
