#!/usr/bin/env python3
"""Do two builds of one HIP source hold the same kernels?  Per kernel: the resource fields of the code object's notes and its
instruction text, with what depends only on where a kernel lies in the file masked (the literals of the s_add_u32 /
s_addc_u32 pair behind an s_getpc_b64: PC-relative addresses of the file's tables and of far branch targets; the address,
encoding and symbol annotation that llvm-objdump writes behind each instruction).  Prints the kernels that differ; exit
status 1 if any does.  A .hip input is compiled to a bare code object with the library's flags (build.py) beside it.
usage: same_code.py OLD NEW [--meta OLD.txt NEW.txt] ['old-regex=new-text' ...]
  old-regex=new-text: re.sub on the OLD mangled names for templates that were renamed, e.g.
  '13k_band_newtonI(\\w+?)EEv=13k_band_searchI\\1Lb0EEEv'"""
import os, re, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from triangular_transport_toolbox_amd import build
LLVM = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc_path()))), 'llvm', 'bin')
FIELDS = ['.vgpr_count', '.agpr_count', '.sgpr_count', '.vgpr_spill_count', '.sgpr_spill_count', '.private_segment_fixed_size',
          '.group_segment_fixed_size']

def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout

def code_object(path):
    if not path.endswith('.hip'): return path
    out = path + '.co'
    flags = [f for f in build.FLAGS if f != '-shared'] + ['-I', build.CSRC, '--cuda-device-only', '--no-gpu-bundle-output']
    run(build.hipcc_path(), *flags, '-x', 'hip', '-c', path, '-o', out)
    return out

def meta(co):
    """{kernel: [fields]} from the notes: one map per kernel under amdhsa.kernels, opened by '  - .'"""
    res, cur = {}, {}
    for l in run(os.path.join(LLVM, 'llvm-readobj'), '--notes', co).split('\n') + ['  - .']:
        if l.startswith('  - .'):
            if '.name' in cur: res[cur['.name']] = [cur[f] for f in FIELDS]
            cur = {}
        m = re.match(r'^(?:    |  - )(\.\w+):\s+(\S+)$', l)
        if m: cur[m.group(1)] = m.group(2)
    return res

def text(co):
    """{function: [masked instructions]}"""
    res, cur, pc = {}, None, 0
    for l in run(os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', '--no-leading-addr', co).split('\n'):
        m = re.match(r'^<(\S+)>:$', l)
        if m: cur = res.setdefault(m.group(1), []); continue
        s = l.split('//')[0].strip()
        if cur is None or not s: continue
        if pc and re.match(r'^s_addc?_u32 ', s): s = s.rsplit(',', 1)[0] + ', PCREL'
        pc = 2 if s.startswith('s_getpc_b64') else max(pc - 1, 0)
        cur.append(s)
    return res

args = sys.argv[1:]
lists = None
if '--meta' in args:
    i = args.index('--meta'); lists = args[i + 1:i + 3]; del args[i:i + 3]
old, new = code_object(args[0]), code_object(args[1])
subs = [a.split('=', 1) for a in args[2:]]
def renamed(name):
    for pat, rep in subs: name = re.sub(pat, rep, name)
    return name
mo, mn, to, tn = meta(old), meta(new), text(old), text(new)
for path, m in zip(lists or [], (mo, mn)):
    with open(path, 'w') as f:
        f.write('# .name ' + ' '.join(FIELDS) + '\n' + ''.join('%s %s\n' % (k, ' '.join(m[k])) for k in sorted(m)))
bad, seen = 0, set()
for k in sorted(mo):
    k2 = renamed(k); seen.add(k2)
    if k2 not in mn: print('only in OLD  %s%s' % (k, '' if k2 == k else ' (looked for %s)' % k2)); bad += 1; continue
    if mo[k] != mn[k2]: print('metadata     %s: %s -> %s' % (k2, ' '.join(mo[k]), ' '.join(mn[k2]))); bad += 1
    a, b = to[k], tn[k2]
    if a != b:
        i = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print('instructions %s: %d -> %d, first difference at %d: %s | %s' % (k2, len(a), len(b), i, (a + ['-'])[i], (b + ['-'])[i])); bad += 1
for k in sorted(set(mn) - seen): print('only in NEW  %s' % k); bad += 1
print('%d kernels in OLD, %d in NEW, %d renamed, %d instructions compared: %s' % (
    len(mo), len(mn), sum(renamed(k) != k for k in mo), sum(len(to[k]) for k in mo), '%d differences' % bad if bad else 'same code'))
sys.exit(1 if bad else 0)
