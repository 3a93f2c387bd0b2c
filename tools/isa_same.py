#!/usr/bin/env python3
"""Is the device code of two sets of ISA listings the same?  For a change that only moves kernels between translation units.
    make -C metric_depth_video_toolbox_amd/csrc asm SRC=mdvt_mesh_rows [ASMFLAGS=-DMDVT_TUNING]     (one listing per unit and variant)
    python tools/isa_same.py before/ after/            (a set = directories of *.s and / or single listings, comma separated)
Every function of a listing (kernels and the device functions the compiler did not inline) is compared by name: its text with
comments stripped and the function-local label numbers (.LBB<n>_, .Ltmp<n>) normalised, and, for a kernel, every .amdhsa_ field
of its descriptor (registers, LDS, scratch, ...).  Reports what differs, what is missing, new, or defined twice in a set; exit
status 0 only if nothing is.  It compares text: no instruction is looked at or named."""
import glob, os, re, sys


def listings(arg):
    out = []
    for p in arg.split(','):
        out += sorted(glob.glob(os.path.join(p, '*.s'))) if os.path.isdir(p) else [p]
    return out


def normal(line):
    line = re.sub(r'\.LBB\d+_', '.LBB_', re.sub(r'\.Ltmp\d+', '.Ltmp', line.split(';')[0]))
    return ' '.join(line.split())


def functions(path):
    """name -> (text, fields or None) of one listing"""
    lines = open(path).read().split('\n')
    names = [m.group(1) for m in (re.match(r'\s*\.type\s+(\S+),@function', l) for l in lines) if m]
    start = {l.split(':')[0]: k for k, l in enumerate(lines) if ':' in l and l.split(':')[0] in names}
    fields, cur = {}, None
    for l in lines:
        t = l.strip()
        if t.startswith('.amdhsa_kernel '): cur = t.split()[1]; fields[cur] = []
        elif t == '.end_amdhsa_kernel': cur = None
        elif cur and t.startswith('.amdhsa_'): fields[cur].append(normal(t))
    out = {}
    for n in names:
        k, text = start[n] + 1, []
        while not lines[k].startswith('.Lfunc_end'):
            if normal(lines[k]): text.append(normal(lines[k]))
            k += 1
        out[n] = (text, fields.get(n))
    return out


def collect(arg):
    found, twice = {}, []
    for p in listings(arg):
        for n, f in functions(p).items():
            if n in found: twice.append(n)
            found[n] = f
    return found, twice


a, a2 = collect(sys.argv[1])
b, b2 = collect(sys.argv[2])
bad = 0
for tag, names in (('twice in the first set', a2), ('twice in the second set', b2), ('missing from the second set', sorted(set(a) - set(b))),
                   ('new in the second set', sorted(set(b) - set(a)))):
    for n in names: print(f'{tag}: {n}'); bad += 1
for n in sorted(set(a) & set(b)):
    text, fld = a[n][0] == b[n][0], a[n][1] == b[n][1]
    if not (text and fld):
        print(f"differs ({'text' if not text else ''}{' ' if not (text or fld) else ''}{'descriptor' if not fld else ''}): {n}"); bad += 1
kern = lambda s: sum(1 for v in s.values() if v[1] is not None)
print(f'{kern(a)} kernels + {len(a) - kern(a)} other functions in the first set, {kern(b)} + {len(b) - kern(b)} in the second; '
      f'{len(set(a) & set(b)) } compared, {bad} findings')
sys.exit(1 if bad else 0)
