#!/usr/bin/env python3
"""Compare the device assembly of the kernel instantiations two trees have in common (DESIGN.md sections 5c, 5d: a pull request that adds
a template parameter or a kernel argument must leave the existing instantiations instruction for instruction as they were).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/FILE.hip -o OLD/FILE.s       (in the parent tree)
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/FILE.hip -o NEW/FILE.s       (in this tree)
    python scripts/asm_diff_instantiations.py OLD NEW [FILE ...]          default: pwattn_fwd pwattn_fwd_rw pool_loss

A kernel of OLD is matched to the kernel of NEW with the same demangled name, or with one more trailing ``false`` template argument
(a new flag that defaults to off; a kernel that was no template becomes ``name<false>``); the argument list may have grown.  Symbol names, label numbers and comments are normalised away;
every remaining difference is printed.  Differences in ``.amdhsa_kernarg_size`` and in the offset of an ``s_load`` from the kernel
argument segment (a hidden argument behind a larger block) are counted apart from real ones, and so is the section directive of a kernel
that became a template instantiation (``.text`` -> its own comdat ``.section .text.<symbol>``: where the code lies, not what it is).  Exit status 1 on a real difference."""
import difflib
import os
import re
import subprocess
import sys

def funcs(path):
    out, cur, name = {}, None, None
    order=[]
    for ln in open(path):
        m = re.match(r'^(_Z\w+):', ln)
        if m and cur is None:
            name, cur = m.group(1), []
            continue
        if cur is not None:
            if ln.startswith('.Lfunc_end'):
                out[name] = cur; order.append(name); cur = None
            else:
                cur.append(re.sub(r'\.L(BB|tmp|func_begin)\d+', '.L', re.sub(r'_Z\w+', 'SYM', re.sub(r';.*', '', ln))).rstrip())
    return out, order
def dem(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, r))
real = 0
old_dir, new_dir = sys.argv[1], sys.argv[2]
for f in (sys.argv[3:] or ['pwattn_fwd', 'pwattn_fwd_rw', 'pool_loss']):
    b, bo = funcs(os.path.join(old_dir, f + '.s')); n, no = funcs(os.path.join(new_dir, f + '.s'))
    db, dn = dem(bo), dem(no)
    inv = {v: k for k, v in dn.items()}
    same = diff = moved = 0
    for k in bo:
        d = db[k]
        cand = [d]
        m = re.match(r'^(void nrm::\w+<)([^>]*)(>\()', d)
        if m: cand.append(m.group(1) + m.group(2) + ', false' + m.group(3))
        elif '<' not in d.split('(')[0]: cand.append('void ' + d.split('(')[0] + '<false>(')
        # prefix match on "name<args>(" since the argument list may have grown
        hit = None
        for c in cand:
            key = c.split('>(')[0] + '>(' if '>(' in c else c.split('(')[0] + '('
            hits = [x for x in dn.values() if x.startswith(key)]
            if len(hits) == 1: hit = inv[hits[0]]
        if hit is None:
            print(f, 'NO MATCH', d[:120]); diff += 1; continue
        if b[k] == n[hit]: same += 1
        else:
            dl = [l for l in difflib.unified_diff(b[k], n[hit], lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]
            if all(re.search(r'\.amdhsa_kernarg_size|s_load_dword\w* \S+ s\[\d+:\d+\], 0x|^[-+]\s*\.text$|^[-+]\s*\.section\s+\.text\.SYM,', l) for l in dl):
                moved += 1
                continue
            diff += 1
            print(f, 'DIFF', d[:100], len(dl), 'lines'); print('\n'.join(dl[:12]))
    real += diff
    print(f'{f}: {len(bo)} existing instantiations: {same} identical, {moved} differ only in the kernel-argument size / a hidden-argument offset / the section directive of a kernel that became a template, '
          f'{diff} really different; the new tree has {len(no)} kernels')
sys.exit(1 if real else 0)
