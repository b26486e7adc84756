#!/usr/bin/env python3
"""Compare the device assembly of the kernel instantiations two trees have in common (DESIGN.md sections 5c, 5d: a pull request that adds
a template parameter or a kernel argument must leave the existing instantiations instruction for instruction as they were).

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/FILE.hip -o OLD/FILE.s       (in the parent tree)
    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S csrc/FILE.hip -o NEW/FILE.s       (in this tree)
    python scripts/asm_diff_instantiations.py OLD NEW [FILE ...]          default: pwattn_fwd pwattn_fwd_rw pool_loss

A kernel of OLD is matched to the kernel of NEW with the same demangled name, or with one more trailing ``false`` template argument
(a new flag that defaults to off; a kernel that was no template becomes ``name<false>``), or with one trailing template argument fewer
where DROPPED names the kernel and the old argument was the value given there (a parameter that was removed: only its old default
survives); the argument list may have grown.  A kernel of OLD without a counterpart in NEW is gone (listed, not a difference); the
kernels of NEW that no kernel of OLD was matched to are counted.  Symbol names, label numbers and comments are normalised away;
every remaining difference is printed.  Differences in ``.amdhsa_kernarg_size`` and in the offset of an ``s_load`` from the kernel
argument segment (a hidden argument behind a larger block) are counted apart from real ones, and so is the section directive of a kernel
that became a template instantiation (``.text`` -> its own comdat ``.section .text.<symbol>``: where the code lies, not what it is).  Exit status 1 on a real difference.

``--summary`` (anywhere on the command line) prints, for every really different kernel, what a reader needs to judge a refactoring that
moved code without meaning to change it, instead of the first lines of the diff:
    (a) the kernel descriptor's resource fields (next_free_vgpr, next_free_sgpr, accum_offset, group / private segment size), old -> new;
    (b) every mnemonic of the matrix, memory, LDS and synchronisation classes (v_mfma*, buffer_*, global_*, flat_*, ds_*, s_waitcnt*,
        s_barrier) whose count changed;
    (c) every other v_* mnemonic whose count changed -- v_cvt_f32_u32 / v_rcp_iflag_f32 (the pair a scalar integer division costs) apart;
and the scalar / s_nop mnemonics whose count changed, for completeness.  ``same`` means no count of that class changed: the kernel
then differs in register names, instruction order or scalar bookkeeping only."""
import collections
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
RES = ('next_free_vgpr', 'next_free_sgpr', 'accum_offset', 'group_segment_fixed_size', 'private_segment_fixed_size')
def resources(path):
    """{symbol: {field: value}} from the .amdhsa_kernel blocks"""
    out, cur = {}, None
    for ln in open(path):
        m = re.match(r'\s*\.amdhsa_kernel\s+(\S+)', ln)
        if m: cur = out.setdefault(m.group(1), {}); continue
        if '.end_amdhsa_kernel' in ln: cur = None; continue
        m = re.match(r'\s*\.amdhsa_(\w+)\s+(\S+)', ln)
        if m and cur is not None and m.group(1) in RES: cur[m.group(1)] = m.group(2)
    return out
def mnemonics(lines):
    c = collections.Counter()
    for l in lines:
        m = re.match(r'\s+([a-z]\w+)', l)
        if m and not l.lstrip().startswith('.'): c[m.group(1)] += 1
    return c
HEAVY = re.compile(r'^(v_mfma|buffer_|global_|flat_|ds_|s_waitcnt|s_barrier)')
DIVPAIR = re.compile(r'^(v_cvt_f32_u32|v_rcp_iflag_f32)')
def summary(name, old, new, ro, rn):
    co, cn = mnemonics(old), mnemonics(new)
    ch = {k: (co[k], cn[k]) for k in sorted(set(co) | set(cn)) if co[k] != cn[k]}
    fmt = lambda d: ', '.join(f'{k} {a}->{b}' for k, (a, b) in d.items()) or 'same'
    a = {k: (ro.get(k), rn.get(k)) for k in RES if ro.get(k) != rn.get(k)}
    b = {k: v for k, v in ch.items() if HEAVY.match(k)}
    c = {k: v for k, v in ch.items() if k.startswith('v_') and not HEAVY.match(k) and not DIVPAIR.match(k)}
    d = {k: v for k, v in ch.items() if DIVPAIR.match(k)}
    e = {k: v for k, v in ch.items() if k not in b and k not in c and k not in d}
    print(f'  {name}\n    instructions {sum(co.values())}->{sum(cn.values())}  (a) resources: {fmt(a)}  (b) mfma/memory/lds/sync: {fmt(b)}  (c) other vector: {fmt(c)}'
          f'  division pair: {fmt(d)}  scalar: {fmt(e)}')
    return not a and not b and not c
# template parameters that were removed: {kernel: the value (the old default) whose instantiations survive without the argument}
DROPPED = {'gemm_nt_kernel': '1'}        # KC, 16-wide K-chunks per LDS stage
def dem(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return dict(zip(names, r))
real = 0
SUMMARY = '--summary' in sys.argv
sys.argv = [a for a in sys.argv if a != '--summary']
old_dir, new_dir = sys.argv[1], sys.argv[2]
for f in (sys.argv[3:] or ['pwattn_fwd', 'pwattn_fwd_rw', 'pool_loss']):
    b, bo = funcs(os.path.join(old_dir, f + '.s')); n, no = funcs(os.path.join(new_dir, f + '.s'))
    db, dn = dem(bo), dem(no)
    inv = {v: k for k, v in dn.items()}
    same = diff = moved = within = gone = 0
    matched = set()
    if SUMMARY: rb, rn = resources(os.path.join(old_dir, f + '.s')), resources(os.path.join(new_dir, f + '.s'))
    for k in bo:
        d = db[k]
        cand = [d]
        m = re.match(r'^(void nrm::\w+<)([^>]*)(>\()', d)
        if m: cand.append(m.group(1) + m.group(2) + ', false' + m.group(3))
        if m and m.group(1)[len('void nrm::'):-1] in DROPPED and m.group(2).endswith(', ' + DROPPED[m.group(1)[len('void nrm::'):-1]]):
            cand.append(m.group(1) + m.group(2).rsplit(', ', 1)[0] + m.group(3))
        elif '<' not in d.split('(')[0]: cand.append('void ' + d.split('(')[0] + '<false>(')
        # prefix match on "name<args>(" since the argument list may have grown
        hit = None
        for c in cand:
            key = c.split('>(')[0] + '>(' if '>(' in c else c.split('(')[0] + '('
            hits = [x for x in dn.values() if x.startswith(key)]
            if len(hits) == 1: hit = inv[hits[0]]
        if hit is None:
            print(f, 'GONE', d[:120]); gone += 1; continue
        matched.add(hit)
        if b[k] == n[hit]: same += 1
        else:
            dl = [l for l in difflib.unified_diff(b[k], n[hit], lineterm='', n=0) if not l.startswith(('---', '+++', '@@'))]
            if all(re.search(r'\.amdhsa_kernarg_size|s_load_dword\w* \S+ s\[\d+:\d+\], 0x|^[-+]\s*\.text$|^[-+]\s*\.section\s+\.text\.SYM,', l) for l in dl):
                moved += 1
                continue
            diff += 1
            if SUMMARY: within += summary(d.split('(')[0], b[k], n[hit], rb.get(k, {}), rn.get(hit, {}))
            else: print(f, 'DIFF', d[:100], len(dl), 'lines'); print('\n'.join(dl[:12]))
    real += diff
    print(f'{f}: {len(bo)} existing instantiations: {gone} gone, {same} identical, {moved} differ only in the kernel-argument size / a hidden-argument offset / the section directive of a kernel that became a template, '
          f'{diff} really different; the new tree has {len(no)} kernels, {len(no) - len(matched)} of them without a counterpart in the old')
    if SUMMARY and diff: print(f'{f}: {within} of the {diff} different kernels keep (a) the resource fields, (b) the matrix / memory / LDS / synchronisation counts and (c) the other vector counts')
sys.exit(1 if real else 0)
