"""Is the device code of two source trees the same, kernel for kernel?  The acceptance test of a host-side refactor: no tolerance, equal or not equal.

    python tools/isa_equal.py TREE_A TREE_B [file.hip ...]      (trees: repository roots; default: every tcct_amd/csrc/*.hip of either tree)

Compiles the device side of each file of both trees to gfx950 assembly (isa_scan.compile_asm: the library's flags; no GPU) and compares, per kernel symbol, the function's
text (instructions, the .amdhsa_ descriptor, the resource `.set`s and the "Kernel info" block: VGPR / SGPR / LDS / scratch) and its entry of the amdhsa.kernels metadata
(argument layout, spill counts).  Function numbers in local labels (.LBB12_3, BB12_3 in comments) are masked: they count the functions in front, i.e. the order in which
host code first names the template instantiations, and are not code.  The `__hip_cuid_<hash>` symbol differs between any two compiles; it lies outside every kernel and
is not looked at.  Exit status 1 if a kernel differs, if the sets of kernel symbols differ or if a compile fails."""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

from isa_scan import compile_asm

LABEL = re.compile(r'(\.L[A-Za-z_]+|\bBB)\d+')


def kernels(asm):
    """{kernel symbol: (function text, metadata entry)} of one assembly file"""
    s = re.sub(r'[ \t]+;', ' ;', LABEL.sub(r'\1#', open(asm).read()))      # (comments are aligned to a column: the width of a masked number must not show)
    meta = {}
    m = re.search(r'\namdhsa\.kernels:\n(.*?)\n(?=\S)', s, re.S)
    for entry in re.split(r'\n  - ', '\n' + m.group(1))[1:] if m else []:
        meta[re.search(r'\.name:\s+(\S+)', entry).group(1)] = entry
    out = {}
    for name in re.findall(r'\n\t\.amdhsa_kernel (\S+)\n', s):
        i0 = s.index('\n' + name + ':')
        # up to the next function's section (the kernel's own .text section is re-entered after its descriptor) or, behind the last one, the end-of-code padding
        ends = [m.start() for m in re.finditer(r'\n\t(?:\.section\t(?:\.text|\.AMDGPU\.gpr_maximums)[^\n]*|\.text(?=\n))', s[i0:]) if name + ',' not in m.group(0)]
        out[name] = (s[i0:i0 + ends[0]] if ends else s[i0:], meta.get(name))
    return out


def main():
    a, b, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    bases = sorted({os.path.basename(f) for f in files} or {os.path.basename(f) for t in (a, b) for f in glob.glob(os.path.join(t, 'tcct_amd', 'csrc', '*.hip'))})
    n_same = n_diff = n_only = 0
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(min(8, os.cpu_count() or 1)) as pool:
        jobs = {}
        for side, tree in (('a', a), ('b', b)):
            os.mkdir(os.path.join(tmp, side))
            for base in bases:
                jobs[side, base] = pool.submit(compile_asm, os.path.join(tree, 'tcct_amd', 'csrc', base), os.path.join(tmp, side))
        for base in bases:
            (asm_a, log_a), (asm_b, log_b) = jobs['a', base].result(), jobs['b', base].result()
            if asm_a is None or asm_b is None:
                print(f'{base}: compile failed\n' + (log_a if asm_a is None else log_b)[-800:])
                n_diff += 1
                continue
            ka, kb = kernels(asm_a), kernels(asm_b)
            names = sorted(set(ka) | set(kb))
            dem = subprocess.run(['c++filt'], input='\n'.join(names), stdout=subprocess.PIPE, text=True).stdout.split('\n')
            same = 0
            for name, dn in zip(names, dem):
                if name not in ka or name not in kb:
                    print(f'{base}: ONLY IN {"A" if name in ka else "B"}: {dn[:160]}')
                    n_only += 1
                elif ka[name] != kb[name]:
                    print(f'{base}: DIFFERENT ({"code" if ka[name][0] != kb[name][0] else "metadata"}): {dn[:160]}')
                    n_diff += 1
                else:
                    same += 1
            n_same += same
            print(f'{base}: {same} of {len(names)} kernels identical', flush=True)
    print(f'isa_equal: {len(bases)} files, {n_same} kernels identical, {n_diff} different, {n_only} in one tree only')
    return 1 if n_diff or n_only else 0


if __name__ == '__main__':
    sys.exit(main())
