"""Kernel-by-kernel comparison of the gfx950 code of two builds (no GPU needed): for every object of
lib dir A and lib dir B, the device code object is taken out of the host object's .hip_fatbin section
and every kernel is compared under its mangled name -- disassembly (comments dropped, trailing
padding ignored; branches are pc-relative, so a kernel may move) and its entry in the code object's
metadata (registers, LDS, scratch, workgroup size, kernel arguments).  DESIGN.md 5.18.

    python tools/same_code.py OLD/spt-proto_amd/lib spt-proto_amd/lib [--grep attention]
"""
import glob, os, re, subprocess, sys, tempfile
LLVM = '/opt/rocm/llvm/bin/'
# behind a kernel's last instruction: alignment, zero words (as they disassemble), objdump's elision
PADDING = ('s_nop 0', 'v_cndmask_b32_e32 v0, s0, v0, vcc', '...')


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def kernels(lib):
    """mangled name -> set of (disassembly, metadata entry) over the objects of `lib`"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fb, co = os.path.join(tmp, 'fatbin'), os.path.join(tmp, 'gfx950.co')
        for obj in sorted(glob.glob(os.path.join(lib, '*.o'))):
            if '.hip_fatbin' not in run(LLVM + 'llvm-readelf', '-S', obj):
                continue                                    # (a unit without kernels)
            run(LLVM + 'llvm-objcopy', '--dump-section', '.hip_fatbin=' + fb, obj)
            run(LLVM + 'clang-offload-bundler', '--unbundle', '--type=o', '--input=' + fb, '--output=' + co,
                '--targets=hipv4-amdgcn-amd-amdhsa--gfx950')
            code = {}
            for part in re.split(r'\n(?=<\w+>:\n)', run(LLVM + 'llvm-objdump', '-d', '--no-show-raw-insn',
                                                         '--no-leading-addr', co)):
                m = re.match(r'<(\w+)>:\n', part)
                if m:
                    lines = [re.sub(r'\s*//.*', '', l).strip() for l in part[m.end():].splitlines()]
                    lines = [l for l in lines if l]
                    while lines and lines[-1] in PADDING:
                        lines.pop()
                    code[m.group(1)] = '\n'.join(lines)
            notes = run(LLVM + 'llvm-readelf', '--notes', co).split('amdhsa.kernels:\n', 1)[1]
            for entry in re.split(r'\n(?=  - )', notes.split('\namdhsa.target:')[0]):
                name = re.search(r'\.name:\s+(\w+)', entry).group(1)
                out.setdefault(name, set()).add((code[name], entry))
    return out


if __name__ == '__main__':
    pat = sys.argv[sys.argv.index('--grep') + 1] if '--grep' in sys.argv else ''
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = sorted(n for n in set(a) | set(b) if pat in n)
    same = [n for n in names if a.get(n) == b.get(n)]
    for n in names:
        if n not in same:
            print('{:<10} {}'.format('only old' if n not in b else 'only new' if n not in a else 'DIFFERENT', n))
    print('{} of {} kernels of the old build identical in the new one'.format(len(same), sum(n in a for n in names)))
    sys.exit(any(n in a and n in b for n in names if n not in same))
