"""Per-symbol comparison of the device code of two builds of libfot.so: is every kernel of the old build, instruction
for instruction, in the new one?

    isa_compare.py <old libfot.so> <new libfot.so> [--arch gfx950] [--show N]

Both libraries are copied into a temporary directory, their code objects for the architecture are extracted
(`llvm-objdump --offloading`, one per translation unit) and disassembled (`llvm-objdump -d`).  A symbol's body is its
instruction lines with the addresses and encodings cut away; branch targets are kept as offsets from the symbol's own
start, so a kernel that merely moved inside its code object compares equal and one whose control flow changed does
not.  The one literal that depends on where things lie in the code object -- the 32-bit offset a `s_add_u32` adds to the
result of the `s_getpc_b64` before it -- is replaced by what it points at (symbol + offset, from the code object's symbol
table).  The `s_nop 0` padding the assembler puts behind a symbol's last instruction, up to the next symbol's alignment,
is not part of its body.  Reported: the symbols compared, the symbols only one side has, and every symbol whose bodies differ (with the
first `--show` differing lines, default 6).  Exit status 0: every symbol of the old build exists in the new one with
the same instructions; 1 otherwise.  The new build may have more symbols.
"""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

OBJDUMP = '/opt/rocm/llvm/bin/llvm-objdump' if os.path.exists('/opt/rocm/llvm/bin/llvm-objdump') else shutil.which('llvm-objdump')
RE_SYM = re.compile(r'^([0-9a-f]+) <([^>]+)>:$')
RE_INS = re.compile(r'^\s+(.*?)\s*//\s*([0-9A-Fa-f]+):')
RE_TARGET = re.compile(r'<([^>+]+)(?:\+0x([0-9a-f]+))?>')
RE_GETPC = re.compile(r's_getpc_b64 s\[(\d+):\d+\]')
RE_ADDLO = re.compile(r'(s_add_u32 s(\d+), s\d+, )(0x[0-9a-f]+|-?\d+)$')


def symbol_table(co):
    """sorted (address, name) of the code object's defined symbols"""
    text = subprocess.run([OBJDUMP, '-t', co], check=True, capture_output=True, text=True).stdout
    tab = []
    for line in text.splitlines():
        f = line.split()
        if len(f) >= 5 and re.fullmatch(r'[0-9a-f]{16}', f[0]) and f[-1] != '*ABS*' and not f[-1].startswith('.'):
            tab.append((int(f[0], 16), f[-1]))
    return sorted(tab)


def resolve(tab, addr):
    best = None
    for a, n in tab:
        if a <= addr:
            best = (a, n)
        else:
            break
    return '%s+%d' % (best[1], addr - best[0]) if best else '?'


def symbols(lib, arch, tmp, tag):
    """symbol -> list of instruction texts, over every code object of `lib` for `arch`"""
    d = os.path.join(tmp, tag)
    os.makedirs(d)
    copy = os.path.join(d, 'lib.so')
    shutil.copy(lib, copy)
    subprocess.run([OBJDUMP, '--offloading', copy], check=True, stdout=subprocess.DEVNULL, cwd=d)
    out = {}
    for co in sorted(glob.glob(copy + '.*' + arch)):
        text = subprocess.run([OBJDUMP, '-d', co], check=True, capture_output=True, text=True).stdout
        tab = symbol_table(co)
        name = None
        pc = {}                                                   # SGPR -> value a s_getpc_b64 left in it
        for line in text.splitlines():
            m = RE_SYM.match(line)
            if m:
                name = m.group(2)
                out[name] = []
                continue
            m = RE_INS.match(line)
            if m and name is not None:
                addr = int(m.group(2), 16)
                g = RE_GETPC.search(m.group(1))
                if g:
                    pc = {int(g.group(1)): addr + 4}
                a = RE_ADDLO.search(m.group(1))
                if a and int(a.group(2)) in pc:
                    target = (pc.pop(int(a.group(2))) + int(a.group(3), 0)) & 0xffffffff
                    out[name].append(a.group(1) + '<pc-relative: ' + resolve(tab, target) + '>')
                    continue
                # a branch target prints as <symbol+0xoff>: already relative to the symbol; absolute addresses are not in the text
                out[name].append(RE_TARGET.sub(lambda t: '<' + t.group(1) + '+' + (t.group(2) or '0') + '>', m.group(1)))
    for body in out.values():                                    # alignment padding behind the last instruction
        while body and body[-1] in ('s_nop 0', 's_code_end'):
            body.pop()
    return out


def main(argv):
    if len(argv) < 3 or not OBJDUMP:
        print(__doc__)
        return 2
    arch = argv[argv.index('--arch') + 1] if '--arch' in argv else 'gfx950'
    show = int(argv[argv.index('--show') + 1]) if '--show' in argv else 6
    with tempfile.TemporaryDirectory() as tmp:
        old = symbols(argv[1], arch, tmp, 'old')
        new = symbols(argv[2], arch, tmp, 'new')
    if not old:
        print(f'no {arch} code in {argv[1]}')
        return 1
    gone = sorted(set(old) - set(new))
    added = sorted(set(new) - set(old))
    differ = []
    n_ins = 0
    for name in sorted(set(old) & set(new)):
        n_ins += len(old[name])
        if old[name] != new[name]:
            differ.append(name)
    print(f'symbols compared: {len(set(old) & set(new))} ({n_ins} instructions); differing: {len(differ)}; '
          f'only in the old build: {len(gone)}; only in the new build: {len(added)}')
    for name in gone:
        print(f'  only old: {name}')
    for name in added:
        print(f'  only new: {name} ({len(new[name])} instructions)')
    for name in differ:
        a, b = old[name], new[name]
        print(f'  DIFFERS: {name}: {len(a)} -> {len(b)} instructions')
        shown = 0
        for k in range(max(len(a), len(b))):
            x = a[k] if k < len(a) else '-'
            y = b[k] if k < len(b) else '-'
            if x != y:
                print(f'     [{k}] {x}   |   {y}')
                shown += 1
                if shown >= show:
                    break
    return 1 if differ or gone else 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
