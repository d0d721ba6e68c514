#!/usr/bin/env python3
"""Are the kernels of two device code objects the same machine code?

    hipcc <the Makefile's flags> --cuda-device-only --no-gpu-bundle-output -c gemm.hip -o old/gemm.o     (parent)
    hipcc <the Makefile's flags> --cuda-device-only --no-gpu-bundle-output -c gemm.hip -o new/gemm.o     (result)
    python tools/kernel_identity.py old/gemm.o new/gemm.o [--renames map.json] [--markdown]

Compared per kernel (a symbol S with a descriptor S.kd), read straight from the ELF -- no disassembler, so a function's position in the file does not matter:
  * the encoded instruction bytes of S (st_value / st_size in .text);
  * the 64-byte kernel descriptor S.kd.  Its KERNEL_CODE_ENTRY_BYTE_OFFSET (bytes 16..23) is the distance from the descriptor to the code and moves with the
    layout: it is resolved to the symbol it points at (which must be S) and left out of the byte comparison.
The rename map is a JSON object {old mangled name: new mangled name} for instantiations whose template argument list changed.  Whole files are NOT compared
(notes and symbol order differ between two compiles of the same source).  Exit status 0 = same set of kernels, every pair identical.
"""
import argparse
import json
import struct
import subprocess
import sys


def read_elf(path):
    """-> {name: (bytes, address)} of every sized symbol that lives in a PROGBITS section"""
    d = open(path, 'rb').read()
    assert d[:4] == b'\x7fELF' and d[4] == 2 and d[5] == 1, f'{path}: not a little-endian ELF64'
    shoff, = struct.unpack_from('<Q', d, 0x28)
    shentsize, shnum, _ = struct.unpack_from('<HHH', d, 0x3A)
    secs = [struct.unpack_from('<IIQQQQIIQQ', d, shoff + i * shentsize) for i in range(shnum)]      # name, type, flags, addr, offset, size, link, info, align, entsize
    symtab = next(s for s in secs if s[1] == 2)
    stroff = secs[symtab[6]][4]
    out = {}
    for off in range(symtab[4], symtab[4] + symtab[5], 24):
        name_i, _, _, shndx, value, size = struct.unpack_from('<IBBHQQ', d, off)
        if not size or not 0 < shndx < shnum or secs[shndx][1] != 1:
            continue
        name = d[stroff + name_i:d.index(b'\0', stroff + name_i)].decode()
        fo = secs[shndx][4] + value - secs[shndx][3]
        out[name] = (d[fo:fo + size], value)
    return out


def kernels(path):
    """-> {kernel: (code bytes, descriptor with the entry offset zeroed, name of the symbol the entry offset points at)}"""
    syms = read_elf(path)
    by_addr = {addr: n for n, (_, addr) in syms.items() if not n.endswith('.kd')}
    out = {}
    for n, (kd, kd_addr) in syms.items():
        if not n.endswith('.kd'):
            continue
        assert len(kd) == 64, f'{n}: descriptor of {len(kd)} bytes'
        entry, = struct.unpack_from('<q', kd, 16)
        out[n[:-3]] = (syms[n[:-3]][0], kd[:16] + bytes(8) + kd[24:], by_addr.get(kd_addr + entry, '?'))
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True).stdout.split('\n')
        return dict(zip(names, r))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('old'); ap.add_argument('new')
    ap.add_argument('--renames', help='JSON {old mangled name: new mangled name}')
    ap.add_argument('--markdown', action='store_true', help='print the per-kernel table as a markdown table')
    a = ap.parse_args()
    ren = json.load(open(a.renames)) if a.renames else {}
    old, new = kernels(a.old), kernels(a.new)
    for o, n in ren.items():
        if (o in old) != (n in new):          # (a map may serve several objects: a pair that neither side has is another file's)
            sys.exit(f'rename {o} -> {n}: {"old" if o not in old else "new"} side has no such kernel')
    pairs = [(o, ren.get(o, o)) for o in sorted(old)]
    lost = [o for o, n in pairs if n not in new]
    added = sorted(set(new) - {n for _, n in pairs})
    nice = demangle([n for _, n in pairs if n in new])
    rows, bad = [], 0
    for o, n in pairs:
        if n not in new:
            continue
        (oc, okd, oent), (nc, nkd, nent) = old[o], new[n]
        code_eq, kd_eq = oc == nc, okd == nkd and oent == o and nent == n
        bad += not (code_eq and kd_eq)
        rows.append((nice[n].replace('|', '\\|'), 'renamed' if o != n else '', len(nc), 'equal' if code_eq else f'DIFFERENT (old {len(oc)} B)', 'equal' if kd_eq else 'DIFFERENT'))
    if a.markdown:
        print('| kernel | | code bytes | code | descriptor |\n|---|---|---:|---|---|')
        for r in rows: print('| `%s` | %s | %d | %s | %s |' % r)
    else:
        for r in rows: print('%-9s %8d  code %-9s kd %-9s %s' % (r[1], r[2], r[3], r[4], r[0]))
    print(f'\n{len(old)} kernels in {a.old}, {len(new)} in {a.new}: {len(rows) - bad} identical pairs ({sum(1 for o, n in pairs if o != n and n in new)} renamed), '
          f'{bad} different, {len(lost)} lost, {len(added)} added')
    for k in lost: print('lost : ' + k)
    for k in added: print('added: ' + k)
    return 1 if bad or lost or added else 0


if __name__ == '__main__':
    sys.exit(main())
