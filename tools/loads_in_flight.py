#!/usr/bin/env python
"""How many vector-memory loads does a kernel have in flight between two waits?

Reads the gfx950 disassembly of the built library (vbx_amd.build.disassemble(), no GPU needed) and prints, for every
kernel whose demangled name contains one of the given substrings, the sequence of vector-memory loads and
`s_waitcnt vmcnt(n)` waits in program order -- runs of loads as `L x n`, waits as `W(n)`, barriers as `|` -- with the
largest number of loads issued between two waits and the number of loads that sit directly behind a full wait
(`vmcnt(0)`) with a single load in front of it: the signature of loads that were meant to be in flight together and are
issued one round trip at a time.  Program order is not execution order (loops, branches): the listing is what to read,
the figures say where to look.

usage: tools/loads_in_flight.py [--lib PATH] [--asm FILE] [--full] substring [substring ...]
"""
from __future__ import annotations

import argparse
import os
import re
import subprocess
import sys

_LOAD = re.compile(r'^(global_load_|buffer_load_|flat_load_|scratch_load_)')
_VMCNT = re.compile(r'vmcnt\((\d+)\)')


def kernels(asm: str):
    """(mangled name, [instruction text]) for every function of an llvm-objdump -d listing."""
    name, body = None, []
    for line in asm.splitlines():
        if line.endswith('>:'):
            if name is not None:
                yield name, body
            name, body = line.split('<', 1)[-1][:-2], []
            continue
        if name is None:
            continue
        code = line.split('//')[0].strip()
        if code:
            body.append(code)
    if name is not None:
        yield name, body


def events(body):
    """The loads, vmcnt waits and barriers of a kernel in program order: ('L', mnemonic) / ('W', n) / ('B', None).

    An `s_waitcnt` without a vmcnt field does not wait for vector memory and is left out.
    """
    out = []
    for code in body:
        op = code.split()[0]
        if _LOAD.match(op):
            out.append(('L', op))
        elif op == 's_waitcnt':
            m = _VMCNT.search(code)
            if m:
                out.append(('W', int(m.group(1))))
        elif op == 's_barrier':
            out.append(('B', None))
    return out


def summarize(ev):
    """loads, waits, full waits, the largest run of loads without a wait between them, and the number of single loads
    enclosed by full waits (`W(0) L W(0)`)."""
    loads = sum(1 for k, _ in ev if k == 'L')
    waits = [v for k, v in ev if k == 'W']
    best = run = 0
    lone = 0
    mem = [(k, v) for k, v in ev if k != 'B']
    for k, _ in mem:
        if k == 'L':
            run += 1
            best = max(best, run)
        else:
            run = 0
    for a, b, c in zip(mem, mem[1:], mem[2:]):
        if a == ('W', 0) and b[0] == 'L' and c == ('W', 0):
            lone += 1
    return {'loads': loads, 'waits': len(waits), 'full_waits': sum(1 for w in waits if w == 0),
            'max_loads_between_waits': best, 'lone_loads_between_full_waits': lone}


def compact(ev) -> str:
    parts, i = [], 0
    while i < len(ev):
        k, v = ev[i]
        if k == 'L':
            j = i
            while j < len(ev) and ev[j][0] == 'L':
                j += 1
            parts.append(f'L x {j - i}')
            i = j
            continue
        parts.append(f'W({v})' if k == 'W' else '|')
        i += 1
    return ' '.join(parts)


def demangle(names):
    try:
        res = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True, check=True)
        out = res.stdout.splitlines()
        if len(out) == len(names):
            return out
    except (OSError, subprocess.CalledProcessError):
        pass
    return list(names)


def short(name: str) -> str:
    return re.sub(r'\(vbx::BatchView<\w+>\)', '', name).replace('vbx::', '').replace('void ', '')


def report(asm: str, want, full: bool = False) -> str:
    ks = list(kernels(asm))
    names = [short(n) for n in demangle([k for k, _ in ks])]
    lines = []
    for nm, (_, body) in zip(names, ks):
        if not any(w in nm for w in want):
            continue
        ev = events(body)
        s = summarize(ev)
        lines.append(f'{nm}\n  loads {s["loads"]}  vmcnt waits {s["waits"]} (full: {s["full_waits"]})  most loads between two waits '
                     f'{s["max_loads_between_waits"]}  lone loads between full waits {s["lone_loads_between_full_waits"]}')
        lines.append('  ' + compact(ev))
        if full:
            lines += [f'    {v}' if k == 'L' else f'    s_waitcnt vmcnt({v})' if k == 'W' else '    s_barrier' for k, v in ev]
    return '\n'.join(lines) + '\n'


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--lib', default=None, help='library to disassemble (default: the built one)')
    ap.add_argument('--asm', default=None, help='read a listing from this file instead')
    ap.add_argument('--full', action='store_true', help='also list every event on a line of its own')
    ap.add_argument('kernels', nargs='+', help='substrings of demangled kernel names')
    a = ap.parse_args()
    if a.asm:
        with open(a.asm) as fh:
            asm = fh.read()
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from vbx_amd import build
        asm = build.disassemble(a.lib)
    sys.stdout.write(report(asm, a.kernels, a.full))


if __name__ == '__main__':
    main()
