#!/usr/bin/env python3
"""Compare two hipcc --offload-device-only -S outputs kernel by kernel: the
instruction streams of every *kernel* symbol with comments, directives and
labels stripped.  The check of a refactor that should not move code.

  python tools/isa_diff.py OLD.s NEW.s [--opcodes]

One line per kernel: SAME or DIFF and both static instruction counts.
--opcodes compares the mnemonics only (operands, e.g. kernel-argument
offsets, may differ).  Exit status 1 if any kernel differs or is missing.
"""
import re
import sys


def kernels(path, opcodes):
    out, cur = {}, None
    for l in open(path):
        m = re.match(r"^(\w*kernel\w*):", l)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        s = l.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            cur = None
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        cur.append(s.split()[0] if opcodes else " ".join(s.split()))
    return out


def main():
    opcodes = "--opcodes" in sys.argv
    a, b = (kernels(f, opcodes) for f in sys.argv[1:3])
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"ONLY-{'OLD' if name in a else 'NEW'} {name}")
            bad = 1
            continue
        same = a[name] == b[name]
        bad |= not same
        print(f"{'SAME' if same else 'DIFF'} {len(a[name]):6d} {len(b[name]):6d}  {name}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
