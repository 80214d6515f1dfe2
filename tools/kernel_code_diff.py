#!/usr/bin/env python
"""Which kernels of two builds of a translation unit have other INSTRUCTIONS (an object-code diff beside tools/kernel_code_hash.py).

    python tools/kernel_code_diff.py OLD.o NEW.o

Disassembles the gfx950 code object of both host objects and compares every function instruction by instruction.  A kernel that only moved
inside .text differs in the bytes of its pc-relative displacements -- the two literals behind an `s_getpc_b64` that form the address of a
called function -- and in nothing else: those literals are masked, so such a kernel counts as unchanged and is reported as `moved`.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_code_hash import LLVM, code_object  # noqa: E402


def functions(obj, tmp):
    co = code_object(obj, tmp)
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                         text=True).stdout
    out, name, pcrel = {}, None, 0
    for l in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", l.strip())
        if m:
            name, pcrel = m.group(1), 0
            out[name] = ([], [])  # (masked, exact)
            continue
        if name is None or not l.strip():
            continue
        ins = re.sub(r"\s*//.*$", "", l.strip())
        ins = re.sub(r"\s+", " ", ins)
        exact = ins
        if ins.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_addc?_u32 ", ins):
            ins = re.sub(r", (0x[0-9a-f]+|-?\d+)$", ", <pcrel>", ins)
            pcrel -= 1
        if re.match(r"s_c?branch|s_call", ins):  # branch targets are printed as addresses: keep the mnemonic
            ins = ins.split(" ")[0]
            exact = ins
        out[name][0].append(ins)
        out[name][1].append(exact)
    return out


def main():
    old, new = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as t1, tempfile.TemporaryDirectory() as t2:
        fa, fb = functions(old, t1), functions(new, t2)
    changed = 0
    for n in sorted(set(fa) | set(fb)):
        a, b = fa.get(n), fb.get(n)
        if a is None or b is None:
            print("only in one:", n)
            changed += 1
        elif a[0] != b[0]:
            print(f"CHANGED {n}: {len(a[0])} -> {len(b[0])} instructions")
            changed += 1
        elif a[1] != b[1]:
            print(f"moved   {n}: same instructions, other pc-relative displacement")
        else:
            print(f"same    {n}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
