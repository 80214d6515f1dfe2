#!/usr/bin/env python
"""Which kernels of two builds of a translation unit have other INSTRUCTIONS (an object-code diff beside tools/kernel_code_hash.py).

    python tools/kernel_code_diff.py OLD.o NEW.o [NEW2.o ...]

Disassembles the gfx950 code object of the host objects and compares every function instruction by instruction.  Several NEW objects are one
translation unit split up: their functions are taken together, a function that two of them hold with the same code (a linkonce copy) counts
once, and one they hold with different code is `CHANGED`.  A kernel that only moved
inside .text differs in the bytes of its pc-relative displacements -- the two literals behind an `s_getpc_b64` that form the address of a
called function -- and in nothing else: those literals are masked, so such a kernel counts as unchanged and is reported as `moved`.
A kernel whose instructions differ, but which has the same NUMBER of instructions, the same multiset of mnemonics and the same resources
in its kernel descriptor (VGPRs, SGPRs, AGPRs, scratch bytes, static LDS, spill counts), is reported as `renamed`: what the compiler does
when source moves between functions -- other register numbers, another order of independent instructions, an inverted branch.  The
mnemonic is the operation: the disassembler's `_e32` / `_e64` suffix names the ENCODING, which follows from the registers (a compare that
writes an SGPR pair instead of VCC has no 32-bit encoding), so it is left out of the multiset and the line says how many instructions
took the other encoding.  Only a `CHANGED` kernel (or one that exists in one object only) makes the exit status non-zero.
"""
import collections
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_code_hash import LLVM, code_object  # noqa: E402


RESOURCES = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count")


def resources(co):
    """{demangled kernel name: the resource numbers of its descriptor}, from the code object's metadata note"""
    txt = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    out, cur = {}, {}
    for l in txt.splitlines() + ["  - "]:
        if re.match(r"^\s+- ", l) and not l.startswith("      "):  # the next entry of amdhsa.kernels
            if ".name" in cur:
                out[cur[".name"]] = tuple(cur.get("." + k) for k in RESOURCES)
            cur = {}
        m = re.match(r"^\s+(?:- )?(\.\w+):\s+(\S+)$", l)
        if m and not l.startswith("      "):
            cur[m.group(1)] = m.group(2)
    # the disassembly names functions demangled: the symbol table printed both ways pairs the names, line by line
    sym = [subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", *flag, co], check=True, capture_output=True, text=True).stdout.splitlines()
           for flag in ([], ["--demangle"])]
    pat = r"\s*\d+:\s+[0-9a-f]+\s+\d+\s+FUNC\s+\S+\s+\S+\s+\S+\s+(.*)$"
    pairs = [(re.match(pat, m), re.match(pat, d)) for m, d in zip(*sym)]
    return {d.group(1).strip(): out[m.group(1).strip()] for m, d in pairs if m and d and m.group(1).strip() in out}


def functions(obj, tmp):
    co = code_object(obj, tmp)
    res = resources(co)
    txt = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", "--no-show-raw-insn", "--no-leading-addr", co], check=True, capture_output=True,
                         text=True).stdout
    out, name, pcrel = {}, None, 0
    for l in txt.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(.*)>:$", l.strip())
        if m:
            name, pcrel = m.group(1), 0
            out[name] = ([], [], res.get(name))  # (masked, exact, resources of a kernel)
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
    # the fill behind a function's last instruction (up to the next function's alignment, or the end of .text) belongs to where the function
    # lies, not to the function: a unit that was split up lays its functions out anew
    # -- cut only behind an instruction that ends the function (no fall-through into the fill), and only what is fill
    fill = ("s_nop 0", "s_code_end", "...")  # ("...": the disassembler's run of zero bytes)
    for masked, exact, _ in out.values():
        n = len(masked)
        while n and masked[n - 1] in fill:
            n -= 1
        if n and masked[n - 1].split(" ")[0] in ("s_endpgm", "s_setpc_b64", "s_branch"):
            del masked[n:], exact[n:]
    return out


def main():
    old, news = sys.argv[1], sys.argv[2:]
    changed = 0
    with tempfile.TemporaryDirectory() as t1:
        fa = functions(old, t1)
    fb = {}
    for new in news:  # the functions of all NEW objects together: identical linkonce copies count once
        with tempfile.TemporaryDirectory() as t2:
            sections = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-SW", new], check=True, capture_output=True, text=True).stdout
            if ".hip_fatbin" not in sections:  # a host-only part of the split unit
                print("no device code:", new)
                continue
            for n, f in functions(new, t2).items():
                if n in fb and (fb[n][0], fb[n][2]) != (f[0], f[2]):
                    print(f"CHANGED {n}: two NEW objects hold it with different code ({len(fb[n][0])} and {len(f[0])} instructions)")
                    changed += 1
                fb.setdefault(n, f)
    for n in sorted(set(fa) | set(fb)):
        a, b = fa.get(n), fb.get(n)
        if a is None or b is None:
            print("only in one:", n)
            changed += 1
        elif a[0] != b[0]:
            encoded = [collections.Counter(i.split(" ")[0] for i in f[0]) for f in (a, b)]
            mnemonics = [collections.Counter({}) for _ in encoded]
            for m, e in zip(mnemonics, encoded):
                for k, cnt in e.items():
                    m[re.sub(r"_e(32|64)$", "", k)] += cnt
            if len(a[0]) == len(b[0]) and mnemonics[0] == mnemonics[1] and a[2] == b[2]:
                other = sum((encoded[0] - encoded[1]).values())
                print(f"renamed {n}: {len(a[0])} instructions, same mnemonics and resources, other registers or order" +
                      (f" ({other} in the other VOP encoding)" if other else ""))
            else:
                print(f"CHANGED {n}: {len(a[0])} -> {len(b[0])} instructions, resources {a[2]} -> {b[2]}")
                changed += 1
        elif a[1] != b[1]:
            print(f"moved   {n}: same instructions, other pc-relative displacement")
        else:
            print(f"same    {n}")
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main())
