#!/usr/bin/env python3
"""Instruction counts of a kernel's loops from the disassembly of the gfx950 code object inside a hipcc object file or library:
`tools/kernel_loop_count.py icicle_amd/lib/msm.o 'k_reduce_wave<icicle_hip::bn254_g1, true>'`. A loop is a backward branch; its
body is what lies between the target and the branch. Prints, for the whole kernel and for every loop, the instructions in all,
the 64-bit multiply-adds (v_mad_u64_u32 / v_mad_i64_i32), the other VALU, SALU, memory and waits. CPU-only: needs the ROCm llvm tools."""
import re
import subprocess
import sys
import tempfile

from kernel_regs import LLVM, code_objects


def classify(op):
    if op.startswith("v_mad_u64_u32") or op.startswith("v_mad_i64_i32"):
        return "mad64"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("s_"):
        return "salu"
    return "mem"  # global_ / flat_ / ds_ / buffer_ / scratch_


def main():
    path, want = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(path, tmp):
            txt = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--demangle", "--no-show-raw-insn", co], capture_output=True, text=True).stdout
            body, on = [], False
            for ln in txt.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.*)>:$", ln)
                if m:
                    name = m.group(1)
                    if not name.startswith("L") and not name.startswith("$"):  # (labels inside a function keep it open)
                        on = want in name and "(" in name and not name.startswith("__")
                    continue
                if on:
                    m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", ln)
                    if m:
                        body.append((int(m.group(3), 16), m.group(1), m.group(2)))
            if not body:
                continue
            addr_index = {a: i for i, (a, _, _) in enumerate(body)}

            def count(lo, hi):
                c = {"mad64": 0, "valu": 0, "salu": 0, "mem": 0, "wait": 0}
                for _, op, _ in body[lo:hi]:
                    c[classify(op)] += 1
                return c

            def show(tag, lo, hi):
                c = count(lo, hi)
                print(f"{tag:<28} total {hi - lo:>6}  mad64 {c['mad64']:>5}  other VALU {c['valu']:>5}  SALU {c['salu']:>4}  memory {c['mem']:>4}  waits {c['wait']:>4}")

            show("kernel", 0, len(body))
            for i, (a, op, args) in enumerate(body):
                if op.startswith("s_cbranch") or op == "s_branch":
                    # the target is printed as a label or as a signed word offset
                    m = re.search(r"<[^>]*\+0x([0-9a-f]+)>", args)
                    tgt = None
                    if re.fullmatch(r"-?\d+", args.split()[0] if args else ""):
                        off = int(args.split()[0])
                        off = off - 65536 if off >= 32768 else off
                        tgt = a + 4 + 4 * off
                    if tgt is not None and tgt <= a and tgt in addr_index:
                        show(f"loop {tgt:#x}..{a:#x}", addr_index[tgt], i + 1)
            return
    sys.exit(f"no kernel matching {want!r}")


if __name__ == "__main__":
    main()
