#!/usr/bin/env python3
"""Compare the gfx950 code of every kernel of one source file between two checkouts (or two .s files).

    tools/kernel_isa_diff.py OLD NEW gemm.hip [gemm_dp.hip ...]

OLD / NEW: a checkout root (the file is taken from audio-visual-llm_amd/csrc and cross-compiled exactly as tests/test_codegen_cpu.py does)
or an assembly file (then exactly one source name is given, for the heading only).  Per kernel symbol: `same opcode sequence`, or the
opcodes whose counts differ; then the metadata of both sides.  A plain opcode and metadata comparison: it knows no particular instruction.
--rename REGEX=REPL (repeatable): applied to the mangled kernel names of both sides before they are paired, for a change that adds or drops
a template parameter, e.g. --rename 'fooILi(\\d+)ELNS_4ModeE\\dE.*=foo<\\1>' --rename 'fooILi(\\d+)E.*=foo<\\1>'."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

CLANG = "/opt/rocm/lib/llvm/bin/clang++"
META = ["vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"]


def asm_of(side, name, tmp):
    if os.path.isfile(side):
        return open(side).read()
    src = os.path.join(side, "audio-visual-llm_amd", "csrc", name)
    out = os.path.join(tmp, name + ".s")
    r = subprocess.run([CLANG, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", os.path.join(side, "include"), "-x", "hip", src,
                        "--cuda-device-only", "-S", "-o", out], capture_output=True, text=True)
    if r.returncode:
        sys.exit(r.stderr[-4000:])
    return open(out).read()


def kernels(asm):
    """{symbol: [instruction lines]} of the kernels (the symbols the metadata names) and {symbol: {key: value}}."""
    meta = {}
    for blk in asm[asm.index("amdhsa.kernels:"):].split("  - .agpr_count")[1:]:
        blk = ".agpr_count" + blk
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        meta[name] = {k: int(re.search(r"\." + k + r":\s+(\d+)", blk).group(1)) for k in META}
    code = {}
    for name in meta:
        body = asm.split("\n" + name + ":", 1)[1].split("\n.Lfunc_end")[0]      # whole function: early returns end the program more than once
        ins = []
        for l in body.split("\n"):
            l = l.split(";")[0].strip()
            if not l or l.startswith(".") or l.endswith(":") or l.startswith("//"):
                continue
            ins.append(l)
        code[name] = ins
    return code, meta


def renamed(code, meta, renames):
    """code and meta keyed by the kernel name after the substitutions REGEX=REPL."""
    key = {}
    for n in code:
        key[n] = n
        for r in renames:
            pat, repl = r.split("=", 1)
            key[n] = re.sub(pat, repl, key[n])
    assert len(set(key.values())) == len(key), "--rename maps two kernels of one side to the same name"
    return {key[n]: code[n] for n in code}, {key[n]: meta[n] for n in code}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("sources", nargs="+")
    ap.add_argument("--rename", action="append", help="REGEX=REPL on the kernel names of both sides before pairing")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as t0, tempfile.TemporaryDirectory() as t1:
        for name in a.sources:
            (c0, m0), (c1, m1) = kernels(asm_of(a.old, name, t0)), kernels(asm_of(a.new, name, t1))
            if a.rename:
                (c0, m0), (c1, m1) = renamed(c0, m0, a.rename), renamed(c1, m1, a.rename)
            print(f"== {name}")
            for k in sorted(set(c0) | set(c1)):
                if k not in c0 or k not in c1:
                    print(f"{k}\n  only in {'old' if k in c0 else 'new'}")
                    continue
                o0, o1 = [l.split()[0] for l in c0[k]], [l.split()[0] for l in c1[k]]
                print(k)
                if o0 == o1:
                    print(f"  same opcode sequence ({len(o0)} instructions)")
                else:
                    n0, n1 = collections.Counter(o0), collections.Counter(o1)
                    d = {op: (n0[op], n1[op]) for op in sorted(set(n0) | set(n1)) if n0[op] != n1[op]}
                    print(f"  opcode sequences differ ({len(o0)} -> {len(o1)} instructions); counts that differ: " +
                          (", ".join(f"{op} {x}->{y}" for op, (x, y) in d.items()) or "none (order only)"))
                same = m0[k] == m1[k]
                print("  metadata " + ("same: " if same else "DIFFERS: ") +
                      ", ".join(f"{key} {m0[k][key]}" if m0[k][key] == m1[k][key] else f"{key} {m0[k][key]}->{m1[k][key]}" for key in META))


if __name__ == "__main__":
    main()
