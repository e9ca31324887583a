#!/usr/bin/env python3
"""Driver of tools/ubench/mont_forms.hip: compiles it for gfx950, reads the instruction mix of every form's
timing kernel out of the compiler's assembly (the largest basic block = the product loop), and -- with --run, on
a machine with a GPU -- runs the binary and prints its rates under the mix.

    python tools/ubench/mont_forms.py --out-dir /tmp/mont_forms            # compile + instruction mix
    python tools/ubench/mont_forms.py --out-dir /tmp/mont_forms --run      # ... and the rates
    python tools/ubench/mont_forms.py --out-dir /tmp/mont_forms --run --no-build   # a binary built elsewhere
"""
import argparse
import collections
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FORMS = ["a opscan", "b pinned colscan", "c pinned lockstep x2", "d asm-mad colscan", "e asm-mad lockstep x2", "f asm-mad3 colscan",
         "g plain colscan", "h asm-column colscan"]
PRODUCTS_PER_ITERATION = {2: 2, 4: 2}          # the lockstep forms do two products per loop iteration


def build(out_dir: str) -> None:
    os.makedirs(out_dir, exist_ok=True)
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--save-temps", os.path.join(HERE, "mont_forms.hip"), "-o", "mont_forms"],
                   check=True, cwd=out_dir)


def blocks_of(asm_path: str):
    """-> {kernel name: [[mnemonic, ...] per basic block]}"""
    out, cur = {}, None
    for line in open(asm_path):
        m = re.match(r"^(_Z12forms_kernel\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [[]])
            continue
        if cur is None:
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
        elif re.match(r"^\.LBB\w+:", line):
            cur.append([])
        else:
            word = line.split(";")[0].split()
            if word and line[0] in " \t" and not word[0].startswith("."):
                cur[-1].append(word[0])
    return out


def mix_table(out_dir: str, waves: int = 4) -> str:
    asm = os.path.join(out_dir, "mont_forms-hip-amdgcn-amd-amdhsa-gfx950.s")
    kernels = blocks_of(asm)
    lines = [f"instruction mix of the product loop (largest basic block of the timing kernel at {waves} waves per SIMD), per product",
             f"{'form':26s} {'VALU':>7s} {'v_mad_u64_u32':>14s} {'v_lshl_add_u64':>15s} {'v_lshrrev_b64':>14s} {'s_nop':>7s}"]
    for form, name in enumerate(FORMS):
        block = max(kernels[f"_Z12forms_kernelILi{form}ELi{waves}ELb0EEvPjji"], key=len)
        c = collections.Counter(block)
        per = PRODUCTS_PER_ITERATION.get(form, 1)
        valu = sum(n for ins, n in c.items() if ins.startswith("v_"))
        lines.append(f"{name:26s} {valu / per:7.1f} {c['v_mad_u64_u32'] / per:14.1f} {c['v_lshl_add_u64'] / per:15.1f} "
                     f"{c['v_lshrrev_b64'] / per:14.1f} {c['s_nop'] / per:7.1f}")
    return "\n".join(lines)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", required=True)
    ap.add_argument("--run", action="store_true")
    ap.add_argument("--no-build", action="store_true")
    args = ap.parse_args()
    if not args.no_build:
        build(args.out_dir)
    print(mix_table(args.out_dir))
    if args.run:
        print()
        sys.stdout.flush()
        return subprocess.run([os.path.join(args.out_dir, "mont_forms")]).returncode
    return 0


if __name__ == "__main__":
    sys.exit(main())
