#!/usr/bin/env python3
"""Read the gfx950 ISA of the BUILT objects (csrc/*.o -> .hip_fatbin -> clang-offload-bundler -> llvm-objdump) and report, per kernel:

  * vector memory instructions addressed THROUGH THE KERNARG POINTER (`global_load_ubyte v, v, s[0:1] offset:N`): what a dynamically
    indexed BYTE table inside a by-value kernel argument compiles to (tools/ubench/kernarg_byval.hip).  A stand-alone kernel of that
    shape faulted once on this stack (profiles/r04_kernarg_byval.txt); the load is legal ISA and the cause is NOT established
    (profiles/r05_kernarg_isa.txt), so the production kernels simply must not contain the pattern: their by-value tables
    (NttCosetTables, PoCols / PoPoints, MsmGroupScalars, LkPtrs ...) are 32- / 64-bit entries indexed by wave-uniform values and
    must keep compiling to scalar loads.  tests/test_isa.py runs this on every kernel of the library (CPU only).
  * MFMA instructions (the north star: none -- 256-bit modular integer work), scratch use, VGPR counts.

    python tools/isa_check.py                  # summary of every object
    python tools/isa_check.py ntt.o --dump     # the offending instructions with context
    python tools/isa_check.py --k3 [msm.o ...] # the bucket accumulation kernel: VGPRs, scratch, and the instruction mix of its loops
                                               # (wide mads, 64-bit adds, 64-bit shifts, compiler nops); the first is the hot one
    python tools/isa_check.py --digest         # per kernel: object, SHA-256 of its instructions, mangled name -- what has to stay equal
                                               # when kernels only move between translation units (sort, drop column 1, diff)

The objects are the ones csrc/Makefile names (its print-objs / print-api-objs targets): no list of translation units is kept here.
"""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "halo2-experiments_amd", "csrc")
LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def _makefile_list(target: str):
    return subprocess.run(["make", "-s", "--no-print-directory", "-C", CSRC, target], check=True, capture_output=True, text=True).stdout.split()


OBJECTS = _makefile_list("print-objs")             # every translation unit of the library
API_OBJECTS = _makefile_list("print-api-objs")     # ... of which these are host only

_VMEM = re.compile(r"^\s*(global_|flat_|buffer_|scratch_)(load|store|atomic)\w*\s+(.*)$")
_SLOAD = re.compile(r"^\s*s_load_dword(?:x\d+)?\s+\S+,\s*(s\[\d+:\d+\])")
_SDEST = re.compile(r"^\s*s_\w+\s+(s\d+|s\[\d+:\d+\])")


def device_disassembly(obj_path: str) -> str:
    """The gfx950 code object inside a host object built by hipcc, disassembled."""
    with tempfile.TemporaryDirectory(prefix="hm_isa_") as tmp:
        fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
        r = subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj_path, os.path.join(tmp, "copy.o")],
                           capture_output=True, text=True)
        if r.returncode != 0:
            if "not found" in r.stderr:                     # a host-only translation unit (capi*.hip, digest.hip, multi.hip, xfer.hip): no device code
                return ""
            raise RuntimeError(r.stderr)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", f"--targets={TARGET}", "--unbundle", f"--output={co}"],
                       check=True, capture_output=True)
        return subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout


def kernels(disassembly: str):
    """-> {mangled name: [instruction text, ...]}"""
    out, cur = {}, None
    for line in disassembly.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    return out


def _regs(operand: str):
    m = re.match(r"s\[(\d+):(\d+)\]$", operand)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r"s(\d+)$", operand)
    return {int(m.group(1))} if m else set()


def kernarg_vector_accesses(insts):
    """Vector memory instructions that use the kernarg pointer pair as their scalar base.  The pair = the base of the kernel's first
    s_load (every kernel here loads its arguments first); tracked until a scalar instruction overwrites either register (a linear
    scan: control flow is ignored, which can only end the tracking early at a join -- none of the kernels reuses the pair)."""
    pair = None
    hits = []
    for i, ins in enumerate(insts):
        if pair is None:
            m = _SLOAD.match(ins)
            if m:
                pair = m.group(1)
            continue
        m = _VMEM.match(ins)
        if m and re.search(r"(^|[\s,])" + re.escape(pair) + r"($|[\s,])", m.group(3)):
            hits.append((i, ins))
            continue
        m = _SDEST.match(ins)
        if m and _regs(m.group(1)) & _regs(pair) and not _SLOAD.match(ins):
            break
        if m and _SLOAD.match(ins) and _regs(m.group(1)) & _regs(pair):
            break
    return pair, hits


def summary(obj: str):
    dis = device_disassembly(os.path.join(CSRC, obj))
    rows = {}
    for name, insts in kernels(dis).items():
        if not insts or name.endswith(".kd"):
            continue
        pair, hits = kernarg_vector_accesses(insts)
        rows[name] = {"instructions": len(insts), "kernarg_pair": pair, "kernarg_vector_accesses": hits,
                      "mfma": sum(1 for x in insts if x.startswith("v_mfma") or x.startswith("v_smfma")),
                      "scratch": sum(1 for x in insts if x.startswith("scratch_"))}
    return rows


def digest(insts) -> str:
    """SHA-256 of a kernel's instruction text without the two things that depend on where the kernel lies in its object: the literal
    of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the pc-relative distance to the object's constants) and the s_nop 0
    padding behind the last instruction."""
    body, pcrel = [], 0
    for ins in insts:
        if ins.startswith("s_getpc_b64"):
            pcrel = 2
        elif pcrel and re.match(r"s_addc?_u32\s", ins):
            ins, pcrel = ins.rsplit(",", 1)[0] + ", <pcrel>", pcrel - 1
        else:
            pcrel = 0
        body.append(ins)
    while body and body[-1] in ("s_nop 0", "..."):     # "...": objdump's mark for the zero fill behind an object's last kernel
        body.pop()
    return hashlib.sha256("\n".join(body).encode()).hexdigest()


def _code_object(obj_path: str, tmp: str) -> str:
    fat, co = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.co")
    subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj_path, os.path.join(tmp, "copy.o")], check=True, capture_output=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", f"--input={fat}", f"--targets={TARGET}", "--unbundle", f"--output={co}"],
                   check=True, capture_output=True)
    return co


def k3_report(obj_path: str, kernel: str = "msm_accumulate_kernel"):
    """VGPRs / scratch of the kernel from the code object's metadata, and the instruction mix of every loop that holds curve
    arithmetic (a loop = the address range of a backward branch, whose target is computed from the branch's own address and its
    16-bit offset; nested loops are listed each).  In K3 the first such loop is accumulate_chain's chain of mixed additions
    (g1x_madd_fast: the hot loop), the later ones finish a chain by the general law after an exceptional case."""
    with tempfile.TemporaryDirectory(prefix="hm_isa_") as tmp:
        co = _code_object(obj_path, tmp)
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True, text=True).stdout
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], check=True, capture_output=True, text=True).stdout
    meta = {}
    for entry in notes.split("- .agpr_count:")[1:]:
        if re.search(r"\.name:\s+\S*" + re.escape(kernel), entry):
            for key in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count"):
                m = re.search(r"\." + key + r":\s+(\d+)", entry)
                meta[key] = int(m.group(1)) if m else None
    insts, inside = [], False                              # (address, mnemonic, operands)
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            inside = kernel in m.group(1) and not m.group(1).endswith(".kd")
            continue
        m = re.match(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):", line)
        if inside and m:
            insts.append((int(m.group(3), 16), m.group(1), m.group(2)))
    loops = []                                             # (first address, last address) of every backward branch
    for addr, op, args in insts:
        if op.startswith("s_cbranch") or op == "s_branch":
            off = int(args.split()[-1])
            target = addr + 4 + 4 * (off - 65536 if off >= 32768 else off)
            if target <= addr:
                loops.append((target, addr))
    rows = []
    for lo, hi in sorted(loops):
        body = [op for addr, op, _ in insts if lo <= addr <= hi]
        count = lambda name: sum(1 for x in body if x == name)
        if count("v_mad_u64_u32") >= 100:                  # the loops that hold curve arithmetic
            rows.append(dict(loop=f"{lo:#x}..{hi:#x}", instructions=len(body), valu=sum(1 for x in body if x.startswith("v_")),
                             v_mad_u64_u32=count("v_mad_u64_u32"), v_lshl_add_u64=count("v_lshl_add_u64"),
                             v_lshrrev_b64=count("v_lshrrev_b64"), s_nop=count("s_nop")))
    return dict(meta, instructions=len(insts)), rows


def main():
    if "--k3" in sys.argv:
        objs = [a for a in sys.argv[1:] if not a.startswith("--")] or [os.path.join(CSRC, "msm.o")]
        bad = 0
        for obj in objs:
            r, loops = k3_report(obj if os.path.exists(obj) else os.path.join(CSRC, obj))
            print(obj, " ".join(f"{k}={v}" for k, v in r.items()))
            for row in loops:
                print("   ", " ".join(f"{k}={v}" for k, v in row.items()))
            bad += r["vgpr_count"] > 128 or r["private_segment_fixed_size"] != 0      # four waves per SIMD, no scratch
        sys.exit(1 if bad else 0)
    objs = [a for a in sys.argv[1:] if not a.startswith("--")] or OBJECTS
    if "--digest" in sys.argv:
        for obj in objs:
            for name, insts in kernels(device_disassembly(os.path.join(CSRC, obj))).items():
                if insts and not name.endswith(".kd"):
                    print(f"{obj:14s} {digest(insts)} {name}")
        return
    dump = "--dump" in sys.argv
    bad = 0
    for obj in objs:
        for name, r in summary(obj).items():
            flag = "  <-- vector access through the kernarg pointer" if r["kernarg_vector_accesses"] else ""
            print(f"{obj:14s} {r['instructions']:7d} inst  mfma {r['mfma']}  scratch {r['scratch']:4d}  kernarg {r['kernarg_pair']}  {name[:90]}{flag}")
            if r["kernarg_vector_accesses"]:
                bad += 1
                if dump:
                    for i, ins in r["kernarg_vector_accesses"]:
                        print("      ", i, ins)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
