#!/usr/bin/env python3
"""Generate the parts of the Rust side of the drop-in boundary that are derived from other files, so that they cannot drift.

    python tools/gen_rust_shim.py            # (re)write the generated files below
    python tools/gen_rust_shim.py --check    # exit 1 if any generated file differs from what is committed

What the reference patches: /root/reference/Cargo.toml:10 pins halo2_proofs (git tag v2023_02_02); the two free functions
of its arithmetic.rs are the boundary.

Writes:
    rust/halo2-mi355x-sys/src/lib.rs       from include/halo2_mi355x.h: one `extern "C"` item per header entry, #[repr(C)]
                                           twins of the stats structs, the HM_* constants
    INTEGRATION.md (extern block)          the same extern block and structs, between the GENERATED markers
    rust/halo2_proofs.patch                unified diff for the halo2_proofs checkout: the three glue modules as new files,
                                           zero-context hunks from the edit table
Only reads (maintained by hand):
    include/halo2_mi355x.h                 the C ABI, parsed by halo2-experiments_amd/_header.py (the ctypes binding uses the same parse)
    rust/halo2_proofs-patch/src/{mi355x,mi355x_kzg,mi355x_dev}.rs   the glue modules; every sys:: item they use must be
                                           declared by the header (checked here and by tests/test_capi.py)
    rust/edits.json                        the edits of existing upstream files (also read by rust/apply_edits.py)

There is no Rust toolchain in the build image: none of this has been compiled here.  tests/test_capi.py parses the header
(C) and the generated extern block (Rust) with two independent parsers and compares names, arity and every argument type.
"""
from __future__ import annotations

import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "halo2_mi355x.h")
RUST_DIR = os.path.join(ROOT, "rust")
GLUE_DIR = os.path.join(RUST_DIR, "halo2_proofs-patch", "src")
GLUE_MODULES = ("mi355x.rs", "mi355x_kzg.rs", "mi355x_dev.rs")
INTEGRATION = os.path.join(ROOT, "INTEGRATION.md")
BEGIN_MARK = "<!-- BEGIN GENERATED: extern block (tools/gen_rust_shim.py) -->"
END_MARK = "<!-- END GENERATED -->"

# ---- C side: the header parser is the package's own (the ctypes binding is derived from the same parse) -------------------
def _load_header_parser():
    import importlib.util
    spec = importlib.util.spec_from_file_location("hm_header", os.path.join(ROOT, "halo2-experiments_amd", "_header.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)                # by path: standard library only, the package (ctypes, numpy) is not imported
    return mod


_header = _load_header_parser()
C_SCALARS, STRUCTS = _header.C_SCALARS, _header.STRUCTS
strip_comments, parse_c_type, parse_header = _header.strip_comments, _header.parse_c_type, _header.parse_header


def rust_type(canon: str) -> str:
    parts = canon.split()
    out = parts[0]
    for p in parts[1:]:
        out = ("*const " if p == "c" else "*mut ") + out
    return out


# ---- Rust side (an independent parser: used by the tests on the generated text and on INTEGRATION.md) ---------------------
def parse_rust_type(t: str) -> str:
    t = t.strip()
    ptrs = []
    while t.startswith("*"):
        m = re.match(r"^\*(const|mut)\s+(.*)$", t)
        ptrs.append("c" if m.group(1) == "const" else "m")
        t = m.group(2).strip()
    return " ".join([t] + ptrs[::-1])


def parse_rust_extern(text: str):
    """The `extern "C" { ... }` block(s) of a Rust source -> [(name, ret canonical, [(canonical, name)])]"""
    out = []
    for blk in re.finditer(r'extern\s+"C"\s*\{(.*?)\n\}', text, flags=re.S):
        body = re.sub(r"//[^\n]*", "", blk.group(1))
        for m in re.finditer(r"pub\s+fn\s+(hm_[a-z0-9_]+)\s*\(([^)]*)\)\s*(?:->\s*([^;]+))?;", body, flags=re.S):
            params = []
            for p in m.group(2).split(","):
                p = p.strip()
                if not p:
                    continue
                name, ty = p.split(":", 1)
                params.append((parse_rust_type(ty), name.strip()))
            out.append((m.group(1), parse_rust_type(m.group(3)) if m.group(3) else "()", params))
    return out


# ---- emitters -------------------------------------------------------------------------------------------------------
def emit_extern_block(functions) -> str:
    lines = ['extern "C" {']
    for name, ret, params in functions:
        args = ", ".join(f"{pn or 'arg' + str(i)}: {rust_type(pt)}" for i, (pt, pn) in enumerate(params))
        line = f"    pub fn {name}({args}) -> {rust_type(ret)};"
        if len(line) > 150:                     # wrap long prototypes once, at a comma near the middle
            cut = line.rfind(", ", 0, 140)
            line = line[:cut + 1] + "\n        " + line[cut + 2:]
        lines.append(line)
    lines.append("}")
    return "\n".join(lines)


def emit_structs(structs) -> str:
    out = []
    for cname, fields in structs.items():
        out.append("#[repr(C)]\n#[derive(Clone, Copy, Debug)]\npub struct %s {" % STRUCTS[cname])
        for fname, base, count in fields:
            out.append(f"    pub {fname}: " + (f"[{base}; {count}]," if count else f"{base},"))
        out.append("}\n")
    return "\n".join(out)


def emit_lib_rs(functions, structs, defines) -> str:
    consts = "\n".join(f"pub const {n}: c_int = {v};" for n, v in defines if "(" not in v)     # the int ones; HM_NO_CHAIN is a size_t
    return f'''//! halo2-mi355x-sys -- raw bindings of libhalo2_mi355x.so (include/halo2_mi355x.h), the MI355X backend of
//! halo2_proofs::arithmetic::{{best_multiexp, best_fft}} for bn256.
//!
//! GENERATED by tools/gen_rust_shim.py from the header: do not edit; re-run the script when the header changes
//! (tests/test_capi.py fails when this file and the header disagree on a name, an arity or an argument type).
//! Not compiled in the repository's build image (no Rust toolchain there).
#![allow(non_camel_case_types)]

use std::ffi::CStr;
use std::os::raw::{{c_char, c_int, c_long, c_void}};

{consts}

{emit_structs(structs)}
{emit_extern_block(functions)}

/// The calling thread's last error message (hm_last_error), as an owned String.
pub fn last_error() -> String {{
    unsafe {{ CStr::from_ptr(hm_last_error()) }}.to_string_lossy().into_owned()
}}

#[allow(dead_code)]
fn _unused(_: c_long, _: *const c_char, _: *mut c_void) {{}}
'''


def _read(path: str) -> str:
    with open(path) as f:
        return f.read()


def emit_patch() -> str:
    """The glue modules as new files, then the edits of rust/edits.json as zero-context hunks, one per occurrence, in table
    order within each file."""
    def new_file(path, text):
        lines = text.rstrip("\n").split("\n")
        return (f"diff --git a/{path} b/{path}\nnew file mode 100644\n--- /dev/null\n+++ b/{path}\n@@ -0,0 +1,{len(lines)} @@\n"
                + "\n".join("+" + l for l in lines) + "\n")
    out = """# GENERATED by tools/gen_rust_shim.py -- patch for a checkout of privacy-scaling-explorations/halo2 at tag v2023_02_02
# (the revision /root/reference/Cargo.toml:10 pins), applied from the checkout's halo2_proofs/ directory:
#     patch -p1 < <this repository>/rust/halo2_proofs.patch
# The upstream sources are not available in the build image, so the edits of existing files are ZERO-CONTEXT hunks that depend
# on one line each, written from memory of the tag; `patch` finds them by content (line numbers are approximate: expect
# "offset" messages).  An anchor line that occurs several times (the struct literals of ParamsKZG, the last line of its two
# commit functions) has one hunk per occurrence, in file order.  rust/apply_edits.py makes the SAME edits from the same
# table, is idempotent and refuses a file whose anchors do not occur as often as expected: prefer it.
"""
    for name in GLUE_MODULES:
        out += new_file(f"src/{name}", _read(os.path.join(GLUE_DIR, name)))
    by_file = {}
    for e in json.loads(_read(os.path.join(RUST_DIR, "edits.json"))):
        for k, repl in enumerate(e["replacements"]):
            by_file.setdefault(e["file"], []).append((e["near_line"] + 60 * k, e["anchor"], repl))
    for path, hunks in by_file.items():
        out += f"diff --git a/{path} b/{path}\n--- a/{path}\n+++ b/{path}\n"
        shift = 0
        for at, anchor, repl in sorted(hunks, key=lambda h: h[0]):
            new_range = f"+{at + shift},{len(repl)}" if repl else f"+{at + shift - 1},0"
            out += f"@@ -{at} {new_range} @@\n-{anchor}\n" + "".join("+" + l + "\n" for l in repl)
            shift += len(repl) - 1
    return out


def check_glue_against_header(functions, defines):
    """Every sys:: item the glue modules use must be something lib.rs declares (an entry point, a constant, last_error)."""
    declared = {f[0] for f in functions} | {d[0] for d in defines} | {"last_error"}
    for name in GLUE_MODULES:
        for item in sorted(set(re.findall(r"sys::(\w+)", _read(os.path.join(GLUE_DIR, name))))):
            if item not in declared:
                raise SystemExit(f"gen_rust_shim: {name} uses sys::{item}, which include/halo2_mi355x.h does not declare")


def generate():
    """-> {path: text} of every generated file."""
    functions, structs, defines = parse_header(_read(HEADER))
    check_glue_against_header(functions, defines)
    files = {
        os.path.join(RUST_DIR, "halo2-mi355x-sys", "src", "lib.rs"): emit_lib_rs(functions, structs, defines),
        os.path.join(RUST_DIR, "halo2_proofs.patch"): emit_patch(),
    }
    doc = _read(INTEGRATION)
    if BEGIN_MARK in doc and END_MARK in doc:
        a, b = doc.index(BEGIN_MARK) + len(BEGIN_MARK), doc.index(END_MARK)
        block = "\n```rust\nuse std::os::raw::{c_char, c_int, c_long, c_void};\n\n" + emit_extern_block(functions) + "\n\n" + \
                emit_structs(structs).rstrip("\n") + "\n```\n"
        files[INTEGRATION] = doc[:a] + block + doc[b:]
    return files


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    stale = []
    for path, text in generate().items():
        old = _read(path) if os.path.exists(path) else None
        if old == text:
            continue
        if args.check:
            stale.append(os.path.relpath(path, ROOT))
        else:
            os.makedirs(os.path.dirname(path), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)
            print("wrote", os.path.relpath(path, ROOT))
    if stale:
        print("stale generated files (run tools/gen_rust_shim.py):", ", ".join(stale))
        sys.exit(1)


if __name__ == "__main__":
    main()
