"""Parser of include/halo2_mi355x.h, the one statement of the C ABI.  The ctypes binding (_lib.py) and the Rust `extern` block
(tools/gen_rust_shim.py) are both derived from what it returns.  Standard library only.

A type is written in canonical form: the base type followed by one 'c' (pointer to const) or 'm' (pointer to mutable) per
pointer level, outermost last: 'u64 c' = const uint64_t*, 'c_void c c' = const void* const*.
"""
from __future__ import annotations

import re

C_SCALARS = {"int": "c_int", "long": "c_long", "size_t": "usize", "uint64_t": "u64", "uint32_t": "u32", "int32_t": "i32",
             "uint8_t": "u8", "double": "f64", "char": "c_char", "void": "c_void"}
STRUCTS = {"hm_msm_stats": "HmMsmStats", "hm_stats": "HmStats", "hm_bases_info": "HmBasesInfo"}


def strip_comments(text: str) -> str:
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def parse_c_type(decl: str):
    """'const uint64_t* const* name[12]' -> (canonical type, name)."""
    decl = decl.strip()
    m = re.match(r"^(.*?)(\w+)\s*(\[\s*\w*\s*\])?$", decl, flags=re.S)
    if not m:
        raise ValueError(f"cannot parse parameter {decl!r}")
    ty, name, arr = m.group(1).strip(), m.group(2), m.group(3)
    if ty == "" or ty == "const":              # unnamed parameter such as 'void'
        ty, name = decl, ""
    toks = re.findall(r"\w+|\*", ty)
    base = [t for t in toks if t not in ("const", "*", "struct")]
    if len(base) != 1:
        raise ValueError(f"cannot parse type {ty!r}")
    b = base[0]
    rust_base = C_SCALARS.get(b) or STRUCTS.get(b)
    if rust_base is None:
        raise ValueError(f"unknown C type {b!r}")
    # constness of each level: a 'const' binds to what is on its left, or to the base type when it comes first
    levels = []                                # constness of [base, after 1st *, after 2nd * ...]
    cur_const = False
    seen_base = False
    for t in toks:
        if t == "const":
            cur_const = True
        elif t == "*":
            levels.append(cur_const)
            cur_const = False
        elif t != "struct":
            seen_base = True
    levels.append(cur_const)                   # constness of the outermost object (the parameter itself): irrelevant
    ptrs = [("c" if levels[i] else "m") for i in range(len(levels) - 1)]
    if arr:                                    # T name[N] decays to T*: pointee constness = constness of the element level
        ptrs.append("c" if levels[-1] else "m")
    assert seen_base
    return " ".join([rust_base] + ptrs), name


def parse_header(text: str):
    """-> (functions [(name, ret canonical, [(canonical type, name)])], structs {c name: [(field, canonical, count)]},
    defines [(name, value text)]: a decimal integer, behind its cast where the header writes one -- '((size_t)-1)' -> '(size_t)-1')"""
    clean = strip_comments(text)
    defines = [(m.group(1), m.group(2)) for m in re.finditer(r"#define\s+(HM_[A-Z0-9_]+)\s+\(?((?:\(\w+\))?-?\d+)\)?", clean)]
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;", clean, flags=re.S):
        fields = []
        for stmt in m.group(2).split(";"):
            stmt = stmt.strip()
            if not stmt:
                continue
            ty = re.match(r"^(\w+)\s+(.*)$", stmt, flags=re.S)
            base = C_SCALARS[ty.group(1)]
            for item in ty.group(2).split(","):
                im = re.match(r"^\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*$", item)
                fields.append((im.group(1), base, int(im.group(2)) if im.group(2) else 0))
        structs[m.group(3)] = fields
    body = re.sub(r"typedef\s+struct\s+\w+\s*\{.*?\}\s*\w+\s*;", " ", clean, flags=re.S)
    body = re.sub(r"#.*", " ", body)
    functions = []
    for m in re.finditer(r"([\w\s\*]+?)\b(hm_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", body, flags=re.S):
        ret = " ".join(m.group(1).replace("extern", " ").replace('"C"', " ").split())
        ret_c, _ = parse_c_type(ret + " _r")
        params = []
        plist = m.group(3).strip()
        if plist and plist != "void":
            for p in plist.split(","):
                params.append(parse_c_type(p))
        functions.append((m.group(2), ret_c, params))
    return functions, structs, defines
