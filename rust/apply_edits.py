#!/usr/bin/env python3
"""Apply the halo2_proofs edits of this directory to a checkout of privacy-scaling-explorations/halo2 at tag v2023_02_02
(what /root/reference/Cargo.toml:10 pins) -- the same edits as halo2_proofs.patch, from the same table (edits.json, the
table's source, maintained by hand; tools/gen_rust_shim.py builds the patch from it), but found as literal LINES instead of
line numbers:

    python3 apply_edits.py <halo2 checkout>/halo2_proofs          # edit in place
    python3 apply_edits.py --dry-run <...>/halo2_proofs           # say what would change

* copies halo2_proofs-patch/src/*.rs into <halo2_proofs>/src/;
* for every entry of edits.json: the anchor line must occur in its file exactly as many times as the entry has
  replacements (1st occurrence -> 1st replacement, ...); otherwise NOTHING of that file is written and the entry is
  reported -- the upstream text was written from memory of the tag (no network in the image these files were made in), so
  a mismatch means "make this edit by hand", never "guess";
* entries marked "optional" (the batch-commit method of the Params trait) are SKIPPED with a message when their anchor is
  not found as expected, and the rest of the file is still edited;
* idempotent: a file that already carries the marker of an edit (its first added line) is left alone.

Nothing here has been run against the real upstream sources; tests/test_rust_edits.py runs it on a skeleton with the
recalled anchor lines."""
import json
import os
import shutil
import sys


def apply_to_text(text, entries):
    """-> (new text, problems).  `entries`: the edits.json entries of ONE file, in table order."""
    lines = text.split("\n")
    problems = []
    for e in entries:
        anchor, repls = e["anchor"], e["replacements"]
        added = [l for r in repls for l in r if l != anchor]
        marker = next((l for l in added if "mi355x" in l or "gpu" in l), added[0] if added else None)
        if marker is not None and any(l == marker for l in lines):
            continue                                  # this edit has been made already
        hits = [i for i, l in enumerate(lines) if l == anchor]
        if len(hits) != len(repls):
            if e.get("optional"):
                print(f"SKIPPED (optional) anchor {anchor!r}: expected {len(repls)} occurrence(s), found {len(hits)}")
                continue
            problems.append(f"anchor {anchor!r}: expected {len(repls)} occurrence(s), found {len(hits)}")
            continue
        for i, r in reversed(list(zip(hits, repls))):
            lines[i:i + 1] = r
    return "\n".join(lines), problems


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    dry = "--dry-run" in sys.argv
    if len(args) != 1:
        raise SystemExit(__doc__)
    root = args[0]
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "edits.json")) as f:
        table = json.load(f)
    if not os.path.isdir(os.path.join(root, "src")):
        raise SystemExit(f"{root} does not look like halo2_proofs/ (no src/)")
    for name in sorted(os.listdir(os.path.join(here, "halo2_proofs-patch", "src"))):
        dst = os.path.join(root, "src", name)
        print(("would copy " if dry else "copy ") + name + " -> " + dst)
        if not dry:
            shutil.copyfile(os.path.join(here, "halo2_proofs-patch", "src", name), dst)
    failed = False
    by_file = {}
    for e in table:
        by_file.setdefault(e["file"], []).append(e)
    for rel, entries in by_file.items():
        path = os.path.join(root, rel)
        if not os.path.exists(path):
            if all(e.get("optional") for e in entries):
                print(f"SKIPPED (optional) {rel}: no such file")
                continue
            print(f"MISSING {rel}: make its {len(entries)} edit(s) by hand (README.md)")
            failed = True
            continue
        with open(path) as f:
            old = f.read()
        new, problems = apply_to_text(old, entries)
        for p in problems:
            print(f"NOT APPLIED {rel}: {p}")
        if problems:
            failed = True
            continue
        if new == old:
            print(f"unchanged {rel} (already edited)")
        else:
            print(("would edit " if dry else "edit ") + rel)
            if not dry:
                with open(path, "w") as f:
                    f.write(new)
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
