"""The reference-side binding as files (rust/): the edit table, the script that applies it and the unified diff are
exercised here on a SKELETON of the upstream crate -- the anchor lines as recalled from halo2_proofs at tag v2023_02_02
(/root/reference/Cargo.toml:10 pins it; its text is not available in this image), with filler between them.  What this
proves: the table, the script and the patch agree with each other, the script is idempotent and refuses a file whose
anchors differ.  What it cannot prove: that the recalled lines are upstream's."""
import json
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUST = os.path.join(ROOT, "rust")


def _skeleton(tmp_path):
    """halo2_proofs/ with every file of the edit table: filler lines, each anchor as often as the table expects, in an
    order that resembles the upstream file."""
    table = json.load(open(os.path.join(RUST, "edits.json")))
    root = tmp_path / "halo2_proofs"
    by_file = {}
    for e in table:
        by_file.setdefault(e["file"], []).append(e)
    for rel, entries in by_file.items():
        path = root / rel
        path.parent.mkdir(parents=True, exist_ok=True)
        spots = sorted((e["near_line"] + 60 * k, e["anchor"]) for e in entries for k in range(len(e["replacements"])))
        lines, nxt = [], 1
        for at, anchor in spots:
            while nxt < at:
                lines.append(f"// filler {nxt}")
                nxt += 1
            lines.append(anchor)
            nxt += 1
        lines += [f"// filler {nxt + i}" for i in range(5)]
        path.write_text("\n".join(lines) + "\n")
    (root / "src").mkdir(exist_ok=True)
    return root, table


def _run(root, *flags):
    return subprocess.run([sys.executable, os.path.join(RUST, "apply_edits.py"), *flags, str(root)], capture_output=True, text=True)


def test_apply_edits_makes_every_edit_once(tmp_path):
    root, table = _skeleton(tmp_path)
    dry = _run(root, "--dry-run")
    assert dry.returncode == 0 and "would edit src/arithmetic.rs" in dry.stdout
    assert "mi355x" not in (root / "src" / "arithmetic.rs").read_text()
    r = _run(root)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (root / "src" / "mi355x.rs").exists() and (root / "src" / "mi355x_kzg.rs").exists()
    arith = (root / "src" / "arithmetic.rs").read_text()
    assert arith.count("fn original_best_multiexp<C: CurveAffine>") == 1 and arith.count("fn original_best_fft<G: Group>") == 1
    assert arith.count("pub mod mi355x;") == 1 and arith.count("pub mod mi355x_kzg;") == 1 and arith.count("pub mod mi355x_dev;") == 1
    assert (root / "src" / "mi355x_dev.rs").exists()
    kzg = (root / "src" / "poly" / "kzg" / "commitment.rs").read_text()
    assert kzg.count("gpu: Default::default(),") == 3 and kzg.count("pub(crate) gpu: crate::arithmetic::mi355x_kzg::SrsHandles,") == 1
    assert kzg.count("self.gpu.reset();") == 1
    # commit_lagrange is the first of the two functions in the file, commit the second
    assert 0 < kzg.index("self.gpu.commit_lagrange::<E::G1Affine>") < kzg.index("self.gpu.commit::<E::G1Affine>")
    assert "halo2-mi355x-sys" in (root / "Cargo.toml").read_text()
    # the optional batch-commit method: provided by the trait, overridden for ParamsKZG
    assert (root / "src" / "poly" / "commitment.rs").read_text().count("fn commit_lagrange_batch(") == 1
    assert kzg.count("self.gpu.commit_lagrange_batch::<E::G1Affine>") == 1
    # the optional EvaluationDomain edits: each step tries the GPU first, the upstream statements stay behind it
    dom = (root / "src" / "poly" / "domain.rs").read_text()
    assert dom.count("mi355x::try_coeff_to_extended(") == 1 and dom.count("mi355x::try_extended_to_coeff(") == 1
    assert dom.index("try_coeff_to_extended") < dom.index("        self.distribute_powers_zeta(&mut a.values, true);")
    assert dom.index("        assert_eq!(a.values.len(), self.extended_len());") < dom.index("try_extended_to_coeff")
    again = _run(root)                                          # idempotent
    assert again.returncode == 0 and "already edited" in again.stdout
    assert (root / "src" / "poly" / "kzg" / "commitment.rs").read_text() == kzg


def test_apply_edits_refuses_a_file_whose_anchors_differ(tmp_path):
    root, _ = _skeleton(tmp_path)
    path = root / "src" / "poly" / "kzg" / "commitment.rs"
    text = path.read_text().replace("            s_g2,", "            s_g2: s_g2,", 1)      # one struct literal spelled differently
    path.write_text(text)
    r = _run(root)
    assert r.returncode == 1 and "NOT APPLIED src/poly/kzg/commitment.rs" in r.stdout and "expected 3 occurrence(s), found 2" in r.stdout
    assert path.read_text() == text                              # nothing of that file was written
    assert "mi355x" in (root / "src" / "arithmetic.rs").read_text()   # the other files were


def test_a_missing_optional_anchor_is_skipped_not_fatal(tmp_path):
    root, _ = _skeleton(tmp_path)
    trait = root / "src" / "poly" / "commitment.rs"
    trait.write_text(trait.read_text().replace("    /// Writes params to a buffer.", "    /// Writes the parameters."))
    r = _run(root)
    assert r.returncode == 0 and "SKIPPED (optional)" in r.stdout
    assert "commit_lagrange_batch" not in trait.read_text()
    assert "self.gpu.commit_lagrange::<E::G1Affine>" in (root / "src" / "poly" / "kzg" / "commitment.rs").read_text()
    trait.unlink()
    assert _run(root).returncode == 0                            # a file with optional edits only may be absent


@pytest.mark.skipif(shutil.which("patch") is None, reason="no patch(1)")
def test_the_unified_diff_makes_the_same_edits(tmp_path):
    a, _ = _skeleton(tmp_path / "a")
    b, _ = _skeleton(tmp_path / "b")
    assert _run(a).returncode == 0
    r = subprocess.run(["patch", "-p1", "-i", os.path.join(RUST, "halo2_proofs.patch")], cwd=b, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    for rel in ("src/arithmetic.rs", "src/poly/kzg/commitment.rs", "src/poly/commitment.rs", "src/poly/domain.rs", "Cargo.toml", "src/mi355x.rs",
                "src/mi355x_kzg.rs", "src/mi355x_dev.rs"):
        assert (a / rel).read_text() == (b / rel).read_text(), rel


def test_the_device_resident_glue_binds_what_the_header_declares():
    """mi355x_dev.rs (DevicePoly, DeviceDomain, commit_dev, QuotientProgram): every sys:: item it calls is declared by the generated
    lib.rs with the arity it is called with (the header <-> lib.rs check is tests/test_capi.py); RAII on both handle types; nothing
    panics."""
    import re
    dev = open(os.path.join(RUST, "halo2_proofs-patch", "src", "mi355x_dev.rs")).read()
    lib = open(os.path.join(RUST, "halo2-mi355x-sys", "src", "lib.rs")).read()
    declared = {m.group(1): len([a for a in m.group(2).split(",") if a.strip()])
                for m in re.finditer(r"pub\s+fn\s+(hm_[a-z0-9_]+)\s*\(([^)]*)\)", lib, flags=re.S)}
    calls = re.findall(r"sys::(hm_[a-z0-9_]+)\s*\(", dev)
    assert set(calls) >= {"hm_device_malloc", "hm_device_free", "hm_copy_to_device", "hm_copy_to_host", "hm_device_synchronize",
                          "hm_ntt_batch_bn256_fr_dev", "hm_coeff_to_extended_bn256_fr_dev", "hm_extended_to_coeff_bn256_fr_dev",
                          "hm_msm_bn256_g1_dev", "hm_msm_batch_bn256_g1_dev", "hm_eval_polynomial_bn256_fr_dev", "hm_graph_create",
                          "hm_quotient_by_cosets_bn256_fr_dev", "hm_graph_destroy"}
    for m in re.finditer(r"sys::(hm_[a-z0-9_]+)\s*\(", dev):
        name, i, depth, args, cur = m.group(1), m.end(), 1, 0, ""
        while depth:                                          # count top-level commas of the call's argument list
            ch = dev[i]
            if ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                args += 1 if cur.strip() else 0
                cur = ""
                i += 1
                continue
            if depth:
                cur += ch
            i += 1
        args += 1 if cur.strip() else 0
        assert name in declared and declared[name] == args, (name, declared.get(name), args)
    assert dev.count("impl Drop for") == 2 and "panic!" not in dev and "unwrap()" not in dev


def test_glue_is_free_of_the_risks_the_review_named():
    glue = open(os.path.join(RUST, "halo2_proofs-patch", "src", "mi355x.rs")).read()
    kzg = open(os.path.join(RUST, "halo2_proofs-patch", "src", "mi355x_kzg.rs")).read()
    assert "OnceLock" not in glue + kzg and "std::sync::Once" in glue            # no dependence on Rust >= 1.70
    assert "use group::prime::PrimeCurveAffine;" in glue and "use group::Group as _;" in glue
    assert "HM_ERR_PARTIAL_OUTPUT" in glue and "panic!" in glue                  # never run the CPU body on a half-written array
    assert "hm_register_bases(" in kzg and "hm_msm_batch_bn256_g1_h(" in kzg and "hm_release_bases(" in kzg
    # the EvaluationDomain steps: coeff_to_extended writes a fresh Vec (no failure can touch the input), extended_to_coeff is in place
    # and therefore panics on a half-written array instead of letting the CPU body continue on it
    assert "Vec::with_capacity(len)" in glue and "*a = ext;" in glue and glue.count("HM_ERR_PARTIAL_OUTPUT") >= 3
    assert "hm_coeff_to_extended_bn256_fr(" in glue and "hm_extended_to_coeff_bn256_fr(" in glue and "a.truncate(keep);" in glue


def test_the_device_glue_cannot_cost_the_drop_in_its_build():
    """mi355x_dev.rs (264 lines that have never met rustc) was compiled for every user of the drop-in patch.  Now behind a
    cargo feature; every glue module carries its own lint allowance (the crate denies missing_docs / missing_debug_implementations
    / unsafe_code as recalled); none depends on the ff version's `one()`."""
    table = json.load(open(os.path.join(RUST, "edits.json")))
    arith = next(e for e in table if e["file"] == "src/arithmetic.rs" and "best_multiexp" in e["anchor"])
    lines = arith["replacements"][0]
    i = lines.index("pub mod mi355x_dev;")
    assert lines[i - 2] == '#[cfg(feature = "mi355x-dev")]' and lines[i - 1] == '#[path = "mi355x_dev.rs"]'
    assert lines[lines.index("pub mod mi355x;") - 1] == '#[path = "mi355x.rs"]' and "cfg" not in lines[lines.index("pub mod mi355x;") - 2]
    feat = [e for e in table if e["file"] == "Cargo.toml" and e["anchor"] == "[features]"]
    assert len(feat) == 1 and feat[0]["optional"] is True and feat[0]["replacements"][0] == ["[features]", "mi355x-dev = []"]
    for name in ("mi355x.rs", "mi355x_kzg.rs", "mi355x_dev.rs"):
        text = open(os.path.join(RUST, "halo2_proofs-patch", "src", name)).read()
        assert "#![allow(unsafe_code, missing_docs, missing_debug_implementations" in text, name
        head = text[: text.index("#![allow(")]
        assert all(ln.startswith("//") or not ln.strip() for ln in head.splitlines()), name       # inner attributes come before any item
        assert "Fr::one()" not in text.replace("bn256::Fr::one()", "") and "Fr::ONE" not in text, name
    dev = open(os.path.join(RUST, "halo2_proofs-patch", "src", "mi355x_dev.rs")).read()
    for struct in ("DevicePoly", "DeviceDomain", "QuotientProgram"):
        at = dev.index(f"pub struct {struct} ")
        assert dev[:at].rstrip().endswith("#[derive(Debug)]"), struct
