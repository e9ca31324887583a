"""CPU: the lockstep (product-scanning) Montgomery products of csrc/ff29.h -- fe_mul_x2, fe_mul_x3, fe_sqr_x2, fe_mul_mul2 -- and the
single fe_mul, fe_mul2, fe_sqr against a verbatim copy of the three operand-scanning routines, bit for bit, for Fq and Fr: 10^5 random operand quadruples and the
edge operands (0, 1, p - 1, every limb at MASK29, the top limb at each class's bound, lazy limbs up to 2^31 - 1).  The checker is
a stand-alone program (tests/mont_forms_host.cpp) built with AddressSanitizer and UBSan; the -DHM_BOUNDS build declares every
operand at its class maximum, so a column sum that could overflow aborts it."""
import os
import subprocess

import pytest

from halo2_experiments_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("bounds", [False, True], ids=["plain", "hm_bounds"])
def test_new_forms_match_operand_scanning(tmp_path, bounds):
    exe = str(tmp_path / "mont_forms_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
           "-I", _lib.CSRC, os.path.join(HERE, "mont_forms_host.cpp"), "-o", exe]
    if bounds:
        cmd.insert(1, "-DHM_BOUNDS")
    subprocess.run(cmd, check=True)
    r = subprocess.run([exe, "100000"], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "all bit-identical" in r.stdout
