"""The wave kernel's 13-bit two-symbol table (hpk_code.h, lut13: the LUT3 layout at 13 index bits) checked entry
by entry on the host: tests/lut13_check.cpp decodes every one of the 8,192 prefixes again by brute force from
the 257 code lengths and compares symbols, bits held, codes held, len0 and the not-two flag; an entry with two
codes holds <= 13 bits, and no prefix that starts with a code of <= 13 bits has an empty entry. CPU only (g++)."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "loona_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_lut13_fields_match_a_brute_force_decode(tmp_path):
    exe = tmp_path / "lut13_check"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), os.path.join(HERE, "lut13_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.match(r"ok 8192 entries: (\d+) empty, (\d+) of one code, (\d+) of two \((\d+) holding 13 bits\)", out.stdout)
    assert m, out.stdout
    empty, one, two, thirteen = map(int, m.groups())
    assert empty + one + two == 8192
    # the 13-bit pairs (6+7, 7+6, 5+8, 8+5) that a 12-bit entry cannot hold are there
    assert thirteen > 0
