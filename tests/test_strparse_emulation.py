"""The per-thread code of the string-literal decode's parse step, run on the CPU (no GPU needed).

tests/emu/strparse_emu.cpp includes the REAL loona_amd/csrc/hpk_strparse.h as it is (str_parse) behind
tests/emu/shim.h and runs it on every window of decode_strings_cases.prefix_shapes(): the values 0, 126, 127,
128, 254, 255, 127 + 2^7, 127 + 2^14, 127 + 2^21 and the largest 5-octet value under both H values, each cut at
every window length from 0 up to its integer's length, with length == window, length == window + 1 and trailing
bytes, a 5th octet with the continuation bit, and padded non-canonical integers. The answers are
hpack_ref.decode_integer's and decode_string's on the same window. The program also checks that no byte outside
the window's intersection with the blob is read: through a checking accessor, and with the blob at the end of a
buffer whose next page has no access, at all 4 dword alignments, with and without poison bytes after the window.
The program is also built with -fsanitize=address,undefined and run stand-alone on the same case file."""

import os
import shutil
import struct
import subprocess

import pytest

import decode_strings_cases as dc
import san_util
from hpk_util import hpack_ref

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("strparse_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "strparse_emu.cpp"), "-o", str(d / "strparse_emu")])
    return str(d / "strparse_emu"), d


def reference(window):
    """(status, H, payload start, payload length, consumed) of one window by hpack_ref alone"""
    try:
        ln, used = hpack_ref.decode_integer(window, 7)
    except hpack_ref.DecoderError as e:
        return ({"TooManyOctets": dc.TOO_MANY, "NotEnoughOctets": dc.INT_SHORT}[e.detail], 0, 0, 0, 0)
    try:
        _, consumed = hpack_ref.decode_string(window)
    except hpack_ref.DecoderError as e:
        if e.detail == "NotEnoughOctets":
            return (dc.STR_SHORT, 0, 0, 0, 0)
        consumed = used + ln  # (a Huffman error: the prefix and the length check passed)
    assert consumed == used + ln
    return (dc.OK, window[0] >> 7, used, ln, consumed)


@pytest.fixture(scope="module")
def cases(emu):
    """the case file both builds of the program read, and its windows"""
    shapes = dc.prefix_shapes()
    assert len(shapes) > 150
    path = emu[1] / "cases.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(shapes)))
        for _, w in shapes:
            f.write(struct.pack("<I", len(w)) + w)
    return str(path), shapes


def check(p, shapes):
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    lines = [ln for ln in p.stdout.splitlines() if ln and ln[0].isdigit()]
    assert len(lines) == len(shapes) and f"ok: 0 failures in {len(shapes)} cases" in p.stdout
    seen = set()
    for (what, w), ln in zip(shapes, lines):
        got = tuple(int(x) for x in ln.split())
        want = reference(w)
        assert got == want, f"{what} ({w[:8].hex()}..., {len(w)} bytes): {got} for {want}"
        seen.add(want[0])
    assert seen == {dc.OK, dc.TOO_MANY, dc.INT_SHORT, dc.STR_SHORT}


def test_strparse_matches_hpack_ref(emu, cases):
    check(subprocess.run([emu[0], cases[0]], capture_output=True, text=True, timeout=120), cases[1])


def test_strparse_under_host_sanitizers(emu, cases):
    """The same program with ASan and UBSan, stand-alone, on the same case file and with the same checks."""
    exe = san_util.build_emu(emu[1], "strparse_emu_san", san_util.ASAN, source="strparse_emu", oracle=False)
    p = subprocess.run([exe, cases[0]], capture_output=True, text=True, timeout=300)
    check(p, cases[1])
    san_util.assert_no_reports(p)
