"""The per-thread code of the two-source ordered pack, run on the CPU (no GPU needed).

tests/emu/pack2_emu.cpp includes the REAL loona_amd/csrc/hpk_pack.h as it is behind tests/emu/shim.h and replays
whole destination tiles the way hpk_pack2 (hpk_decode_strings.hip) drives pack2_chunk: a workgroup's contiguous
run of tiles, its window of staged offsets and selectors restaged when it is used up. Per literal a random (or
alternating, or constant) choice between two source blobs; both sources at every misalignment 0..15; runs of
empty literals longer than the window (kPackLds); literals longer than a tile (kPackTile); 1-7-byte literals so
that nearly every 16-byte chunk mixes both sources (the program counts them); capacity cuts; a poisoned byte
just outside each source's range. The result is compared with memcpy and every byte outside the written range
with a canary. What it cannot cover (LDS, barriers, the scans) is tests/test_gpu_decode_strings.py's job.
The program is also built with -fsanitize=address,undefined and run stand-alone."""

import os
import shutil
import subprocess

import pytest

import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not shutil.which("g++"):
        pytest.skip("no host C++ compiler")
    d = tmp_path_factory.mktemp("pack2_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "pack2_emu.cpp"), "-o", str(d / "pack2_emu")])
    return str(d / "pack2_emu")


@pytest.mark.parametrize("seed", [1, 2])
def test_pack2_emulation_matches_memcpy(emu, seed):
    p = subprocess.run([emu, str(seed), "1"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout[-4000:] + p.stderr
    assert "ok: 0 mismatches" in p.stdout


def test_pack2_emulation_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (another seed)."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("pack2_emu_san"), "pack2_emu_san", san_util.ASAN, source="pack2_emu", oracle=False)
    p = subprocess.run([exe, "3", "1"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p)
