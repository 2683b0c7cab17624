"""The per-thread code of the ordered pack kernel, run on the CPU (no GPU needed).

tests/emu/pack_emu.cpp includes the REAL loona_amd/csrc/hpk_pack.h as it is (pack_upper, pack_segment,
pack_chunk, pack_chunk_range, pack_store) behind tests/emu/shim.h, and replays whole destination tiles the
way hpk_pack.hip drives them: a workgroup's contiguous run of tiles, its window of staged offsets restaged
when it is used up. The layouts put literal boundaries on the tile edges, a literal over several tiles,
more empty and one-byte literals than the window holds, exact totals around the tile size, empty batches,
misaligned source and destination bases and capacity cuts; the result is compared with memcpy and every
byte outside the written range with a canary. What it cannot cover (LDS, barriers, the length scan) is
tests/test_packed.py's job on the GPU.
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
    d = tmp_path_factory.mktemp("pack_emu")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-I", os.path.join(REPO, "loona_amd", "csrc"), "-I",
                           os.path.join(HERE, "emu"), os.path.join(HERE, "emu", "pack_emu.cpp"), "-o", str(d / "pack_emu")])
    return str(d / "pack_emu")


@pytest.mark.parametrize("seed", [1, 2])
def test_pack_emulation_matches_memcpy(emu, seed):
    p = subprocess.run([emu, str(seed), "2"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "ok: 0 mismatches" in p.stdout


def test_pack_emulation_under_host_sanitizers(tmp_path_factory):
    """The same program with ASan and UBSan, stand-alone (another seed)."""
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    exe = san_util.build_emu(tmp_path_factory.mktemp("pack_emu_san"), "pack_emu_san", san_util.ASAN, source="pack_emu", oracle=False)
    p = subprocess.run([exe, "3", "2"], capture_output=True, text=True, timeout=300)
    san_util.assert_clean(p)
