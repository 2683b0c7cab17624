"""Helpers of the tests that build a program of their own with a host sanitizer and run it stand-alone.

Every sanitized thing in the suite is a program with its own main, started with subprocess: the CPU replays of the
device headers (tests/emu/*.cpp) and the stand-alone driver of the host codec (tests/host/). build_emu compiles a
replay, and the C oracle it links, with one set of flags; assert_clean is what every such run must satisfy."""

import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

ASAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
TSAN = ["-g", "-fsanitize=thread"]
# what no run may print to stderr: UBSan's, ASan's and TSan's reports, and any of the runtimes' warnings
REPORTS = ("runtime error", "AddressSanitizer", "ThreadSanitizer", "WARNING:")


def have_compilers():
    return bool(shutil.which("g++") and shutil.which("gcc"))


def opt(flags):
    return "-O1" if flags else "-O2"


def build_oracle(workdir, name, flags=()):
    """oracle/hpk_oracle.c -> an object file built with `flags`"""
    obj = str(workdir / (name + "_oracle.o"))
    subprocess.check_call(["gcc", opt(flags), "-std=c11", "-D_GNU_SOURCE", *flags, "-c", os.path.join(REPO, "oracle", "hpk_oracle.c"),
                           "-o", obj])
    return obj


def build_emu(workdir, name, flags=(), source=None, oracle=True):
    """tests/emu/<source>.cpp (default: <name>.cpp) -> the program workdir/<name>, it and the oracle object it links
    built with the same `flags` (none: -O2; a sanitizer's: -O1)"""
    src = os.path.join(HERE, "emu", (source or name) + ".cpp")
    obj = str(workdir / (name + ".o"))
    subprocess.check_call(["g++", "-std=c++17", opt(flags), *flags, "-I", os.path.join(REPO, "loona_amd", "csrc"),
                           "-I", os.path.join(HERE, "emu"), "-c", src, "-o", obj])
    objs = [obj] + ([build_oracle(workdir, name, flags)] if oracle else [])
    subprocess.check_call(["g++", *flags, "-o", str(workdir / name), *objs, "-lpthread"])
    return str(workdir / name)


def has_symbol(exe, symbol):
    """whether the program's symbol table names `symbol` (a sanitizer's runtime entry point: a build that silently
    dropped the sanitizer cannot pass for one that has it)"""
    out = subprocess.run(["nm", "-a", exe], capture_output=True, text=True, check=True).stdout
    return any(line.split()[-1].startswith(symbol) for line in out.splitlines() if line.split())


def assert_no_reports(p):
    for word in REPORTS:
        assert word not in p.stderr, p.stderr[-4000:]


def assert_clean(p, ok="ok: 0 mismatches"):
    """exit status 0, the program's own verdict line, and no sanitizer report"""
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-4000:]
    assert ok in p.stdout, p.stdout[-3000:]
    assert_no_reports(p)
