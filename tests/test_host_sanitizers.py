"""The host codec (hpk_cpu.cpp, hpk_hdec.cpp, hpk_henc.cpp, hpk_h2.cpp) under ASan + UBSan and under TSan, stand-alone (no GPU needed).

tests/host/host_driver.cpp is a program of its own around the C ABI (include/hpk.h); it is built here three ways (plain
-O2, -fsanitize=address,undefined, -fsanitize=thread), each time together with the host sources and with
tests/host/device_stubs.cpp in place of the device half: libhpk.so is not linked, nothing is loaded into python, and the
driver only ever passes ctx == NULL (a device stub that is reached aborts). The case files (tests/host_cases.py) carry
the inputs of the suite's other tests and the expected results from oracle/hpack_ref.py and the C oracle; the driver
hands every input to the library as an exact-size heap copy and checks every result itself.
  codec    every decode corpus in one call each (the seeded corruptions, the random and the scan's placed blocks, every
           truncation of the RFC 7541 App. C blocks on its primed table and on a fresh one, the apply's placed cases, a
           slice of the interop stories, the table churn, the Huffman error vectors), then the encoder: the interop stories' header lists through
           hpk_henc_encode (HPK_E_NOSPACE one below the need) and hpk_henc_encode_blocks (an injected batch failure);
  frames   tests/test_h2.py's frame sequences through hpk_h2_read_frames, and the single-literal and CPU batch calls;
  threads  four callers at once, each decoding (encoding) >= 1,024 blocks per call on its own decoders: one owns the
           process-wide pool, the others spawn their own threads, all share hpk_blocks_out_free's kept buffers;
  fork     a pooled call, fork(), the same call in the child (ASan build and plain build only).
What this cannot cover are the ctx != NULL branches of hpk_hdec.cpp and hpk_henc.cpp: they need the device (the GPU tests)."""

import os
import re
import subprocess

import pytest

import blocks_scan_cases as bc
import h2_cases as hc
import host_cases as cases
import san_util

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SOURCES = [os.path.join(HERE, "host", "host_driver.cpp"), os.path.join(HERE, "host", "device_stubs.cpp")] + \
    [os.path.join(REPO, "loona_amd", "csrc", f) for f in ("hpk_cpu.cpp", "hpk_hdec.cpp", "hpk_henc.cpp", "hpk_h2.cpp")]
CALLERS, ROUNDS = 4, 3


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    if not san_util.have_compilers():
        pytest.skip("no host C/C++ compiler")
    return tmp_path_factory.mktemp("host_driver")


def build(workdir, name, flags):
    """the driver, the stubs and the host sources, every one compiled here with the same flags"""
    exe = str(workdir / name)
    subprocess.check_call(["g++", "-std=c++17", san_util.opt(flags), "-Wall", *flags, *SOURCES, "-o", exe, "-lpthread"])
    return exe


@pytest.fixture(scope="module")
def plain(workdir):
    exe = build(workdir, "host_driver", [])
    assert not san_util.has_symbol(exe, "__asan_init") and not san_util.has_symbol(exe, "__tsan_init")
    return exe


@pytest.fixture(scope="module")
def asan(workdir):
    exe = build(workdir, "host_driver_asan", san_util.ASAN)
    assert san_util.has_symbol(exe, "__asan_init"), "the ASan build holds no AddressSanitizer runtime"
    return exe


@pytest.fixture(scope="module")
def tsan(workdir):
    exe = build(workdir, "host_driver_tsan", san_util.TSAN)
    assert san_util.has_symbol(exe, "__tsan_init"), "the TSan build holds no ThreadSanitizer runtime"
    return exe


@pytest.fixture(scope="module")
def files(workdir):
    """{name: (path, cases)}: the case files, written once"""
    out = {}

    def write(name, sections, n):
        path = str(workdir / (name + ".bin"))
        with open(path, "wb") as f:
            f.write(cases.case_file(sections))
        out[name] = (path, n)

    # codec: every decode corpus a section of one call, then the encoder's two sections
    sections, total = [], 0
    corp = cases.decode_corpora()
    assert set(corp) == {"corrupted", "corrupted9", "random", "rfc", "placed", "interop", "rfc_prefixes", "churn", "huffman"}
    nprefix = sum(len(w) for w in bc.rfc_blocks())  # every proper prefix of every block
    assert len(corp["rfc"]) == len(corp["rfc_prefixes"]) == nprefix and len(corp["random"]) > 3000 and len(corp["placed"]) >= 35
    for name in sorted(corp):
        body, n = cases.decode_section(*cases.from_decoders(corp[name]))
        sections.append((cases.DECODE, body))
        total += n
    stories = cases.story_lists(2)  # (every other interop story)
    assert len(stories) >= 60
    for specs, calls in (cases.encode_single_calls(stories[:20]), cases.encode_block_calls(stories)):
        body, n = cases.encode_section(specs, calls)
        sections.append((cases.ENCODE, body))
        total += n
    write("codec", sections, total)
    # frames: the HTTP/2 layer and the Huffman entry points
    h2 = cases.h2_section()
    assert h2.seen_errors == set(range(10)), "a connection error of hpk_h2_error does not occur in the sequences"
    body, n = h2.body()
    hbody, hn, statuses = cases.huffman_section()
    assert statuses == {0, 1, 2, 3}
    write("frames", [(cases.H2, body), (cases.HUFFMAN, hbody)], n + hn)
    # threads: CALLERS callers, ROUNDS rounds; a decode call and encode calls of >= 1,024 blocks
    decs, calls = cases.from_decoders(cases.interop_slice(1024, start=40))
    assert len(calls) == 1 and len(calls[0]) >= 1024
    dbody, dn = cases.decode_section(decs, calls)
    specs, ecalls = cases.encode_block_calls(stories[:40], per_call=20)
    assert sum(len(b) >= 1024 for _, b in ecalls) >= 2
    ebody, en = cases.encode_section(specs, ecalls)
    write("threads", [(cases.THREADS, cases.u32(CALLERS, ROUNDS, 1) + dbody), (cases.THREADS, cases.u32(CALLERS, ROUNDS, 2) + ebody)],
          CALLERS * ROUNDS * (dn + en))
    # fork: the same pooled decode call in the parent, in the child, in the parent again
    write("fork", [(cases.FORK, dbody)], 2 * dn + 1)
    return out


def run(exe, case, timeout=600):
    path, n = case
    env = dict(os.environ, HPK_HDEC_THREADS="4")  # (the pool is entered whatever the machine's core count)
    p = subprocess.run([exe, path], capture_output=True, text=True, timeout=timeout, env=env)
    return p, n


def check(p, n):
    """exit status 0, the verdict line with the expected case count, no sanitizer report, no device stub reached"""
    san_util.assert_clean(p, f"ok: 0 mismatches in {n} cases")
    assert "device stub reached" not in p.stderr


def counts(out, key):
    return {int(k): int(v) for k, v in re.findall(r"^%s (\d+): (\d+)$" % key, out, re.M)}


def test_model_of_the_frame_layer_is_pinned():
    """h2_cases.ref_read gives what tests/test_h2.py states by hand: the placed connection errors, the continuation
    check's order, and the interop connections' blocks (host_cases.h2_section asserts the rest as it writes)"""
    for frames, err, _ in hc.CONNECTION_ERRORS:
        c = hc.RefConn()
        errors, _, _ = hc.ref_read([c], [b"".join(frames)])
        assert errors == [hc.H2_NAMES[err]] and c.error == hc.H2_NAMES[err]
    for second, err in hc.CHECK_ORDER:
        errors, _, blocks = hc.ref_read([hc.RefConn()], [hc.frame(hc.HEADERS, 0, 1, hc.BLOCK[:5]) + second])
        assert errors == [hc.H2_NAMES[err]] and blocks == []


def test_plain_build_and_coverage(plain, files):
    """The unsanitized build passes every file, and the corpora reach what they are meant to reach (so they cannot
    quietly shrink): every hpk_block_error the C ABI can return, every hpk_h2_error, all three Huffman error statuses as
    a block's detail, and in the threaded mode calls of >= 1,024 blocks by callers that overlapped.
    HPK_BLK_INT_VALUE_TOO_LARGE is unused by the reference; HPK_BLK_INT_INVALID_PREFIX cannot occur either: every
    prefix decode_integer is called with is a constant between 4 and 7 (hpk_hdec.cpp: scan_block, scan_string)."""
    blk, h2, detail = {}, {}, {}
    for name in ("codec", "frames", "threads", "fork"):
        p, n = run(plain, files[name])
        check(p, n)
        for acc, key in ((blk, "blk_error"), (h2, "h2_error"), (detail, "huff_detail")):
            for k, v in counts(p.stdout, key).items():
                acc[k] = acc.get(k, 0) + v
        check_mode(p, name)
    assert set(blk) >= {0, 1, 2, 4, 6, 7, 8, 9} and not set(blk) & {3, 5}, blk
    assert set(h2) == set(range(10)), h2
    assert set(detail) >= {1, 2, 3}, detail


def check_mode(p, name):
    """the threaded mode's own report, from any build: CALLERS >= 4 callers, calls of >= 1,024 blocks in both kinds, and
    callers seen inside a call at the same time (so one owned the pool and another took the spawn-your-own-threads
    branch of Pool::run); the fork mode's: the child's exit status"""
    if name == "threads":
        lines = re.findall(r"^threads: (\d+) callers, (\d+) rounds, kind (\d), (\d+) calls of >= 1024 blocks so far, max overlap (\d+)$",
                           p.stdout, re.M)
        assert [ln[2] for ln in lines] == ["1", "2"], p.stdout[-2000:]
        big = 0
        for callers, rounds, _, calls_so_far, overlap in lines:
            assert int(callers) == CALLERS >= 4 and int(rounds) == ROUNDS
            assert int(calls_so_far) >= big + CALLERS * ROUNDS, "no call of >= 1,024 blocks in this mode"
            big = int(calls_so_far)
            assert int(overlap) >= 2, "the callers never overlapped: the pool's busy branch was not taken"
    if name == "fork":
        assert "fork: child exit status 0" in p.stdout


@pytest.mark.parametrize("name", ["codec", "frames", "threads", "fork"])
def test_under_asan_and_ubsan(asan, files, name):
    p, n = run(asan, files[name])
    check(p, n)
    check_mode(p, name)


@pytest.mark.parametrize("name", ["codec", "frames", "threads"])
def test_under_tsan(tsan, files, name):
    """(no fork under TSan.) On some kernels a TSan binary dies at start-up with TSan's own `unexpected memory mapping`
    message; only then is this skipped, with the message."""
    p, n = run(tsan, files[name], timeout=900)
    if p.returncode != 0 and "unexpected memory mapping" in p.stderr and "ok:" not in p.stdout and "mismatch" not in p.stdout:
        pytest.skip("ThreadSanitizer cannot start on this kernel: " + p.stderr.strip().splitlines()[0])
    check(p, n)
    check_mode(p, name)
