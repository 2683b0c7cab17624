// device_stubs.cpp — the device half of libhpk as the stand-alone host driver sees it (tests/host/host_driver.cpp,
// tests/test_host_sanitizers.py): the host units hpk_cpu.cpp, hpk_hdec.cpp, hpk_henc.cpp and hpk_h2.cpp are compiled by themselves
// under a host sanitizer, and the symbols they take from hpk_ctx.hip and the hpk_calls_*.hip call layer are defined
// here instead.
//
// The driver only ever passes ctx == NULL, so:
//   * a stub the NULL-context path can legitimately reach answers what the real function answers for no context:
//     hpk_ctx_block_scan / _apply / _plan give HPK_BLOCK_*_HOST (hpk_internal.h), hpk_set_err_msg stores the calling
//     thread's message and returns the code, hpk_last_error returns that message;
//   * every other stub prints its name and calls abort(): a run that ends normally proves that nothing device-side
//     was reached.
// If a later change gives the host units another symbol of the device half, the driver no longer links. That is the
// intended signal: decide here which of the two kinds the new symbol is.
#include <stdio.h>
#include <stdlib.h>

#include <string>

#include "../../include/hpk.h"
#include "../../loona_amd/csrc/hpk_internal.h"

namespace {

[[noreturn]] void reached(const char* name) {
    fprintf(stderr, "device stub reached: %s\n", name);
    abort();
}

thread_local std::string t_err;

}  // namespace

// ---- reachable without a context ---------------------------------------------------------------------------------
int hpk_set_err_msg(const char* what, int code) {
    t_err = what ? what : "";
    return code;
}

extern "C" const char* hpk_last_error(const hpk_ctx*) { return t_err.c_str(); }

int hpk_ctx_block_scan(const hpk_ctx* c) {
    if (c) reached("hpk_ctx_block_scan with a context");
    return HPK_BLOCK_SCAN_HOST;
}

int hpk_ctx_block_apply(const hpk_ctx* c) {
    if (c) reached("hpk_ctx_block_apply with a context");
    return HPK_BLOCK_APPLY_HOST;
}

int hpk_ctx_block_plan(const hpk_ctx* c) {
    if (c) reached("hpk_ctx_block_plan with a context");
    return HPK_BLOCK_PLAN_HOST;
}

// ---- the device half proper: never reached with ctx == NULL --------------------------------------------------------
int hpk_ctx_pinned(hpk_ctx*, size_t, void**) { reached("hpk_ctx_pinned"); }

int hpk_decode_host_begin(hpk_ctx*, const uint8_t*, size_t, const uint32_t*, uint32_t, uint8_t*, size_t, const uint32_t*,
                          uint32_t*, uint8_t*, int*, uint32_t*) {
    reached("hpk_decode_host_begin");
}

int hpk_host_chunk_wait(hpk_ctx*, int) { reached("hpk_host_chunk_wait"); }

int hpk_decode_host_end(hpk_ctx*) { reached("hpk_decode_host_end"); }

int hpk_ctx_max_chunks() { reached("hpk_ctx_max_chunks"); }

int hpk_blocks_device(hpk_ctx*, const uint8_t*, const uint32_t*, uint32_t, hpk_blkdev*, hpk_applyplan*) {
    reached("hpk_blocks_device");
}

int hpk_plan_device(hpk_ctx*, hpk_planjob*) { reached("hpk_plan_device"); }

void hpk_ctx_plan_answered(hpk_ctx*) { reached("hpk_ctx_plan_answered"); }

extern "C" int hpk_encode_strings_packed(hpk_ctx*, const uint8_t*, size_t, const uint32_t*, uint32_t, const uint8_t*, uint8_t*,
                                         size_t, uint32_t*, uint32_t*, uint8_t*, int) {
    reached("hpk_encode_strings_packed");
}

extern "C" int hpk_test_blkapply_geometry(uint32_t*, uint32_t*, uint32_t*) { reached("hpk_test_blkapply_geometry"); }

extern "C" int hpk_test_blkplan_geometry(uint32_t*, uint32_t*, uint32_t*, uint32_t*) { reached("hpk_test_blkplan_geometry"); }
