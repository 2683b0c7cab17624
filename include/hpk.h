/*
 * hpk.h — C ABI of the MI355X-native HPACK Huffman codec (RFC 7541 §5.2 + App. B).
 *
 * This is the drop-in boundary for loona-hpack's Huffman string-literal path.
 * Every entry point is `extern "C"`, takes plain pointers and sizes, never
 * throws across the boundary and never panics on input bytes.
 *
 * Reference interfaces each entry point replaces (paths relative to
 * bearcove/loona @ 2025-05-09):
 *
 *   hpk_huffman_decode_one   HuffmanDecoder::new().decode(buf)
 *                            crates/loona-hpack/src/huffman.rs:86-88, :95-161
 *                            called from decode_string, crates/loona-hpack/src/decoder.rs:148-149
 *   hpk_status               HuffmanDecoderError {PaddingTooLarge, InvalidPadding, EOSInString}
 *                            crates/loona-hpack/src/huffman.rs:28-41 (1:1 mapping, 0 = Ok)
 *   hpk_decode_batch         many decode_string Huffman branches at once
 *                            (decoder.rs:143-157), literals gathered across header blocks /
 *                            streams by the caller (crates/loona/src/h2/server.rs:1619-1638)
 *   hpk_huffman_encode_one   NEW: the reference never Huffman-encodes
 *   hpk_encode_batch         (crates/loona-hpack/src/encoder.rs:296-307 writes raw literals);
 *                            this is the H-bit branch encode_string_literal would add.
 *
 * Threading: one hpk_ctx per host thread (loona is !Send, thread-per-core,
 * crates/buffet/src/lib.rs:38-49). A context owns a HIP stream (or borrows
 * one via hpk_ctx_set_stream) and grow-only device scratch buffers.
 */
#ifndef HPK_H
#define HPK_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- per-literal status (one byte per literal in batch calls) ---------- */
typedef enum hpk_status {
    HPK_OK = 0,                 /* Ok(Vec<u8>)                                 */
    HPK_PADDING_TOO_LARGE = 1,  /* HuffmanDecoderError::PaddingTooLarge  (>7 residual bits) */
    HPK_INVALID_PADDING = 2,    /* HuffmanDecoderError::InvalidPadding   (residual != EOS MSBs) */
    HPK_EOS_IN_STRING = 3,      /* HuffmanDecoderError::EOSInString      (30-bit EOS decoded) */
    HPK_OUTPUT_OVERFLOW = 4,    /* not a reference error: caller's out capacity < decoded size */
    HPK_BAD_OFFSETS = 5,        /* not a reference error: device-pointer call whose offsets are not
                                   non-decreasing or pass a blob's capacity; the call's results are
                                   void (see hpk_decode_batch) */
    /* hpk_decode_strings_packed only: decode_string's errors before any Huffman work (decoder.rs:67-143).
       As hpk_block_error they are HPK_BLK_INT_TOO_MANY_OCTETS (2), HPK_BLK_INT_NOT_ENOUGH_OCTETS (4) and
       HPK_BLK_STR_NOT_ENOUGH_OCTETS (6), in this order. */
    HPK_PREFIX_TOO_MANY_OCTETS = 6,   /* IntegerDecodingError::TooManyOctets: continuation bit on the 5th octet */
    HPK_PREFIX_NOT_ENOUGH_OCTETS = 7, /* IntegerDecodingError::NotEnoughOctets: empty window, or it ends inside the integer */
    HPK_STRING_NOT_ENOUGH_OCTETS = 8  /* StringDecodingError::NotEnoughOctets: consumed + len passes the window */
} hpk_status;

/* ---- API return codes (negative = the call itself failed) -------------- */
#define HPK_E_OK 0
#define HPK_E_INVAL (-1)    /* bad argument (null pointer, offsets not monotone, ...) */
#define HPK_E_NOSPACE (-2)  /* single-literal call: `cap` too small               */
#define HPK_E_DEVICE (-3)   /* HIP runtime error; see hpk_last_error()            */
#define HPK_E_NODEVICE (-4) /* no GPU / kernel image for gfx950 not loadable      */

/* ---- flags for batch calls --------------------------------------------- */
#define HPK_PTR_HOST 0x0   /* all buffers are host memory: staged H2D / run / D2H in overlapping
                              chunks on the ctx's copy streams, synchronous                */
#define HPK_PTR_DEVICE 0x1 /* all buffers are device memory: enqueue on the ctx stream */
#define HPK_ASYNC 0x2      /* with HPK_PTR_DEVICE: return without synchronising       */

/* Upper bounds for output capacity. Every HPACK code is >= 5 bits and <= 30 bits. */
size_t hpk_decoded_bound(size_t encoded_len); /* floor(8n/5)    */
size_t hpk_encoded_bound(size_t decoded_len); /* ceil(30n/8)    */

/* Canonical Huffman encoded length of `in` (bytes, incl. EOS-prefix padding). */
size_t hpk_huffman_encoded_len(const uint8_t* in, size_t n);

/* ---- single-literal CPU entry points (the scalar drop-in) --------------- */
/* Decode n bytes. Returns an hpk_status (>= 0) and sets *out_len to the number
 * of bytes written (also on error: the symbols decoded before the error), or a
 * negative HPK_E_* code. `out` may be NULL iff cap == 0. */
int hpk_huffman_decode_one(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);

/* Encode n bytes (MSB-first codes, padded with the most significant bits of
 * EOS). Returns HPK_E_OK or HPK_E_NOSPACE (then *out_len = cap and out holds the encoding's
 * first cap bytes, as the batch calls' HPK_OUTPUT_OVERFLOW). */
int hpk_huffman_encode_one(const uint8_t* in, size_t n, uint8_t* out, size_t cap, size_t* out_len);

/* ---- device context ----------------------------------------------------- */
typedef struct hpk_ctx hpk_ctx;

hpk_ctx* hpk_ctx_create(int device);           /* NULL on failure (see hpk_last_error(NULL)) */
void hpk_ctx_destroy(hpk_ctx* ctx);
/* Run on `hip_stream`: NULL = the ctx's own (non-blocking) stream; HPK_STREAM_LEGACY = the
 * legacy null stream (stream 0, what torch's default stream is). */
#define HPK_STREAM_LEGACY ((void*)(intptr_t)-1)
int hpk_ctx_set_stream(hpk_ctx* ctx, void* hip_stream);
void* hpk_ctx_stream(hpk_ctx* ctx);
int hpk_ctx_sync(hpk_ctx* ctx);
const char* hpk_last_error(const hpk_ctx* ctx); /* thread-local text of the last failure */

/* ---- batch decode --------------------------------------------------------
 * Literal i occupies in_blob[in_off[i] .. in_off[i+1]) and may write
 * out_blob[out_off[i] .. out_off[i+1]) (its capacity; hpk_decoded_bound of
 * its length always suffices). On return out_len[i] = bytes decoded and
 * status[i] = hpk_status. Bytes of a literal's region past out_len[i] are
 * unspecified. Offsets are u32 (one shard): in_off/out_off have n+1 entries,
 * must be non-decreasing and at most HPK_MAX_OFFSET; in_cap / out_cap are the
 * byte sizes of in_blob / out_blob (the reference checks a literal's length
 * against its buffer before any Huffman work, decoder.rs:138-142).
 *
 * Host pointers: offsets and capacities are checked before anything is copied
 * (HPK_E_INVAL). Device pointers: the offsets live in device memory, so the
 * kernels check them as they read them: a literal whose offsets decrease or
 * pass a capacity makes the kernel write HPK_BAD_OFFSETS (out_len 0) for it and
 * for any other literals of the same batch it has not written yet, and nothing
 * is read or written outside [in_blob, in_blob + in_cap) and
 * [out_blob, out_blob + out_cap). The context keeps a sticky error flag: a
 * synchronous call returns HPK_E_INVAL when it is set (and clears it);
 * hpk_ctx_check() does the same after HPK_ASYNC calls. out_len and status
 * must have room for n entries. */
#define HPK_MAX_OFFSET 0xFFFFFFDFu /* offsets + a 16-byte misalignment + a 16-byte chunk stay < 2^32 */
int hpk_decode_batch(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                     uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                     uint8_t* status, int flags);

/* ---- batch decode, compacted output --------------------------------------
 * The reference returns each literal as an exact-length Vec (huffman.rs:98, 160); this form writes
 * each literal's decoded bytes exactly, in runs with no region slack between a run's literals, instead of
 * into bound-sized regions: on return literal i's bytes are out_blob[out_off[i] .. out_off[i] + out_len[i])
 * and out_off[n] is the end of the span written to. The span is NOT gap-free: see the layouts below
 * (listed literals keep their bound, and the wave-fill kernel's workgroup shares end in unwritten tails).
 * out_off (n+1 entries) is an OUTPUT here. Literals are packed in runs (a fill of the kernel at a
 * time, literal order inside a run, runs in completion order), so out_off is not monotone. A literal
 * the kernel hands to its long- or huge-literal phase keeps a region of its 4-rounded decoded bound,
 * the bytes past its out_len unwritten: every literal of >= 64 encoded bytes, and every literal
 * (short ones too) of a workgroup range the kernel lists whole because most of its input bytes are
 * in such literals. Batches the wave-fill kernel decodes (every batch unless the workgroup-fill kernel is
 * forced by hpk_ctx_set_decode_kernel) are packed per workgroup: workgroup w's runs and listed regions fill
 * its literal range [a, b)'s share [U(a), U(b)) from its start, the rest of the share unwritten, where
 * U(i) = floor(8 (in_off[i] - in_off[0]) / 5) + 4 i (it holds every 4-rounded decoded bound of the
 * range), and out_off[n] = U(n); the workgroup-fill kernel packs every run from one device cursor and
 * out_off[n] is its end.
 * Device pointers only (HPK_PTR_DEVICE, optionally HPK_ASYNC); out_cap must be at least
 * hpk_decoded_bound(in_cap) + 4 * n (HPK_E_INVAL otherwise). Statuses, errors and offsets checks
 * as hpk_decode_batch. */
int hpk_decode_batch_compact(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                             uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                             uint8_t* status, int flags);

/* ---- batch decode, packed output: the decoded bytes end to end, in literal order ------------
 * The reference hands each literal back as an exact-length Vec (huffman.rs:98, 160); this form gives
 * what those Vecs would be, concatenated: on return out_off (n+1 entries, an OUTPUT) is the exclusive
 * sum of out_len (out_off[0] = 0, non-decreasing, out_off[n] = the decoded total), literal i's bytes are
 * out_blob[out_off[i] .. out_off[i+1]) with no gap and no slack, and the blob can be sent, copied to the
 * host or sliced as it is. status[i] and out_len[i] are exactly hpk_decode_batch's (an error literal
 * keeps the bytes decoded before its error).
 * out_cap may be any size (the caller does not know the total in advance; hpk_decoded_bound(in_cap)
 * always suffices). No byte of out_blob at or past out_off[n] is written and nothing outside
 * [out_blob, out_blob + out_cap). If out_off[n] > out_cap the bytes below out_cap are written, the rest
 * are not, and out_off, out_len and status are still complete: a synchronous call then returns
 * HPK_E_NOSPACE; after an HPK_ASYNC call the caller compares out_off[n] with its capacity itself.
 * Bad offsets as hpk_decode_batch (status HPK_BAD_OFFSETS with out_len 0, the sticky flag, HPK_E_INVAL
 * from the synchronous call, which wins over HPK_E_NOSPACE). n == 0 writes out_off[0] = 0.
 * Device pointers only (HPK_PTR_DEVICE, optionally HPK_ASYNC); hpk_decoded_bound(in_cap) + 4 n must not
 * pass HPK_MAX_OFFSET (HPK_E_INVAL, as the compacted form). Always the launch path: the small-call
 * mode's persistent kernel does not answer it.
 * How: the region decode (hpk_decode_batch's kernels, untouched) into scratch of the context, laid out
 * by the literals' 4-rounded decoded bounds, then a scan of out_len and an ordered pack kernel that
 * writes out_blob in whole aligned 16-byte chunks. The scratch is hpk_decoded_bound(in_cap) + 4 n bytes
 * per stream the context is used on (grow-only, freed with the context): about 1.9 GB for a shard of
 * 32M literals. */
int hpk_decode_batch_packed(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                            uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                            uint8_t* status, int flags);

/* The pack step on its own, for results the caller already holds in the region or the compacted
 * layout: literal i is src_blob[src_off[i] .. src_off[i] + src_len[i]); the starts may come in any
 * order (n entries of src_off are read, so a region form's n+1 array can be passed as it is). Writes
 * dst_off (n+1 entries: the exclusive sum of src_len) and the bytes end to end, dst_blob[dst_off[i] ..
 * dst_off[i+1]) = literal i. Capacity, HPK_E_NOSPACE and what is left unwritten as
 * hpk_decode_batch_packed. A literal with src_off[i] + src_len[i] > src_cap is a bad offset: it
 * contributes length 0 and sets the sticky flag (HPK_E_INVAL from a synchronous call); so does every
 * literal when the lengths' sum passes HPK_MAX_OFFSET. Nothing outside [src_blob, src_blob + src_cap)
 * is read. Device pointers only (HPK_PTR_DEVICE, optionally HPK_ASYNC). */
int hpk_pack_batch(hpk_ctx* ctx, const uint8_t* src_blob, size_t src_cap, const uint32_t* src_off,
                   const uint32_t* src_len, uint32_t n, uint8_t* dst_blob, size_t dst_cap, uint32_t* dst_off, int flags);

/* ---- batch encode --------------------------------------------------------
 * Symmetric: literal i = in_blob[in_off[i] .. in_off[i+1]) is Huffman-encoded
 * into out_blob[out_off[i] ..) with capacity out_off[i+1]-out_off[i]
 * (hpk_encoded_bound suffices). out_len[i] = encoded bytes; status[i] is
 * HPK_OK or HPK_OUTPUT_OVERFLOW (out_len = the capacity, holding the
 * encoding's prefix). Offsets and capacities as hpk_decode_batch. */
int hpk_encode_batch(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                     uint8_t* out_blob, size_t out_cap, const uint32_t* out_off, uint32_t* out_len,
                     uint8_t* status, int flags);

/* ---- batch encode: the encoded lengths alone ----------------------------------------------
 * out_len[i] = hpk_huffman_encoded_len of literal i = in_blob[in_off[i] .. in_off[i+1]): ceil(code bits / 8),
 * 0 for an empty literal, with no byte encoded. It is the number the H-bit branch that
 * encode_string_literal (crates/loona-hpack/src/encoder.rs:296-307) would add needs per string: RFC 7541
 * §5.2 is used only where this is strictly below the raw length. A literal whose offsets decrease or pass
 * in_cap counts 0 and sets the sticky flag (a synchronous call then returns HPK_E_INVAL): hpk_pack_batch's
 * rule; it voids no other literal. Cost of a bad batch: the up to 1,024 consecutive literals the kernel
 * was looking at when it met the bad one are each summed by one lane, byte by byte, large ones included. Nothing outside [in_blob, in_blob + in_cap) is read (as hpk_encode_batch,
 * in whole aligned 16-byte chunks that hold a byte of the blob). n == 0 is a no-op. Device pointers only
 * (HPK_PTR_DEVICE, optionally HPK_ASYNC), on the context's stream; always the launch path. No scratch. */
int hpk_encoded_len_batch(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off,
                          uint32_t n, uint32_t* out_len, int flags);

/* ---- batch encode, packed output: the encoded bytes end to end, in literal order ------------
 * hpk_encode_batch needs a region per literal, and the only size known before encoding is
 * hpk_encoded_bound (3.75x the input; header text encodes to about 0.8x). This form needs none (the H-bit
 * branch of crates/loona-hpack/src/encoder.rs:296-307 writes each string right after its length prefix):
 * out_off (n+1 entries) is an OUTPUT, the exclusive sum of out_len; literal i's encoding is
 * out_blob[out_off[i] .. out_off[i+1]) with no gap, and out_off[n] is the encoded total. n == 0 writes
 * out_off[0] = 0. The bytes are exactly hpk_encode_batch's for a region that is large enough, out_len[i] is
 * the full encoded length, and status[i] is HPK_OK or HPK_BAD_OFFSETS, never HPK_OUTPUT_OVERFLOW. The result
 * is hpk_decode_batch_packed's input as it stands (out_off as in_off).
 * out_cap may be any size: the bytes below min(out_off[n], out_cap) are written, nothing at or past that
 * point nor outside [out_blob, out_blob + out_cap), and out_off, out_len and status are complete either way.
 * If out_off[n] > out_cap a synchronous call returns HPK_E_NOSPACE; after HPK_ASYNC the caller compares.
 * Bad offsets: a literal whose input offsets decrease or pass in_cap gets HPK_BAD_OFFSETS and out_len 0 and
 * sets the sticky flag (HPK_E_INVAL from the synchronous call, which wins over HPK_E_NOSPACE). The call may
 * void other literals of the batch the same way (this version voids none: every other literal is encoded);
 * whatever it voids, out_off is the exclusive sum of out_len and every literal with status HPK_OK holds its
 * complete encoding. If the encoded total passes HPK_MAX_OFFSET, every out_off is 0, every literal is void
 * (HPK_BAD_OFFSETS, out_len 0), nothing is written to out_blob and the flag is set; hpk_encoded_bound(in_cap)
 * may pass 4 GiB as long as the true total does not.
 * Device pointers only (HPK_PTR_DEVICE, optionally HPK_ASYNC), on the context's stream with its per-stream
 * scratch; always the launch path. How: the length pass (hpk_encoded_len_batch's kernel) writes out_len and
 * status, a scan of out_len with 64-bit tile sums writes out_off, and the encode kernel's packed
 * instantiation writes every literal at its final place. The scratch is the scan's tile sums (8 bytes per
 * 4,096 literals): there is no intermediate blob and no second copy. The input offsets must not change
 * between the call and its completion. Cost of a bad batch: the length pass as hpk_encoded_len_batch, and
 * in the encode every literal from the bad one to the end of its workgroup's share of the batch (the batch
 * is split by bytes over up to two workgroups per CU) is encoded by one lane, byte by byte. */
int hpk_encode_batch_packed(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                            uint8_t* out_blob, size_t out_cap, uint32_t* out_off, uint32_t* out_len,
                            uint8_t* status, int flags);

/* ---- batch encode, packed string literals: H bit, length prefix, shorter form ----------------
 * What an HPACK encoder writes per string (RFC 7541 §5.2; encode_string_literal, crates/loona-hpack/src/
 * encoder.rs:296-307): the payload's length as a 7-bit-prefix integer (§5.1; encode_integer_into,
 * encoder.rs:93-122), 0x80 ORed into its first octet for the Huffman form, then the payload: the raw octets or
 * their Huffman coding. policy[i] (n entries, or NULL = all HPK_STR_AUTO) picks literal i's form: */
#define HPK_STR_AUTO     0  /* H-bit form iff the literal is non-empty and its Huffman encoding is strictly
                               shorter than its raw bytes; else raw (put_string, hpack_ref.Encoder._string) */
#define HPK_STR_RAW      1  /* always raw: byte-identical to encode_string_literal */
#define HPK_STR_HUFFMAN  2  /* always the H-bit form (an empty literal is the single octet 0x80) */
#define HPK_STR_VERBATIM 3  /* the bytes as they are, no prefix: representation octets the host has made final */
/* Literal i's representation is out_blob[out_off[i] .. out_off[i+1]): under policies 0-2 the prefix (1 to 6
 * octets) followed by the payload, under HPK_STR_VERBATIM the input bytes alone. out_len[i] is the whole
 * representation, prefix included; out_off (n+1 entries, an OUTPUT) is the exclusive sum of out_len; status[i]
 * is HPK_OK or HPK_BAD_OFFSETS. The chosen form can be read from out_blob[out_off[i]] & 0x80, and Huffman
 * payload bytes are exactly hpk_encode_batch_packed's. Sizing: len + 6 bytes per literal always suffice unless
 * the policy is HPK_STR_HUFFMAN, where hpk_encoded_bound(len) + 6 do.
 * Capacity, errors and offsets as hpk_encode_batch_packed: out_cap may be any size; nothing is written at or
 * past min(out_off[n], out_cap) nor outside the blob; HPK_E_NOSPACE from a synchronous call when out_off[n] >
 * out_cap, and HPK_E_INVAL wins over it; n == 0 writes out_off[0] = 0; a literal whose input offsets decrease
 * or pass in_cap, or whose policy is above 3, is void (HPK_BAD_OFFSETS, out_len 0, the sticky flag), every
 * literal with status HPK_OK holds its complete representation, and this version voids no other literal; a
 * total past HPK_MAX_OFFSET voids every literal, zeroes every out_off and writes no byte. The context's stream
 * and per-stream scratch; always the launch path.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC; or HPK_PTR_HOST, synchronous: offsets and policies are
 * checked on the host before anything is copied (HPK_E_INVAL, nothing written), the input is staged in one
 * piece into grow-only scratch of the stream's slot, and exactly min(out_off[n], out_cap) bytes come back with
 * out_off, out_len and status.
 * How: the length pass (hpk_encoded_len_batch's kernel) and an elementwise form step write out_len and
 * status, the length scan writes out_off, and one tile kernel writes prefixes, Huffman codes and raw bytes at
 * their final places through an LDS image in whole 16-byte chunks. No intermediate blob; the input is read
 * twice. A raw or verbatim literal larger than a tile (16 KiB of input) is copied by a whole workgroup, a
 * Huffman one is coded by one lane. Cost of a bad batch as hpk_encode_batch_packed. */
int hpk_encode_strings_packed(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                              const uint8_t* policy, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                              uint32_t* out_len, uint8_t* status, int flags);
/* The representations' lengths alone (out_len as above, 0 for a void literal, which sets the sticky flag), no
 * byte written: hpk_encoded_len_batch with the form and the prefix applied. Device pointers only
 * (HPK_PTR_DEVICE, optionally HPK_ASYNC). No scratch. */
int hpk_string_len_batch(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* in_off, uint32_t n,
                         const uint8_t* policy, uint32_t* out_len, int flags);

/* ---- batch decode, packed string literals: prefix, H bit, raw or Huffman ---------------------
 * The mirror of hpk_encode_strings_packed and the batch form of decode_string (crates/loona-hpack/src/
 * decoder.rs:135-163): string i is decode_string(&in_blob[str_off[i] .. str_end[i]]), that is the length as a
 * 7-bit-prefix integer (decode_integer, decoder.rs:67-125; non-canonical forms such as 7f 80 00 are accepted, as
 * there), the check that prefix octets + length stay inside the window, then the payload: borrowed as it is, or
 * Huffman-decoded when the first octet's 0x80 is set. The window may be longer than the string (the reference
 * passes "the rest of the block"), and windows of different strings may overlap or coincide. str_end == NULL is
 * the mirror form: str_off then has n + 1 entries and string i's window is [str_off[i], str_off[i+1]), which is
 * hpk_encode_strings_packed's out_off as it stands.
 * Outputs as hpk_decode_batch_packed: out_off (n + 1 entries, an OUTPUT) is the exclusive sum of out_len and
 * string i's bytes are out_blob[out_off[i] .. out_off[i+1]) with no gap. A raw string's bytes are its payload
 * verbatim (status HPK_OK); a Huffman string's bytes, out_len and status are exactly hpk_decode_batch's for its
 * payload (an error literal keeps the bytes decoded before its error). consumed (n entries, may be NULL): the
 * prefix octets + the payload length of every string whose prefix and length check passed, Huffman errors
 * included; otherwise 0. A string that fails before its payload has out_len 0, consumed 0 and status
 * HPK_PREFIX_TOO_MANY_OCTETS (reported whether or not more bytes follow the 5th octet),
 * HPK_PREFIX_NOT_ENOUGH_OCTETS or HPK_STRING_NOT_ENOUGH_OCTETS; the call itself still returns HPK_E_OK.
 * Capacity, HPK_E_NOSPACE, n == 0 and what is left unwritten as hpk_decode_batch_packed: out_cap may be any
 * size, nothing is written at or past min(out_off[n], out_cap) nor outside the blob, the arrays are complete
 * either way, and HPK_E_INVAL wins over HPK_E_NOSPACE. A string with str_off[i] > str_end[i] or str_end[i] >
 * in_cap (mirror form: decreasing offsets, or past in_cap) is void: HPK_BAD_OFFSETS, out_len 0, consumed 0, the
 * sticky flag; it voids no other string. hpk_decoded_bound(in_cap) + 4 n must not pass HPK_MAX_OFFSET
 * (HPK_E_INVAL). The Huffman payloads' total can pass in_cap only when payloads overlap: the sticky flag is then
 * set and the call's Huffman results are void in hpk_decode_batch's sense (those cut off get HPK_BAD_OFFSETS);
 * overlapping windows whose decoded total passes HPK_MAX_OFFSET zero every out_off, write no byte and set the
 * flag. Nothing outside [in_blob, in_blob + in_cap) is ever read, and of a window only the integer's octets and
 * the payload.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC; or HPK_PTR_HOST, synchronous: the windows are checked on the
 * host before anything is copied (HPK_E_INVAL, nothing written), the input is staged in one piece into grow-only
 * scratch of the stream's slot, and exactly min(out_off[n], out_cap) bytes come back with out_off, out_len,
 * consumed and status. Always the launch path: the small-call mode does not answer it.
 * How: a parse kernel (one thread per string), the ordered pack gathering the Huffman payloads into a contiguous
 * blob, hpk_decode_batch_packed's region decode of it (no decode kernel changes), an elementwise merge, the scan
 * of out_len, and the ordered pack with a source per string (the region scratch or the input blob). Scratch per
 * stream: hpk_decode_batch_packed's, plus in_cap bytes and 18 bytes per string. */
int hpk_decode_strings_packed(hpk_ctx* ctx, const uint8_t* in_blob, size_t in_cap, const uint32_t* str_off,
                              const uint32_t* str_end, uint32_t n, uint8_t* out_blob, size_t out_cap, uint32_t* out_off,
                              uint32_t* out_len, uint32_t* consumed, uint8_t* status, int flags);

/* Which decode kernel a context's batches use. All give identical results (the parity tests run
 * every case through each); they differ in speed. HPK_DECODE_AUTO (the default): the wave-fill kernel
 * for every batch (since round 6; it had been the workgroup-fill kernel below 4M literals). */
#define HPK_DECODE_AUTO 0
#define HPK_DECODE_FILL 1 /* workgroup fills: one fill at a time per CU, barriers between fills */
#define HPK_DECODE_WAVE 2 /* wave fills: every wave its own fills, no barriers between them */
int hpk_ctx_set_decode_kernel(hpk_ctx* ctx, int kind);

/* Small-call mode (opt-in; hpk_persist.h). A persistent kernel of `workgroups` (1-16) workgroups, its
 * decode tables resident in LDS, takes this context's synchronous device-pointer hpk_decode_batch
 * calls of 1..max_literals literals through a host-mapped doorbell (after the work already queued on
 * the context's stream): such a call skips the kernel launch and the stream synchronisation.
 * Results are identical to the launch path's (a batch with bad offsets is handed to the launch path).
 * While the kernel runs it holds `workgroups` CUs, which the context's batch kernels then leave out.
 * It exits after idle_ms (1-10000) without a call (the next small call starts it again), when the
 * mode is turned off (max_literals = 0) or when the context is destroyed. No counterpart in the
 * reference: loona decodes one connection's header block at a time (crates/loona/src/h2/server.rs:
 * 1619-1637), the granularity this mode serves. */
int hpk_ctx_set_small_mode(hpk_ctx* ctx, uint32_t max_literals, int workgroups, uint32_t idle_ms);

/* Read and clear the context's sticky device error flag (after HPK_ASYNC calls; synchronises the
 * ctx stream). Returns HPK_E_OK, HPK_E_INVAL (some call saw bad offsets) or HPK_E_DEVICE.
 * The flag belongs to the context, not to a stream: it reports a bad call made on any stream the
 * context was bound to (hpk_ctx_set_stream) once that call has run, so after async calls on
 * several streams synchronise each of them before relying on the answer; a synchronous call
 * returns (and clears) a flag left by an earlier async call on another stream. */
int hpk_ctx_check(hpk_ctx* ctx);

/* ---- batch calls on the host CPU ----------------------------------------
 * Same layout and results as the device calls, run by `nthreads` host threads over contiguous
 * literal shards balanced by bytes (thread-per-core, like loona). This is the table-driven CPU
 * path ("cpu-fast" in the bench), not the reference restatement. nthreads <= 0: the cores, at most
 * 16 and at least 2048 literals per thread. */
int hpk_decode_batch_cpu(const uint8_t* in_blob, const uint32_t* in_off, uint32_t n, uint8_t* out_blob,
                         const uint32_t* out_off, uint32_t* out_len, uint8_t* status, int nthreads);
int hpk_encode_batch_cpu(const uint8_t* in_blob, const uint32_t* in_off, uint32_t n, uint8_t* out_blob,
                         const uint32_t* out_off, uint32_t* out_len, uint8_t* status, int nthreads);

/* ---- pinned host memory ---------------------------------------------------
 * Page-lock a host range (e.g. buffet's buffer arena, crates/buffet/src/bufpool/privatepool.rs:94-108)
 * so HPK_PTR_HOST batches inside it DMA directly and their copies overlap the kernels.
 * Returns HPK_E_OK or HPK_E_DEVICE. */
int hpk_host_register(void* ptr, size_t bytes);
int hpk_host_unregister(void* ptr);

/* buffet's buffer arena (crates/buffet/src/bufpool/privatepool.rs:80-108: one anonymous mmap of
 * num_bufs x buf_size, 64Ki x 4 KiB by default there), page-locked when pin != 0, so the frames
 * and literals read into its buffers DMA straight to the device. NULL on failure. */
typedef struct hpk_arena hpk_arena;
hpk_arena* hpk_arena_create(size_t num_bufs, size_t buf_size, int pin);
void* hpk_arena_base(const hpk_arena* arena);
size_t hpk_arena_len(const hpk_arena* arena);
void hpk_arena_destroy(hpk_arena* arena);

/* ---- HPACK header blocks: two-pass decode -----------------------------------------------
 * hpk_hdec mirrors hpack::Decoder (crates/loona-hpack/src/decoder.rs:257-555; header table
 * crates/loona-hpack/src/lib.rs:43-289): one per connection, holding the dynamic table.
 * hpk_hdec_decode_blocks decodes many header blocks at once — block b is
 * blocks[block_off[b] .. block_off[b+1]) for decoder decs[b]; the blocks of one decoder must be
 * in connection order — with every Huffman string of every block decoded in ONE batch: through
 * `ctx` on the GPU, or, when ctx is NULL, by the library's CPU batch path
 * (hpk_decode_batch_cpu). Per block the result equals Decoder::decode_with_cb on the same state:
 * the headers emitted before the first error, and that error with the reference's precedence
 * (decoder.rs:368-450). Results are returned in library-allocated buffers (hpk_blocks_out_free,
 * which keeps the largest freed buffers for the next call instead of returning them to the
 * allocator). With a context the device batch runs while the blocks whose strings are back are
 * applied: a device failure (HPK_E_DEVICE) mid-call leaves the decoders as far as the apply got,
 * and `out` empty. Host threads: up to 16, HPK_HDEC_THREADS overrides (measurements). */
typedef struct hpk_hdec hpk_hdec;

typedef enum hpk_block_error {   /* DecoderError (decoder.rs:237-253) and its nested kinds */
    HPK_BLK_OK = 0,
    HPK_BLK_HEADER_INDEX_OUT_OF_BOUNDS = 1,  /* HeaderIndexOutOfBounds                         */
    HPK_BLK_INT_TOO_MANY_OCTETS = 2,         /* IntegerDecodingError::TooManyOctets           */
    HPK_BLK_INT_VALUE_TOO_LARGE = 3,         /* IntegerDecodingError::ValueTooLarge (unused)  */
    HPK_BLK_INT_NOT_ENOUGH_OCTETS = 4,       /* IntegerDecodingError::NotEnoughOctets         */
    HPK_BLK_INT_INVALID_PREFIX = 5,          /* IntegerDecodingError::InvalidPrefix           */
    HPK_BLK_STR_NOT_ENOUGH_OCTETS = 6,       /* StringDecodingError::NotEnoughOctets          */
    HPK_BLK_STR_HUFFMAN = 7,                 /* StringDecodingError::HuffmanDecoderError(detail = hpk_status) */
    HPK_BLK_INVALID_MAX_DYNAMIC_SIZE = 8,    /* InvalidMaxDynamicSize                          */
    HPK_BLK_SIZE_UPDATE_AT_END = 9           /* SizeUpdateAtEnd                                */
} hpk_block_error;

typedef struct hpk_header {      /* one emitted (name, value), offsets into hpk_blocks_out.arena */
    uint32_t name_off, name_len, value_off, value_len;
} hpk_header;

typedef struct hpk_block_result {
    uint32_t first_header;       /* index into hpk_blocks_out.headers                         */
    uint32_t n_headers;          /* headers emitted (before the error, if any)               */
    int32_t error;               /* hpk_block_error                                           */
    int32_t detail;              /* hpk_status for HPK_BLK_STR_HUFFMAN, else 0                 */
} hpk_block_result;

typedef struct hpk_blocks_out {
    uint8_t* arena;
    size_t arena_len;
    hpk_header* headers;
    size_t n_headers;
    hpk_block_result* blocks;
    uint32_t n_blocks;
} hpk_blocks_out;

hpk_hdec* hpk_hdec_create(void);                                  /* Decoder::new(): max table 4096 */
void hpk_hdec_destroy(hpk_hdec* dec);
int hpk_hdec_set_max_table_size(hpk_hdec* dec, size_t max_size); /* decoder.rs:296-311 */
int hpk_hdec_set_max_allowed_table_size(hpk_hdec* dec, size_t max_allowed); /* decoder.rs:316-318 */
int hpk_hdec_table_size(const hpk_hdec* dec, size_t* size, size_t* entries, size_t* max_size);
int hpk_hdec_decode_blocks(hpk_ctx* ctx, hpk_hdec* const* decs, const uint8_t* blocks, const uint32_t* block_off,
                           uint32_t nblocks, hpk_blocks_out* out);
void hpk_blocks_out_free(hpk_blocks_out* out);

/* ---- HPACK header blocks: the table-free scan on the device -------------------------------
 * hpk_scan_blocks tokenises many header blocks at once — block b is blocks[block_off[b] .. block_off[b+1]) —
 * with no decoder in hand: the batch form of the table-free half of Decoder::decode_with_cb (crates/loona-hpack/
 * src/decoder.rs:368-450; decode_literal :502-527; decode_integer :67-125; decode_string's framing :135-143).
 * Where the fields and strings of a block lie never depends on table state. Per field it gives the kind from
 * the first octet (1xxxxxxx indexed, 7-bit prefix; 01 literal with incremental indexing, 6; 001 size update, 5;
 * 0001 never indexed, 4; 0000 plain, 4), decode_integer's value (at most 5 octets; non-canonical forms are
 * accepted, as there), and for a literal its strings: a name string only when the index is 0, then the value
 * string, each framed against the rest of the block with the length comparison in 64 bits. A block's walk stops
 * at its end or at its first integer or length error, which is recorded in the block's last field with the stage
 * at which the reference would raise it. A string's payload is never read, and nothing outside
 * [blocks, blocks + cap) and of a block nothing outside the block.
 * Outputs: field_off and str_blk_off (nblocks + 1 entries each, exclusive sums: field_off[nblocks] is the field
 * total, str_blk_off[nblocks] the string total); block b's records are fields[field_off[b] .. field_off[b+1])
 * and its strings str_blk_off[b] .. str_blk_off[b+1] of the call's string list. The list is in block order, then
 * field order, name before value; a string is listed only if its prefix and its length check passed, and its
 * window [str_off[s], str_end[s]) is exact: from the first prefix octet to the payload's last byte. str_off and
 * str_end are hpk_decode_strings_packed's inputs as they stand. A string whose framing failed is not listed: its
 * field carries err and err_stage. status[b] is HPK_OK or HPK_BAD_OFFSETS.
 * Capacities: fields_cap (records) and strs_cap (windows) may be any size; cap of each always suffices. Records
 * and windows below the capacities are written and nothing at or past them; both offset arrays and status are
 * complete either way. A synchronous call returns HPK_E_NOSPACE when a total passes its capacity; HPK_E_INVAL
 * wins over HPK_E_NOSPACE. A block whose offsets decrease or pass cap is void: 0 fields, 0 strings,
 * HPK_BAD_OFFSETS, the sticky flag; it voids no other block. cap above HPK_MAX_OFFSET is HPK_E_INVAL.
 * nblocks == 0 writes the two zeros.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC (fields must then be 16-byte aligned: HPK_E_INVAL); or
 * HPK_PTR_HOST, synchronous: the offsets are checked on the host before anything is copied (HPK_E_INVAL, nothing
 * written), the input is staged in one piece into grow-only scratch of the stream's slot, and exactly the written
 * parts come back. Always the launch path: the small-call mode does not answer it.
 * How: a count pass (one lane per block, 256-lane workgroups: field count, string count, status), the length
 * scan over each count array, and an emit pass (one lane per block again, the same walk: each record one 16-byte
 * store). Both passes run the walk of hpk_blkscan.h, so they cannot disagree. Scratch per stream: 8 bytes per
 * block and the scan's tile sums. Cost of a big block: one lane walks a whole block, two dependent byte loads per
 * small field, so a block of many thousands of small fields takes that many load latencies whatever the rest of
 * the batch does; blocks are not split. */
typedef enum hpk_field_kind { HPK_FIELD_INDEXED = 0, HPK_FIELD_LIT_INCR = 1, HPK_FIELD_SIZE_UPDATE = 2,
                              HPK_FIELD_LIT_NEVER = 3, HPK_FIELD_LIT_PLAIN = 4 } hpk_field_kind;
typedef struct hpk_field {   /* 16 bytes */
    uint32_t index;     /* header index / name index / new max size (decode_integer's value) */
    uint32_t str;       /* index in the call's string list of this field's first listed string */
    uint8_t  kind;      /* hpk_field_kind */
    uint8_t  nstr;      /* strings of this field in the list: 0, 1 or 2 (name first) */
    uint8_t  err;       /* hpk_block_error the scan found in this field, else 0; only a block's last field has one */
    uint8_t  err_stage; /* 0 index, 1 name, 2 value: where the reference would raise err */
    uint32_t at;        /* offset of the field's first octet in the blob */
} hpk_field;

int hpk_scan_blocks(hpk_ctx* ctx, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                    hpk_field* fields, size_t fields_cap, uint32_t* field_off,
                    uint32_t* str_off, uint32_t* str_end, size_t strs_cap, uint32_t* str_blk_off,
                    uint8_t* status, int flags);

/* Where hpk_hdec_decode_blocks (and hpk_h2_read_frames, which calls it) scans a context's blocks.
 * HPK_BLOCK_SCAN_HOST (the default): the two-pass path above. HPK_BLOCK_SCAN_DEVICE (opt-in; calls without a
 * context are not affected): the blocks and block_off are uploaded once as they are; hpk_scan_blocks' kernels
 * tokenise them; the two totals are read back; hpk_decode_strings_packed's pipeline decodes every listed string,
 * raw and Huffman alike; the field records, field_off, the strings' out_off / out_len / status and the packed
 * string bytes come back into the context's page-locked area; then the host applies the records in order per
 * decoder, every string's bytes taken from the packed bytes. Results and decoder states equal the default
 * path's exactly. The apply starts only when everything is back, so a device failure on this path leaves every
 * decoder untouched. Known cost: raw strings travel to the device and back inside the packed bytes.
 * Scratch per stream: the blocks, 16 bytes per field, 17 bytes per string and 12 per block, beside
 * hpk_decode_strings_packed's. */
#define HPK_BLOCK_SCAN_HOST 0    /* the default: the host scan */
#define HPK_BLOCK_SCAN_DEVICE 1
int hpk_ctx_set_block_scan(hpk_ctx* ctx, int kind);

/* ---- HPACK header blocks: the apply on the device ------------------------------------------
 * hpk_apply_blocks applies the field records of many header blocks, in order, against each connection's dynamic
 * table: the batch form of the table-dependent half of Decoder::decode_with_cb (crates/loona-hpack/src/decoder.rs:
 * 368-450: the indexed lookup :387-392, the literals :393-430 with decode_literal :502-527, update_max_dynamic_size
 * :537-554, SizeUpdateAtEnd :445-447) and of the table itself (crates/loona-hpack/
 * src/lib.rs: DynamicTable :43-164 with add_header :108-122 and consolidate_table :124-142, get_from_table :228-255),
 * the counterpart of the table-free half that hpk_scan_blocks covers. Its inputs are hpk_scan_blocks' fields and
 * field_off and, for the scan's string list, hpk_decode_strings_packed's out_off / out_len / status.
 * The arena. The apply never touches a byte of any string: names and values are references. Every offset is a u32
 * into ONE arena that the caller defines and the call never reads: the static text (hpk_static_table) lies at
 * static_base, string s of the list at str_base + str_out_off[s], and the entries of the tables carried in wherever
 * the caller's tab_ent records say. An emitted header is an hpk_header whose offsets point into that arena, and so
 * is an entry of a table that comes back. static_base + the static text's length must not pass 2^32 (HPK_E_INVAL).
 * Decoders. Decoder d applies blocks dec_blk[dec_blk_off[d] .. dec_blk_off[d+1]) in that order (a connection's
 * blocks in connection order; the lists of different decoders may interleave in any way, and a block belongs to at
 * most one list) against tabs[d]: its entries are tab_ent[ent .. ent + count), newest first, of cap records it may
 * grow into. count, size and max_size come back updated with the entries in the same layout.
 * Results. results[b] is exactly what hpk_hdec_decode_blocks gives for block b on the same state: n_headers before
 * the first error, error and detail with the reference's precedence; first_header = field_off[b], block b's headers
 * are headers[field_off[b] .. field_off[b] + n_headers) (a field emits at most one header, so the field total is the
 * capacity that always suffices and there is no count pass), and records of headers that no block covers are not
 * written. results of a block in no list is zero. ndecs == 0 or nblocks == 0 does nothing but zero results.
 * Deferral. On the device a decoder's table is a ring of ring_entries records (hpk_test_blkapply_geometry). With
 * lim = min(ring_entries, tabs[d].cap), a block is deferred, before it touches the table, when the decoder's
 * max_size at the call's start exceeds 32 * lim (or its count exceeds lim), or when any size update record of the
 * block carries a value above 32 * lim. Every later block of the list is deferred too: result HPK_BLK_DEFERRED with
 * 0 headers, tabs[d] as it was after the last applied block, and tabs[d].applied the number of blocks applied: where
 * the caller takes over (hpk_hdec_decode_blocks applies them on the host). An entry takes at least 32 octets of the
 * size, so the live count never passes lim otherwise.
 * Bad inputs (the rule for device pointers, as hpk_decode_batch). A decoder is void when its ent + cap passes
 * tab_ent_cap or its count its cap; when its list's offsets decrease or pass dec_blk_off[ndecs]; when a listed block
 * index is >= nblocks; when a listed block's field_off decreases or passes headers_cap (fields and headers are
 * arrays of headers_cap records); when a field's str + nstr passes nstrs; or when str_base + out_off + out_len of a
 * listed string passes 2^32. All blocks of a void decoder are HPK_BLK_DEFERRED, its applied is 0 and its table
 * untouched; the sticky flag is set (a synchronous call then returns HPK_E_INVAL). Nothing outside the arrays'
 * stated sizes is read or written. If field_off[nblocks] > headers_cap a synchronous call returns HPK_E_NOSPACE
 * (HPK_E_INVAL wins over it); after HPK_ASYNC the caller compares.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC (anything else is HPK_E_INVAL); fields, headers and tab_ent must be
 * 16-byte aligned (HPK_E_INVAL). On the context's stream; no scratch; always the launch path: the small-call mode
 * does not answer it.
 * How: one kernel, one wave per decoder (hpk_blkapply.hip). A lane-parallel look over the decoder's records finds
 * the bad inputs and the deferring size updates; then per chunk of chunk_fields records the lanes stage everything
 * that does not depend on the table (one 16-byte load each and the strings' three arrays), the wave resolves the
 * records in order against the ring in LDS, and the chunk's headers go out as one 16-byte store per lane. */
typedef struct hpk_dtab {   /* one decoder's dynamic table for hpk_apply_blocks; 32 bytes */
    uint32_t ent, cap;      /* its entries are tab_ent[ent .. ent + cap); entries 0 .. count-1, newest first */
    uint32_t count, size;   /* in/out: entries, and the RFC 7541 §4.1 size (sum of name + value + 32) */
    uint32_t max_size;      /* in/out: the current limit (SizeUpdate changes it) */
    uint32_t max_allowed;   /* in: the SETTINGS limit (decoder.rs:316-318), HPK_DTAB_NO_LIMIT = none set */
    uint32_t applied;       /* out: how many blocks of this decoder's list were applied (the rest are deferred) */
    uint32_t reserved;
} hpk_dtab;
#define HPK_DTAB_NO_LIMIT 0xFFFFFFFFu
#define HPK_BLK_DEFERRED 10 /* hpk_block_result.error, hpk_apply_blocks only: not applied, the decoder untouched from here on */

int hpk_apply_blocks(hpk_ctx* ctx,
        const hpk_field* fields, const uint32_t* field_off, uint32_t nblocks,        /* hpk_scan_blocks' outputs */
        const uint32_t* str_out_off, const uint32_t* str_out_len, const uint8_t* str_status, uint32_t nstrs,
                                                               /* hpk_decode_strings_packed's, for the scan's string list */
        uint32_t str_base, uint32_t static_base,               /* where the packed strings / the static text lie in the arena */
        const uint32_t* dec_blk_off, const uint32_t* dec_blk, uint32_t ndecs,
                                  /* decoder d's blocks, in connection order: dec_blk[dec_blk_off[d] .. dec_blk_off[d+1]) */
        hpk_dtab* tabs, hpk_header* tab_ent, size_t tab_ent_cap,
        hpk_header* headers, size_t headers_cap, hpk_block_result* results, int flags);

/* RFC 7541 App. A as the kernel sees it (the reference's STATIC_TABLE, crates/loona-hpack/src/lib.rs:293-356): the
   61 entries' names and values end to end, and 61 hpk_header records with offsets relative to the text's start.
   Host memory of the library, valid for the process. Any of the three pointers may be NULL. */
int hpk_static_table(const uint8_t** text, size_t* text_len, const hpk_header** entries);

/* Where hpk_hdec_decode_blocks (and hpk_h2_read_frames, which calls it) applies a context's blocks.
 * HPK_BLOCK_APPLY_HOST (the default): on the host, after the scan hpk_ctx_set_block_scan selects.
 * HPK_BLOCK_APPLY_DEVICE (opt-in; calls without a context are not affected) selects the whole device pipeline,
 * whatever hpk_ctx_set_block_scan says: the blocks are grouped by decoder on the host; every distinct decoder's live
 * entries and their bytes go up with the blocks as hpk_dtab / hpk_header records and a blob of prior bytes; the
 * device-scan path's steps run as they are (count, scans, totals, emit, strings); hpk_apply_blocks' kernel applies;
 * results and tabs come back. If no block was deferred, the header records, the tables' final entries and exactly
 * the packed bytes come back: out->arena is the static text, then the prior bytes, then the packed strings;
 * out->headers is the field-total array (out->n_headers its length, first_header = field_off[b], records that no
 * block covers zero); and every decoder's table is rebuilt from its final entries' bytes in that arena. If any
 * block was deferred (or a decoder's max_size exceeds 32 * ring_entries, or its count ring_entries, before the call,
 * which the host sees without the device), the field records come back instead and the device-scan path's host apply
 * runs for the whole call: no decoder has been touched until then, so nothing is merged. Results and decoder states
 * equal the default path's exactly. Nothing is written to a decoder before everything is back, so a device failure on
 * this path leaves every decoder untouched. */
#define HPK_BLOCK_APPLY_HOST 0    /* the default */
#define HPK_BLOCK_APPLY_DEVICE 1
int hpk_ctx_set_block_apply(hpk_ctx* ctx, int kind);
/* Testing only: the block apply's geometry (hpk_apply_blocks): the records of a decoder's ring in LDS, the field
 * records a wave stages at a time, and the decoders per workgroup (one wave each). The tests place their cases
 * relative to these. */
int hpk_test_blkapply_geometry(uint32_t* ring_entries, uint32_t* chunk_fields, uint32_t* wg_decoders);

/* ---- HTTP/2 framing in front of the block decoder ------------------------
 * hpk_h2conn is one connection's header-reading state: its HPACK decoder and a HEADERS block still
 * waiting for CONTINUATION frames. hpk_h2_read_frames takes the bytes received on many
 * connections — connection c's are bytes[off[c] .. off[c+1]), whole frames (RFC 9113 §4.1:
 * 24-bit length, type, flags, 31-bit stream id) followed by at most one incomplete frame — and
 * does what the reference does per connection: the deframer's length check and padding removal
 * (crates/loona/src/h2/server.rs:290-390; Frame::parse crates/loona-h2/src/lib.rs:397-411), the
 * HEADERS priority block (server.rs:895-911), CONTINUATION gathering until END_HEADERS and the
 * concatenation (read_headers, server.rs:1349-1417, 1619-1638; flags lib.rs:139-168). Every
 * complete header block of every connection is then decoded by ONE hpk_hdec_decode_blocks call
 * (one Huffman batch through ctx, or the CPU path when ctx is NULL). Other frame types are
 * skipped. The first connection error stops the connection for this and all later calls (the
 * reference sends GOAWAY); an HPACK decoding error is HPK_H2_COMPRESSION_ERROR and the
 * connection's later blocks of the same call are marked skipped. */
typedef struct hpk_h2conn hpk_h2conn;

typedef enum hpk_h2_error {                   /* H2ConnectionError (crates/loona/src/h2/types.rs:300-370) */
    HPK_H2_OK = 0,
    HPK_H2_FRAME_TOO_LARGE = 1,               /* FrameTooLarge                 -> FRAME_SIZE_ERROR  */
    HPK_H2_PADDED_FRAME_EMPTY = 2,            /* PaddedFrameEmpty              -> FRAME_SIZE_ERROR  */
    HPK_H2_PADDED_FRAME_TOO_SHORT = 3,        /* PaddedFrameTooShort           -> PROTOCOL_ERROR    */
    HPK_H2_PRIORITY_PARSE = 4,                /* ReadAndParse(PrioritySpec)    -> PROTOCOL_ERROR    */
    HPK_H2_HEADERS_INVALID_PRIORITY = 5,      /* HeadersInvalidPriority        -> PROTOCOL_ERROR    */
    HPK_H2_EXPECTED_CONTINUATION_FRAME = 6,   /* ExpectedContinuationFrame     -> PROTOCOL_ERROR    */
    HPK_H2_EXPECTED_CONTINUATION_FOR_STREAM = 7, /* ExpectedContinuationForStream -> PROTOCOL_ERROR */
    HPK_H2_UNEXPECTED_CONTINUATION_FRAME = 8, /* UnexpectedContinuationFrame   -> PROTOCOL_ERROR    */
    HPK_H2_COMPRESSION_ERROR = 9              /* HpackDecodingError            -> COMPRESSION_ERROR */
} hpk_h2_error;

typedef struct hpk_h2_block {   /* one complete header block, in connection order */
    uint32_t conn;              /* index of its connection in the call                        */
    uint32_t stream_id;
    uint32_t end_stream;        /* the HEADERS frame's END_STREAM flag                        */
    uint32_t skipped;           /* 1: after a COMPRESSION_ERROR on its connection: not decoded */
} hpk_h2_block;

typedef struct hpk_h2_out {
    hpk_blocks_out hb;          /* hb.blocks[i] / headers of blocks[i] (hpk_hdec_decode_blocks) */
    hpk_h2_block* blocks;       /* hb.n_blocks entries                                          */
    int32_t* conn_error;        /* per connection: hpk_h2_error (sticky)                        */
    uint32_t* conn_consumed;    /* per connection: bytes of whole frames consumed (the rest is an
                                   incomplete frame: pass it again with more bytes)             */
    uint32_t n_conns;
} hpk_h2_out;

hpk_h2conn* hpk_h2conn_create(void);
void hpk_h2conn_destroy(hpk_h2conn* conn);
hpk_hdec* hpk_h2conn_decoder(hpk_h2conn* conn);                      /* its HPACK decoder */
int hpk_h2conn_set_max_frame_size(hpk_h2conn* conn, uint32_t max);  /* our SETTINGS_MAX_FRAME_SIZE */
int hpk_h2conn_error(const hpk_h2conn* conn);                       /* hpk_h2_error */
int hpk_h2_error_code(int h2_error);                                /* RFC 9113 §7 code for GOAWAY */
int hpk_h2_read_frames(hpk_ctx* ctx, hpk_h2conn* const* conns, const uint8_t* bytes, const uint32_t* off,
                       uint32_t nconn, hpk_h2_out* out);
void hpk_h2_out_free(hpk_h2_out* out);

/* ---- HTTP/2 framing: the frame scan on the device ------------------------------------------
 * hpk_scan_frames is step 1 of hpk_h2_read_frames on many connections at once, with no decoder in hand:
 * connection c's bytes are bytes[off[c] .. off[c+1]) and its frame state conns[c]. Per connection it does, frame by
 * frame, what the reference does: the deframer's length check (a length above max_frame_size is FrameTooLarge even
 * before the payload has arrived, and that frame is not consumed: crates/loona/src/h2/server.rs:318-325), an
 * incomplete frame ends the walk unconsumed and without an error, the padding of DATA and HEADERS frames goes
 * (server.rs:356-382: PaddedFrameEmpty, PaddedFrameTooShort; PADDED on any other type is not padding), a pending
 * block takes only CONTINUATION frames of its stream, the stream id compared before the type (read_headers,
 * server.rs:1376-1417: :1391-1397, then :1399-1408), a CONTINUATION with no block pending is
 * UnexpectedContinuationFrame (server.rs:1299-1303), frames other than HEADERS are skipped, and a HEADERS frame's
 * priority block goes (server.rs:895-911: fewer than 5 octets ReadAndParse(PrioritySpec), a 31-bit dependency equal
 * to the stream id HeadersInvalidPriority). A stream id's reserved bit is masked (Frame::parse,
 * crates/loona-h2/src/lib.rs:397-411). A connection whose error is set on entry consumes nothing. A frame that
 * raises an error other than FrameTooLarge is consumed.
 * Outputs. blocks: one hpk_fblock per header block completed in this call, in connection order, then frame order
 * (hpk_h2_read_frames' block order); connection c's are conn_blk_off[c] .. conn_blk_off[c+1]. Block b's bytes are
 * the fragments frag[blocks[b].frag .. + blocks[b].nfrag) of the closed list, fragment g being bytes[frag_off[g] ..
 * frag_off[g] + frag_len[g]): the closed list holds only fragments of completed blocks, in order, so the blocks tile
 * it. A connection that enters pending has its carry window [carry_off, carry_off + carry_len) as fragment 0 of that
 * block, even when the window is empty (and with its error set on entry: the block then stays open). The fragments
 * of a block still pending when the walk ends (at the connection's end, or at an error) go to the open list,
 * connection c's at conn_open_off[c] .. conn_open_off[c+1]: their bytes, in order, are what the caller must keep as
 * the next call's carry. The three offset arrays have nconn + 1 entries and are exclusive sums. Lengths are exact:
 * padding, the pad-length octet and the priority block are excluded; zero-length fragments are listed. After an
 * error a connection's walk stops: its earlier completed blocks stay listed. conns[c] comes back with error,
 * pending, pend_stream, consumed and status updated; max_frame_size and the carry window are the caller's.
 * Capacities: blocks_cap (records), frags_cap and opens_cap (windows) may be any size; (off[nconn] - off[0]) / 9
 * blocks and (off[nconn] - off[0]) / 9 + nconn fragments of either list always suffice. Records and windows below
 * the capacities are written and nothing at or past them; the offset arrays and the states are complete either way.
 * A synchronous call returns HPK_E_NOSPACE when a total passes its capacity; HPK_E_INVAL wins over HPK_E_NOSPACE.
 * A connection whose offsets decrease or pass cap, or whose carry window passes cap while it is pending, is void: 0
 * blocks, 0 fragments, status HPK_BAD_OFFSETS and nothing else of its state touched, the sticky flag; it voids no
 * other connection. cap above HPK_MAX_OFFSET is HPK_E_INVAL. nconn == 0 writes the three zeros. Nothing outside
 * [bytes, bytes + cap) is read, and of a connection nothing outside its range (the carry window is listed, not read).
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC (conns and blocks must then be 16-byte aligned: HPK_E_INVAL); or
 * HPK_PTR_HOST, synchronous: the offsets and carry windows are checked on the host before anything is copied
 * (HPK_E_INVAL, nothing written; the offsets must then be non-decreasing as a whole), the input is staged in one
 * piece into grow-only scratch of the stream's slot, and exactly the written parts come back. Always the launch
 * path: the small-call mode does not answer it.
 * How: a count pass (one lane per connection, 256-lane workgroups: blocks, closed and open fragments), the length
 * scan over each count array, and an emit pass (one lane per connection again, the same walk: each block record one
 * 16-byte store, the state two). Both passes run the walk of hpk_frmscan.h, so they cannot disagree; the count pass
 * does not write the state. Scratch per stream: 12 bytes per connection and the scan's tile sums. Cost of a long
 * connection: one lane walks a whole connection, two dependent byte loads per frame, so a connection of many
 * thousands of small frames takes that many load latencies whatever the rest of the call does. */
typedef struct hpk_fconn {      /* one connection's frame state; 32 bytes, 16-byte aligned for device calls */
    uint32_t max_frame_size;    /* in */
    int32_t  error;             /* in/out: hpk_h2_error, sticky (never COMPRESSION_ERROR: the scan decodes nothing) */
    uint32_t pending;           /* in/out: 1 = a HEADERS block waits for CONTINUATION */
    uint32_t pend_stream;       /* in/out: its stream id, bit 31 = the HEADERS frame's END_STREAM */
    uint32_t carry_off, carry_len; /* in: where in `bytes` the caller put the fragment bytes that block has so far */
    uint32_t consumed;          /* out: bytes of whole frames consumed */
    uint32_t status;            /* out: HPK_OK or HPK_BAD_OFFSETS */
} hpk_fconn;
typedef struct hpk_fblock { uint32_t conn, stream_id /* bit 31 END_STREAM */, frag, nfrag; } hpk_fblock; /* 16 bytes */

int hpk_scan_frames(hpk_ctx* ctx, const uint8_t* bytes, size_t cap, const uint32_t* off, uint32_t nconn, hpk_fconn* conns,
                    hpk_fblock* blocks, size_t blocks_cap, uint32_t* conn_blk_off,
                    uint32_t* frag_off, uint32_t* frag_len, size_t frags_cap, uint32_t* conn_frag_off,
                    uint32_t* open_off, uint32_t* open_len, size_t opens_cap, uint32_t* conn_open_off, int flags);

/* hpk_frame_blocks concatenates the scan's closed fragments into header blocks: the ordered pack (hpk_pack_batch's
 * kernels) of bytes[frag_off[g] .. + frag_len[g]), g < nfrags, into out_blob, then block_off[b] = the packed offset
 * of fragment blocks[b].frag and block_off[nblocks] = the packed total: read_headers' concatenation
 * (server.rs:1619-1638). (out_blob, block_off) are hpk_scan_blocks' inputs as they stand. Capacity, HPK_E_NOSPACE
 * and bad fragment windows as hpk_pack_batch. A block record whose frag passes nfrags is read as nfrags, and one
 * whose frag goes below its predecessor's as its predecessor's; either sets the sticky flag (HPK_E_INVAL from a
 * synchronous call). Device pointers only (HPK_PTR_DEVICE, optionally HPK_ASYNC); blocks 16-byte aligned. Scratch
 * per stream: nfrags + 1 dwords and the pack's tile sums. */
int hpk_frame_blocks(hpk_ctx* ctx, const uint8_t* bytes, size_t cap, const uint32_t* frag_off, const uint32_t* frag_len,
                     uint32_t nfrags, const hpk_fblock* blocks, uint32_t nblocks,
                     uint8_t* out_blob, size_t out_cap, uint32_t* block_off, int flags);

/* Where hpk_h2_read_frames does its framing (its step 1). HPK_FRAME_SCAN_HOST (the default): on the host,
 * connection by connection. HPK_FRAME_SCAN_DEVICE (opt-in; calls without a context are not affected): the call's
 * bytes go up once, with every pending connection's held fragment bytes behind them as its carry, and the states;
 * hpk_scan_frames' steps and hpk_frame_blocks' steps run; the block records, block_off, the states, the open windows
 * and the gathered block bytes come back; connections with open fragments rebuild their held bytes from those
 * windows; then the block decode and the error pass run as on the default path. Results, conn_error, conn_consumed
 * and every connection's state equal the default path's exactly. Nothing is written to a connection before
 * everything is back, so a device failure on this path leaves every connection untouched. Known cost: the blocks
 * come back to the host and go up again when a device block path is selected (hpk_ctx_set_block_scan,
 * hpk_ctx_set_block_apply); keeping them on the device for the block scan is not done. The call's bytes and the
 * carries together must not pass HPK_MAX_OFFSET (HPK_E_INVAL). */
#define HPK_FRAME_SCAN_HOST 0    /* the default: the host framing */
#define HPK_FRAME_SCAN_DEVICE 1
int hpk_ctx_set_frame_scan(hpk_ctx* ctx, int kind);

/* ---- HTTP/2 framing: the frame write on the device ------------------------------------------
 * hpk_write_frames turns header blocks into what goes on the wire, the mirror of hpk_scan_frames + hpk_frame_blocks:
 * block b is blocks[block_off[b] .. block_off[b+1]) with length L, and M = max_frame[b] is the peer's
 * SETTINGS_MAX_FRAME_SIZE for that block's connection. Its wire form is the reference's loop in send_data_maybe
 * (crates/loona/src/h2/server.rs:470-508): while the piece left is strictly longer than M, a frame of M octets with
 * flags 0, the first such frame HEADERS (0x1), the later ones CONTINUATION (0x9); then the last piece, of 1..M octets
 * (or of 0 when L = 0: a HEADERS frame of length 0), with END_HEADERS (0x4). So there are max(1, ceil(L / M)) frames,
 * L = k M gives k frames with no empty CONTINUATION behind them, and the wire length is L + 9 frames (computed in 64
 * bits). Each frame's header is Frame::write_into's (crates/loona-h2/src/lib.rs:413-422): the 24-bit big-endian
 * length, the type, the flags, and the 31-bit stream id big-endian with the reserved bit 0. stream_id[b]'s bit 31
 * puts END_STREAM (0x1) into the HEADERS frame's flags, never into a CONTINUATION's: hpk_fblock's convention, so a
 * scanned block can be written back as it stands (the reference sets END_STREAM on DATA; here it is the caller's).
 * Outputs. wire_off (nblocks + 1 entries) is the exclusive sum of the wire lengths; block b's frames are
 * out_blob[wire_off[b] .. wire_off[b+1]) with no gap; status[b] is HPK_OK or HPK_BAD_OFFSETS. nblocks == 0 writes
 * wire_off[0] = 0.
 * out_cap may be any size: the octets below min(wire_off[n], out_cap) are written, nothing at or past that point nor
 * outside [out_blob, out_blob + out_cap), and wire_off and status are complete either way. If wire_off[n] > out_cap
 * a synchronous call returns HPK_E_NOSPACE; after HPK_ASYNC the caller compares. HPK_E_INVAL wins over it.
 * Void blocks (device pointers): a block whose offsets decrease or pass cap, or whose max_frame is 0 (the reference's
 * loop never ends) or above 0xFFFFFF (the length field has 24 bits), contributes 0 octets, gets HPK_BAD_OFFSETS and
 * sets the sticky flag (HPK_E_INVAL from a synchronous call); it voids no other block. A wire total past
 * HPK_MAX_OFFSET voids every block, zeroes every wire_off and writes no octet. cap above HPK_MAX_OFFSET is
 * HPK_E_INVAL. Nothing outside [blocks, blocks + cap) is read beyond the aligned dwords that hold it.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC; or HPK_PTR_HOST, synchronous: the offsets (non-decreasing as a
 * whole, within cap) and the frame sizes are checked on the host before anything is copied (HPK_E_INVAL, nothing
 * written), the input is staged in one piece into grow-only scratch of the stream's slot, and exactly
 * min(wire_off[n], out_cap) octets come back. A total past HPK_MAX_OFFSET is then HPK_E_INVAL with every wire_off 0
 * and every status HPK_BAD_OFFSETS. Always the launch path: the small-call mode does not answer it.
 * How: the length scan over the blocks' wire lengths (64-bit tile sums), an elementwise status pass, and hpk_frmwrite,
 * destination-centric like the ordered pack: a thread makes one aligned 16-byte chunk of the wire; position p of a
 * block lies in frame p / (M + 9) at r = p % (M + 9), a header octet made in registers when r < 9, else source octet
 * block_off[b] + f M + r - 9. Scratch per stream: the scan's tile sums.
 * hpk_write_frames_cpu is the same on the host alone, with the host-pointer rules, and gives the same octets. */
int hpk_write_frames(hpk_ctx* ctx, const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                     const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap,
                     uint32_t* wire_off, uint8_t* status, int flags);
int hpk_write_frames_cpu(const uint8_t* blocks, size_t cap, const uint32_t* block_off, uint32_t nblocks,
                         const uint32_t* stream_id, const uint32_t* max_frame, uint8_t* out_blob, size_t out_cap,
                         uint32_t* wire_off, uint8_t* status);

/* Where hpk_h2_write_headers (below) frames its blocks. HPK_FRAME_WRITE_HOST (the default, and always without a
 * context): hpk_write_frames_cpu's code. HPK_FRAME_WRITE_DEVICE (opt-in): hpk_write_frames with host pointers. */
#define HPK_FRAME_WRITE_HOST 0    /* the default: the host framing */
#define HPK_FRAME_WRITE_DEVICE 1
int hpk_ctx_set_frame_write(hpk_ctx* ctx, int kind);
/* Testing only: hpk_h2_write_headers calls on this context that the device framing answered. */
uint64_t hpk_test_frame_write_calls(const hpk_ctx* ctx);

/* ---- HPACK header blocks: encode (the response path) ----------------------
 * hpk_henc mirrors hpack::Encoder (crates/loona-hpack/src/encoder.rs:172-335): one per
 * connection, holding the dynamic table, with the reference's single strategy (a header found
 * whole in the table -> indexed; name found -> indexed name + literal value, not indexed; else a
 * literal name + value with incremental indexing). String literals (encoder.rs:299-307): with
 * huffman == 0 always raw, byte-identical to the reference; with huffman == 1 the H-bit form
 * (RFC 7541 §5.2) whenever its Huffman encoding is strictly shorter than the raw bytes. */
typedef struct hpk_henc hpk_henc;

hpk_henc* hpk_henc_create(int huffman);                           /* Encoder::new(): max table 4096 */
void hpk_henc_destroy(hpk_henc* enc);
int hpk_henc_set_max_table_size(hpk_henc* enc, size_t max_size); /* encoder.rs:193-197 */
int hpk_henc_table_size(const hpk_henc* enc, size_t* size, size_t* entries, size_t* max_size); /* as hpk_hdec_table_size */
/* Encoder::encode (encoder.rs:210-234) of n headers: header j's name is
 * fields[field_off[2j] .. field_off[2j+1]) and its value fields[field_off[2j+1] .. field_off[2j+2]).
 * Writes the block into out[0 .. cap) and its length to *out_len. Returns HPK_E_OK; HPK_E_NOSPACE
 * with *out_len = the size needed and the encoder state unchanged; HPK_E_INVAL on bad arguments. */
int hpk_henc_encode(hpk_henc* enc, const uint8_t* fields, const uint32_t* field_off, size_t n_headers, uint8_t* out,
                    size_t cap, size_t* out_len);

/* Many responses' header blocks at once: block b encodes headers [hdr_off[b], hdr_off[b+1]) (header j
 * as in hpk_henc_encode) with encoder encs[b]; the blocks of one encoder are encoded in list order.
 * The table logic runs on the host (hpk_ctx_set_block_plan moves it to the device, opt-in). With a ctx and at least one non-empty string of a Huffman-coding
 * encoder, every representation of every block goes through ONE hpk_encode_strings_packed call on ctx
 * (HPK_PTR_HOST): octets the host has made final as HPK_STR_VERBATIM, a string as HPK_STR_AUTO if its
 * encoder Huffman-codes, else HPK_STR_RAW, and the call's output is the blocks end to end. Otherwise
 * (ctx NULL: the library's CPU batch path; or nothing to Huffman-code) the blocks are assembled on the
 * host. Either way the H-bit form is used where strictly shorter and the bytes equal hpk_henc_encode's
 * block by block. Results in
 * library-allocated buffers: block b is bytes[block_off[b] .. block_off[b+1]). */
typedef struct hpk_henc_out {
    uint8_t* bytes;
    size_t len;
    uint32_t* block_off;
    uint32_t n_blocks;
} hpk_henc_out;
int hpk_henc_encode_blocks(hpk_ctx* ctx, hpk_henc* const* encs, const uint8_t* fields, const uint32_t* field_off,
                           const uint32_t* hdr_off, uint32_t nblocks, hpk_henc_out* out);
void hpk_henc_out_free(hpk_henc_out* out);
/* A failed hpk_henc_encode_blocks (any negative return) leaves every encoder's dynamic table as it
 * was before the call, as a failed hpk_henc_encode does; the blocks are then not sent at all.
 * Testing only: the calling thread's next n Huffman batches inside hpk_henc_encode_blocks fail
 * with HPK_E_DEVICE (n = 0 clears it), so that guarantee can be checked without a device fault. The
 * device frame scan of hpk_h2_read_frames (HPK_FRAME_SCAN_DEVICE) counts as one such batch: it fails
 * the same way before it touches the device, and every connection stays as it was. */
void hpk_test_fail_batches(int n);

/* The block encoder and the framing in one call: what a server writes for many responses' headers
 * (send_data_maybe's header loop, crates/loona/src/h2/server.rs:470-508, behind Encoder::encode). max_frame is
 * validated before anything else (an entry of 0 or above 0xFFFFFF: HPK_E_INVAL, the encoders untouched);
 * hpk_henc_encode_blocks runs as the context selects it; block b's bytes are then framed for stream_id[b] (bit 31 =
 * END_STREAM) and max_frame[b] as hpk_write_frames frames them. out->bytes are the wire octets and out->block_off
 * (nblocks + 1 entries) is wire_off. The framing is on the host by default and without a context;
 * hpk_ctx_set_frame_write(ctx, HPK_FRAME_WRITE_DEVICE) selects hpk_write_frames with host pointers for that step.
 * By then the encoders' tables are committed, so a failure of the device framing, real or injected, is answered by
 * the host framing and the call succeeds: hpk_test_fail_batches counts the device framing as one batch (use raw
 * encoders, so that no Huffman batch takes the count first), and hpk_test_frame_write_calls tells which path
 * answered. A wire total past HPK_MAX_OFFSET is HPK_E_INVAL with the encoders advanced (4 GiB of headers in one
 * call). Free the result with hpk_henc_out_free. */
int hpk_h2_write_headers(hpk_ctx* ctx, hpk_henc* const* encs, const uint8_t* fields, const uint32_t* field_off,
                         const uint32_t* hdr_off, uint32_t nblocks, const uint32_t* stream_id, const uint32_t* max_frame,
                         hpk_henc_out* out);

/* ---- HPACK header blocks: the encoder's table half on the device ---------------------------
 * hpk_plan_blocks is the batch form of Encoder::encode (crates/loona-hpack/src/encoder.rs:210-264) without the
 * string coding, the mirror of hpk_apply_blocks: for many encoders at once, in order per encoder, each header gets
 * the representation the reference's single strategy picks (HeaderTable::find_header, crates/loona-hpack/src/
 * lib.rs:261-288), the table is updated (add_header / consolidate_table, lib.rs:108-142), and the header is written
 * out as up to three items that hpk_pack_batch and hpk_encode_strings_packed take as they stand.
 * The arena. The plan reads string bytes, so there is ONE device blob `arena` of arena_cap bytes (above
 * HPK_MAX_OFFSET: HPK_E_INVAL): the static text (hpk_static_table) at static_base; the call's names and values end
 * to end at fields_base, header j's name arena[fields_base + field_off[2j] .. fields_base + field_off[2j+1]) and its
 * value the next span (hpk_henc_encode's layout; field_off has 2 hdrs_cap + 1 entries); the prefix area at
 * prefix_base, 4 bytes per header, the only part of the arena the call writes (prefix_base and arena + prefix_base
 * multiples of 4, prefix_base + 4 hdrs_cap within arena_cap, static_base + the static text within arena_cap: else
 * HPK_E_INVAL); and the bytes of the tables carried in wherever their tab_ent records say. Every reference is a
 * (u32 offset, u32 length) pair into the arena; a table entry is an hpk_header, exactly as in hpk_apply_blocks.
 * Encoders. Encoder e plans blocks enc_blk[enc_blk_off[e] .. enc_blk_off[e+1]) in that order; block b is headers
 * [hdr_off[b], hdr_off[b+1]). The lists may interleave in any way, and a block belongs to at most one list.
 * Encoder e works against tabs[e], an hpk_dtab as hpk_apply_blocks takes it: max_allowed is ignored; size must be the sum of name + value + 32
 * over the count entries carried in (the call trusts it: a size that understates them comes back as a wrong table,
 * though nothing outside the stated sizes is touched); count, size,
 * max_size and the entries come back in the same layout (an inserted entry refers to the header's own bytes in the
 * fields region); applied is the number of blocks planned. enc_flags[e] bit 0: the encoder Huffman-codes, its
 * strings get HPK_STR_AUTO, otherwise HPK_STR_RAW.
 * Per header. find_header runs over the static, then the dynamic entries, newest first: the lowest index whose name
 * and value both match, else the highest index whose name matches (the reference's last name match: ":method PUT"
 * gives 3). Then HPK_PLAN_INDEXED: the index as a 7-bit-prefix integer with 0x80. HPK_PLAN_NAME_INDEXED: the index
 * as a 4-bit-prefix integer with 0x00, then the value string; the table is not touched. HPK_PLAN_NEW_NAME: 0x40, the
 * name string, the value string, then add_header: an entry above max_size empties the table and adds nothing; sizes
 * are summed in 64 bits.
 * Outputs. reps[j] is header j's hpk_hrep. Each header has three item slots, 3j to 3j+2 of item_off / item_len /
 * item_policy (3 hdrs_cap entries each): slot 0 is the prefix octets, written at arena[prefix_base + 4j ..) as one
 * dword, policy HPK_STR_VERBATIM (3 octets at most for any index the ring allows); then the strings the kind needs,
 * with the encoder's policy; an unused slot has length 0 under HPK_STR_VERBATIM and so emits nothing. A header emits
 * at most three items, so 3 hdrs_cap is the capacity that always suffices: no count pass and no scan. With the items
 * packed (hpk_pack_batch: arena, item_off, item_len) and coded (hpk_encode_strings_packed with item_policy), block
 * b's bytes are out_off[3 hdr_off[b]] .. out_off[3 hdr_off[b+1]] of the strings call. Headers of a block in no list,
 * of a deferred or of a void encoder keep the defaults the first pass writes for all hdrs_cap headers: kind
 * HPK_PLAN_NONE and three empty verbatim slots. nencs == 0 or nblocks == 0 only writes the defaults.
 * Deferral, hpk_apply_blocks' rule: with lim = min(ring_entries, tabs[e].cap) (hpk_test_blkplan_geometry), every
 * block of an encoder is deferred when its max_size exceeds 32 * lim or its count lim at the call's start: applied =
 * 0, the table untouched.
 * Bad inputs. An encoder is void (applied = 0, the table untouched, the sticky flag set: a synchronous call returns
 * HPK_E_INVAL) when its ent + cap passes tab_ent_cap or its count its cap; when its list's offsets decrease or pass
 * enc_blk_off[nencs]; when a listed block is >= nblocks; when a listed block's hdr_off decreases or passes hdrs_cap;
 * when a listed header's field_off decreases or its fields_base + field_off passes arena_cap; or when a carried-in
 * entry's name or value passes arena_cap. Nothing outside the stated sizes is read or written.
 * Pointers: HPK_PTR_DEVICE, optionally HPK_ASYNC (anything else is HPK_E_INVAL); reps and tab_ent 16-byte aligned
 * (HPK_E_INVAL). On the context's stream; always the launch path. Scratch per stream: 8 bytes per header.
 * How: two kernels (hpk_blkplan.hip). A default-and-hash pass, one lane per header: the defaults, and a 32-bit hash
 * of the name and of the value into scratch (a string with bad offsets hashes to 0 and is not read). The plan
 * kernel, one wave per encoder: the lane-parallel look for void inputs; the table in a ring of ring_entries records
 * in LDS, an hpk_header and the two hashes each, the carried-in entries hashed once at load, one lane per entry;
 * static entry `lane` in each lane's registers; per chunk of chunk_headers headers the lanes stage offsets and
 * hashes and the headers are resolved in turn: the search runs in ascending groups of search_group entries, each
 * lane testing one entry by name length, name hash, value length and value hash and confirming on the arena's
 * bytes, a ballot giving the lowest whole match, which ends the search, and the highest name match so far. The hash
 * only filters: every match is confirmed on bytes.
 * Costs: one lane hashes or confirms a whole string, so a multi-KiB value holds its wave for that many byte loads; a
 * call takes as long as its longest encoder; the strings call sees 3 hdrs_cap items, most of them empty. */
typedef enum hpk_plan_kind { HPK_PLAN_NONE = 0, HPK_PLAN_INDEXED = 1, HPK_PLAN_NAME_INDEXED = 2,
                             HPK_PLAN_NEW_NAME = 3 } hpk_plan_kind;
typedef struct hpk_hrep {    /* one planned header; 16 bytes */
    uint32_t index;          /* the table index of the representation (0 for HPK_PLAN_NEW_NAME and HPK_PLAN_NONE) */
    uint8_t  kind;           /* hpk_plan_kind */
    uint8_t  prefix_len;     /* octets of `prefix` in use (0 for HPK_PLAN_NONE) */
    uint16_t reserved0;
    uint8_t  prefix[4];      /* the representation's first octets: the dword at arena[prefix_base + 4j] */
    uint32_t reserved1;
} hpk_hrep;

int hpk_plan_blocks(hpk_ctx* ctx,
        uint8_t* arena, size_t arena_cap, uint32_t static_base, uint32_t fields_base, uint32_t prefix_base,
        const uint32_t* field_off, const uint32_t* hdr_off, uint32_t nblocks, size_t hdrs_cap,
        const uint32_t* enc_blk_off, const uint32_t* enc_blk, const uint8_t* enc_flags, uint32_t nencs,
                                  /* encoder e's blocks, in connection order: enc_blk[enc_blk_off[e] .. enc_blk_off[e+1]) */
        hpk_dtab* tabs, hpk_header* tab_ent, size_t tab_ent_cap,
        hpk_hrep* reps, uint32_t* item_off, uint32_t* item_len, uint8_t* item_policy, int flags);
/* Where hpk_henc_encode_blocks runs a context's table logic. HPK_BLOCK_PLAN_HOST (the default): on the host, as
 * described at hpk_henc_encode_blocks. HPK_BLOCK_PLAN_DEVICE (opt-in; calls without a context are not affected)
 * selects the whole device pipeline: the blocks are grouped by encoder with a counting pass; one arena goes up (the
 * static text, every distinct encoder's live entries' bytes, the fields; the prefix area is reserved, not uploaded)
 * with the hpk_dtab / hpk_header records, the lists and the offsets; hpk_plan_blocks' two kernels run; hpk_pack_batch's
 * kernels gather the 3 nh items into a contiguous blob; hpk_encode_strings_packed's steps code them with the item
 * policies; the tables, their final entries, the output offsets at the block boundaries and exactly the coded bytes
 * come back. Every encoder's table is then rebuilt from its final entries' bytes in the host's own copy of the arena.
 * Nothing is written to an encoder before everything is back, so a device failure (or hpk_test_fail_batches) on this
 * path leaves every encoder as it was. If any encoder would be deferred (its max_size above 32 * ring_entries or its
 * entries above ring_entries, which the host sees before any upload), if the arena or the items' bound would pass the
 * u32 offset range, if no block has a header, or if an encoder came back not fully planned, the host path answers
 * the whole call with its own checks. Results and encoder states equal the default path's byte for byte.
 * Measurements: with HPK_HENC_TIMING set in the environment, every call on the device path waits for the stream
 * after each pass and prints the passes' wall times to stderr (upload, plan, item gather, string coding, copies
 * back); scripts/blocks_plan_time.py split collects them. */
#define HPK_BLOCK_PLAN_HOST 0    /* the default */
#define HPK_BLOCK_PLAN_DEVICE 1
int hpk_ctx_set_block_plan(hpk_ctx* ctx, int kind);
/* Testing only: how many hpk_henc_encode_blocks calls of this context the device-plan path has answered (its tables
 * committed), so the tests can tell it from the host path, which answers by default and after a fallback. */
uint64_t hpk_test_plan_calls(const hpk_ctx* ctx);
/* Testing only: the block plan's geometry (hpk_plan_blocks): the records of an encoder's ring in LDS, the headers a
 * wave stages at a time, the encoders per workgroup (one wave each) and the entries a search step tests. */
int hpk_test_blkplan_geometry(uint32_t* ring_entries, uint32_t* chunk_headers, uint32_t* wg_encoders,
                              uint32_t* search_group);
/* Testing only: the plan kernels' hash of n strings, string i = blob[off[i] .. off[i+1]), into out (n entries). A
 * pure host function. The tests use it to place collisions. */
int hpk_test_blkplan_hash(const uint8_t* blob, const uint32_t* off, uint32_t n, uint32_t* out);
/* Testing only: the compacted form's internal bound layout of n literals' device offsets in_off
 * (n + 1 entries) into device memory out (n + 1 entries): the exclusive sum mod 2^32 of
 * (floor(8 len / 5) + 3) & ~3, synchronously on the context's stream. */
int hpk_test_bound_scan(hpk_ctx* ctx, const uint32_t* in_off, uint32_t n, uint32_t* out);
/* Testing only: the pack kernel's geometry: the bytes of a destination tile (a multiple of 16; tiles lie on
 * 16-byte boundaries of the destination address) and how many literals' offsets a workgroup stages in
 * LDS at a time. The tests place their edge cases relative to these. */
int hpk_test_pack_geometry(uint32_t* tile_bytes, uint32_t* lds_literals);
/* Testing only: the encode kernel's geometry: input bytes per tile, bytes of the LDS output image,
 * literals per tile, input bytes per thread, and the literal count up to which a batch runs in one
 * workgroup. The tests place their edge cases relative to these. */
int hpk_test_encode_geometry(uint32_t* tile_bytes, uint32_t* image_bytes, uint32_t* tile_literals,
                             uint32_t* thread_bytes, uint32_t* one_wg_literals);
/* Testing only: the length pass's geometry (hpk_encoded_len_batch, hpk_encode_batch_packed): the input bytes
 * of a stretch (a workgroup walks its literals in stretches that start at the 16-byte boundary at or below
 * the first unfinished literal's start, or where the previous stretch ended when a literal passed its end),
 * the literals it looks at per stretch, and the literal count up to which a batch runs in one workgroup. */
int hpk_test_enclen_geometry(uint32_t* stretch_bytes, uint32_t* window_literals, uint32_t* one_wg_literals);
/* Testing only: the string-literal emit kernel's geometry (hpk_encode_strings_packed): input bytes per tile,
 * bytes of the LDS output image, literals per tile, and the literal count up to which a batch runs in one
 * workgroup. Its tiles are cut by the encode kernel's rule on the representations' offsets. */
int hpk_test_strings_geometry(uint32_t* tile_bytes, uint32_t* image_bytes, uint32_t* tile_literals,
                              uint32_t* one_wg_literals);
/* Testing only: the geometry of the decode kernels' two phases behind the fills, for kernel `kind`
 * (HPK_DECODE_FILL or HPK_DECODE_WAVE; anything else is HPK_E_INVAL). out13 is a buffer of 13 values:
 * [0] the workgroup's threads (the lanes the huge-literal phase has), [1] the encoded bytes from which a literal
 * is a huge one, [2] the huge literals a workgroup lists at most (further ones go to the long-literal phase),
 * [3] the least bytes of a huge literal's piece, [4] the encoded bytes from which a literal goes to the
 * long-literal phase and [5] from which it is listed at the front, [6] the long phase's input ring in dwords per
 * lane, [7] the 16-byte chunks a lane loads per refill point, [8] the steps between refill points, [9] the list
 * entries per claim, [10] the waves that decode, [11] a lane's output buffer in bytes, [12] the two-symbol table
 * both phases walk with (2, 3 or 4: hpk_walk.h). The tests place their edge cases relative to these. */
int hpk_test_decode_geometry(int kind, uint32_t* out13);
/* Testing only: how many decode calls of this context the small-call mode's persistent kernel has
 * answered (hpk_ctx_set_small_mode), so the tests can tell it ran. */
uint64_t hpk_test_small_calls(const hpk_ctx* ctx);
/* Testing only: the small-call mode's device stamps of its last request (100 MHz ticks): workgroup 0 saw
 * it, broadcast it, finished its literals; the last workgroup published it; then workgroup 0's shader-clock
 * cycles from the broadcast to its finish and the same interval in 100 MHz ticks; thread 0's first literal in
 * shader-clock cycles: offsets loaded, staged, walked, stored. out10 is a buffer of 10 values: the six
 * request stamps, then the four of the literal. */
int hpk_test_small_stamps(const hpk_ctx* ctx, uint32_t* out10);
/* Testing only: the geometry of the small-call mode's persistent kernel: the encoded bytes up to which a literal
 * is staged in LDS (longer ones are walked from global memory), the 16-byte chunks of a lane's input slot, the
 * dwords of a lane's output slot, and the threads of a workgroup. A pure host function (no device needed). The
 * tests place their edge cases relative to these. */
int hpk_test_persist_geometry(uint32_t* slot_max, uint32_t* slot_chunks, uint32_t* out_dwords, uint32_t* threads);
/* Testing only: stop the small-call mode's persistent kernel if it runs and make `v` the last request number
 * issued, so that the next small call issues the number after it (the numbers wrap at 2^32 and skip
 * 0xFFFFFFFF, the kernel's exit command, and 0). v = 0xFFFFFFFF, or a context whose mode was never turned on, is
 * HPK_E_INVAL. */
int hpk_test_small_set_request(hpk_ctx* ctx, uint32_t v);
/* Testing only: the block scan's geometry (hpk_scan_blocks): the blocks a workgroup of either pass walks, one
 * per lane. The tests place their block counts relative to it. */
int hpk_test_blkscan_geometry(uint32_t* wg_blocks);
/* Testing only: the frame scan's geometry (hpk_scan_frames): the connections a workgroup of either pass walks,
 * one per lane. The tests place their connection counts relative to it. */
int hpk_test_frmscan_geometry(uint32_t* wg_conns);

/* Testing only: the frame write's geometry: the bytes of a destination tile and the blocks a workgroup's LDS window
 * holds (more blocks of no octets than that in a row force a restage inside one tile). */
int hpk_test_frmwrite_geometry(uint32_t* tile_bytes, uint32_t* lds_blocks);

/* Library/kernel identification (for logs and the bench JSON). */
const char* hpk_version(void);

#ifdef __cplusplus
}
#endif

#endif /* HPK_H */
