"""Batched Huffman codec on the GPU (hpk_decode_batch / hpk_encode_batch of include/hpk.h).

Layout (one shard, u32 offsets): literal i is in_blob[in_off[i]:in_off[i+1]]; its output goes to
out_blob[out_off[i]:out_off[i+1]] (capacity), out_len[i] bytes are valid, status[i] is the
hpk_status (0 ok, 1 PaddingTooLarge, 2 InvalidPadding, 3 EOSInString, 4 output overflow).

Device tensors go straight to the kernels on the codec's stream: by default torch's current
stream on the codec's device at the time of each call, so torch ops that produced the inputs and
the caching allocator's reuse of the outputs are ordered with the kernels. Host numpy arrays go
through the library's own H2D/D2H staging. Every buffer is checked before it reaches the C ABI
(dtype, contiguity, device, room for n entries), and the C ABI gets each blob's capacity, so
offsets past a blob are rejected on the device (status HPK_BAD_OFFSETS) instead of read or written.
There is no CPU fallback anywhere in this module.
"""

from __future__ import annotations

import ctypes

import numpy as np

from . import _lib

U32 = np.uint32
# hpk_header, hpk_block_result and hpk_dtab (hpk.h), for apply_blocks' byte tensors
HEADER_DTYPE = np.dtype([("name_off", "<u4"), ("name_len", "<u4"), ("value_off", "<u4"), ("value_len", "<u4")])
RESULT_DTYPE = np.dtype([("first_header", "<u4"), ("n_headers", "<u4"), ("error", "<i4"), ("detail", "<i4")])
DTAB_DTYPE = np.dtype([("ent", "<u4"), ("cap", "<u4"), ("count", "<u4"), ("size", "<u4"), ("max_size", "<u4"),
                       ("max_allowed", "<u4"), ("applied", "<u4"), ("reserved", "<u4")])
# hpk_hrep (hpk.h): one 16-byte record of plan_blocks
HREP_DTYPE = np.dtype([("index", "<u4"), ("kind", "u1"), ("prefix_len", "u1"), ("reserved0", "<u2"), ("prefix", "u1", (4,)),
                       ("reserved1", "<u4")])
# hpk_field (hpk.h): one 16-byte record of scan_blocks
FIELD_DTYPE = np.dtype([("index", "<u4"), ("str", "<u4"), ("kind", "u1"), ("nstr", "u1"), ("err", "u1"),
                        ("err_stage", "u1"), ("at", "<u4")])
# hpk_fconn and hpk_fblock (hpk.h): scan_frames' 32-byte connection states and 16-byte block records
FCONN_DTYPE = np.dtype([("max_frame_size", "<u4"), ("error", "<i4"), ("pending", "<u4"), ("pend_stream", "<u4"),
                        ("carry_off", "<u4"), ("carry_len", "<u4"), ("consumed", "<u4"), ("status", "<u4")])
FBLOCK_DTYPE = np.dtype([("conn", "<u4"), ("stream_id", "<u4"), ("frag", "<u4"), ("nfrag", "<u4")])


def pack(literals):
    """list of bytes -> (blob u8, off u32[n+1])."""
    lens = np.fromiter((len(x) for x in literals), dtype=np.int64, count=len(literals))
    off = np.zeros(len(literals) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    if off[-1] >= 2**32:
        raise ValueError("a shard must stay below 4 GiB (u32 offsets)")
    blob = np.frombuffer(b"".join(bytes(x) for x in literals), dtype=np.uint8).copy()
    return blob, off.astype(U32)


def unpack(blob, off, lens=None):
    blob = np.asarray(blob)
    off = np.asarray(off, dtype=np.int64)
    if lens is None:
        return [blob[off[i] : off[i + 1]].tobytes() for i in range(len(off) - 1)]
    lens = np.asarray(lens, dtype=np.int64)
    return [blob[off[i] : off[i] + lens[i]].tobytes() for i in range(len(off) - 1)]


def _round4(b):
    return (b + 3) & ~3


def decode_offsets_np(in_off):
    """Output offsets from hpk_decoded_bound(len) = floor(8*len/5) per literal, each capacity
    rounded up to 4 bytes so every literal's output starts dword-aligned (the kernels' fast
    store path; unaligned offsets are still handled)."""
    in_off = np.asarray(in_off, dtype=np.int64)
    b = _round4((np.diff(in_off) * 8) // 5)
    out = np.zeros(len(in_off), dtype=np.int64)
    np.cumsum(b, out=out[1:])
    if out[-1] >= 2**32:
        raise ValueError("decoded bound of the shard exceeds 4 GiB")
    return out.astype(U32)


def encode_offsets_np(in_off):
    """Output offsets from hpk_encoded_bound(len) = ceil(30*len/8) per literal (rounded to 4)."""
    in_off = np.asarray(in_off, dtype=np.int64)
    b = _round4((np.diff(in_off) * 30 + 7) // 8)
    out = np.zeros(len(in_off), dtype=np.int64)
    np.cumsum(b, out=out[1:])
    if out[-1] >= 2**32:
        raise ValueError("encoded bound of the shard exceeds 4 GiB")
    return out.astype(U32)


_OFF_DTYPES = ("int32", "uint32")


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def _arg(x, name, kinds, min_len, device_index=None):
    """(pointer, byte size) of a contiguous numpy array or torch tensor, after checking its dtype
    (one of `kinds`), its length (>= min_len entries) and, for device calls, that it is a CUDA
    tensor on the codec's device. Raises ValueError / TypeError instead of handing the C ABI a
    buffer it would misread (an int64 offset tensor read as u32 halves, a view, a short array)."""
    if _is_torch(x):
        dt = str(x.dtype).replace("torch.", "")
        if device_index is not None:
            if not x.is_cuda or x.device.index != device_index:
                raise ValueError(f"{name}: expected a tensor on cuda:{device_index}, got {x.device}")
        elif x.is_cuda:
            raise ValueError(f"{name}: host-pointer call given a CUDA tensor")
        if not x.is_contiguous():
            raise ValueError(f"{name}: tensor must be contiguous")
        n, nbytes, ptr = x.numel(), x.numel() * x.element_size(), x.data_ptr()
    elif isinstance(x, np.ndarray):
        if device_index is not None:
            raise ValueError(f"{name}: device call given a host numpy array")
        dt = str(x.dtype)
        if not x.flags["C_CONTIGUOUS"]:
            raise ValueError(f"{name}: array must be C-contiguous")
        n, nbytes, ptr = x.size, x.nbytes, x.ctypes.data
    else:
        raise TypeError(f"{name}: expected a numpy array or torch tensor, got {type(x).__name__}")
    if dt not in kinds:
        raise TypeError(f"{name}: dtype {dt} not in {kinds}")
    if n < min_len:
        raise ValueError(f"{name}: {n} entries, need >= {min_len}")
    return ctypes.c_void_p(ptr), nbytes


class HuffmanCodec:
    """One device context (hpk_ctx): a HIP stream + LDS-staged decode tables on one GPU.

    loona is thread-per-core and !Send (crates/buffet/src/lib.rs:38-49): use one codec per
    host thread.

    stream: None (default) = torch's current stream on `device` at each call; a torch.cuda.Stream
    or raw hipStream_t int = that stream; "own" = the context's own non-blocking stream."""

    def __init__(self, device: int = 0, stream=None):
        self._L = _lib.lib()
        self.device = device
        h = self._L.hpk_ctx_create(device)
        if not h:
            raise RuntimeError(f"hpk_ctx_create({device}) failed: {_lib.last_error()}")
        self._h = h
        self._follow_torch = stream is None
        self._bound = None
        if stream is not None and stream != "own":
            self.set_stream(stream)

    def close(self):
        if getattr(self, "_h", None):
            self._L.hpk_ctx_destroy(self._h)
            self._h = None
            # hpk_ctx_destroy ignores what its HIP calls return (waiting for a slot's event whose stream
            # the caller has destroyed since can fail), but HIP keeps a thread's last failure, and torch
            # reads it after its next kernel launch and raises it as that launch's. Take it away here.
            _lib.clear_hip_error()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_stream(self, stream):
        """stream: a torch.cuda.Stream (its handle 0 = the legacy null stream), a raw hipStream_t
        int, or None (the ctx's own non-blocking stream). Fixes the stream for later calls."""
        self._follow_torch = False
        self._bind(stream)

    def _bind(self, stream):
        if stream is None:
            arg = None
        else:
            raw = int(getattr(stream, "cuda_stream", stream))
            arg = ctypes.c_void_p(raw) if raw else ctypes.c_void_p(-1 & 0xFFFFFFFFFFFFFFFF)  # HPK_STREAM_LEGACY
        _lib.check(self._L.hpk_ctx_set_stream(self._h, arg), "hpk_ctx_set_stream")
        self._bound = None if arg is None else arg.value

    def _follow(self):
        """Bind torch's current stream on the codec's device (default mode)."""
        if not self._follow_torch:
            return
        import torch

        s = torch.cuda.current_stream(self.device)
        raw = int(s.cuda_stream) or (-1 & 0xFFFFFFFFFFFFFFFF)
        if raw != self._bound:
            self._bind(s)

    DECODE_KERNELS = {"auto": 0, "fill": 1, "wave": 2}

    def set_decode_kernel(self, kind: str):
        """'auto' (default: wave fills for every batch since round 6), 'fill' or 'wave'
        (hpk_ctx_set_decode_kernel): the same results, different speed."""
        if kind not in self.DECODE_KERNELS:
            raise ValueError(f"decode kernel {kind!r} not in {tuple(self.DECODE_KERNELS)}")
        _lib.check(self._L.hpk_ctx_set_decode_kernel(self._h, self.DECODE_KERNELS[kind]), "hpk_ctx_set_decode_kernel")

    def set_small_mode(self, max_literals: int, workgroups: int = 4, idle_ms: int = 50):
        """The small-call mode (hpk_ctx_set_small_mode): synchronous device-pointer decode calls of at
        most max_literals literals go to a persistent kernel of `workgroups` workgroups instead of a
        launch; it exits after idle_ms without a call. max_literals = 0 turns it off."""
        _lib.check(self._L.hpk_ctx_set_small_mode(self._h, int(max_literals), int(workgroups), int(idle_ms)),
                   "hpk_ctx_set_small_mode")

    def sync(self):
        _lib.check(self._L.hpk_ctx_sync(self._h), "hpk_ctx_sync")

    def check(self):
        """Sticky device error flag (bad offsets in an earlier HPK_ASYNC call): raises if set."""
        _lib.check(self._L.hpk_ctx_check(self._h), "hpk_ctx_check")

    # -- raw entry points --------------------------------------------------------------------
    def _call(self, fn, name, in_blob, in_off, out_blob, out_off, out_len, status, device, sync):
        dev = self.device if device else None
        n = (int(in_off.shape[0]) if hasattr(in_off, "shape") else len(in_off)) - 1
        if n < 0:
            raise ValueError("in_off needs n+1 >= 1 entries")
        if n >= 2**32:
            raise ValueError("a batch holds at most 2^32 - 1 literals")
        pi, in_cap = _arg(in_blob, "in_blob", ("uint8",), 0, dev)
        pio, _ = _arg(in_off, "in_off", _OFF_DTYPES, n + 1, dev)
        po, out_cap = _arg(out_blob, "out_blob", ("uint8",), 0, dev)
        poo, _ = _arg(out_off, "out_off", _OFF_DTYPES, n + 1, dev)
        pl, _ = _arg(out_len, "out_len", ("int32", "uint32"), n, dev)
        ps, _ = _arg(status, "status", ("uint8",), n, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        rc = fn(self._h, pi, in_cap, pio, ctypes.c_uint32(n), po, out_cap, poo, pl, ps, flags)
        _lib.check(rc, name)

    def decode_into(self, in_blob, in_off, out_blob, out_off, out_len, status, device=True, sync=False):
        """hpk_decode_batch. device=True: CUDA tensors on the codec's device, enqueued (sync=False:
        HPK_ASYNC; bad offsets then show as status HPK_BAD_OFFSETS and in check()). device=False:
        host numpy arrays, staged and synchronous."""
        self._call(self._L.hpk_decode_batch, "hpk_decode_batch", in_blob, in_off, out_blob, out_off, out_len,
                   status, device, sync)

    def encode_into(self, in_blob, in_off, out_blob, out_off, out_len, status, device=True, sync=False):
        """hpk_encode_batch, same conventions as decode_into."""
        self._call(self._L.hpk_encode_batch, "hpk_encode_batch", in_blob, in_off, out_blob, out_off, out_len,
                   status, device, sync)

    # -- host (numpy) convenience ------------------------------------------------------------
    def decode_host(self, in_blob, in_off, out_off=None):
        """numpy in -> (out_blob, out_off, out_len, status), staged through the ctx."""
        in_blob = np.ascontiguousarray(in_blob, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=U32)
        out_off = decode_offsets_np(in_off) if out_off is None else np.ascontiguousarray(out_off, dtype=U32)
        n = len(in_off) - 1
        out_blob = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(max(n, 1), dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if in_blob.size == 0:
            in_blob = np.zeros(1, dtype=np.uint8)
        self.decode_into(in_blob, in_off, out_blob, out_off, out_len, status, device=False)
        return out_blob, out_off, out_len[:n], status[:n]

    def encode_host(self, in_blob, in_off, out_off=None):
        in_blob = np.ascontiguousarray(in_blob, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=U32)
        out_off = encode_offsets_np(in_off) if out_off is None else np.ascontiguousarray(out_off, dtype=U32)
        n = len(in_off) - 1
        out_blob = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
        out_len = np.zeros(max(n, 1), dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if in_blob.size == 0:
            in_blob = np.zeros(1, dtype=np.uint8)
        self.encode_into(in_blob, in_off, out_blob, out_off, out_len, status, device=False)
        return out_blob, out_off, out_len[:n], status[:n]

    # -- device (torch) convenience ----------------------------------------------------------
    def decode_device(self, in_blob, in_off, out_off=None, out_blob=None, out_len=None, status=None, sync=False):
        """torch cuda tensors (u8 blob, int32/uint32 offsets) -> (out_blob, out_off, out_len, status)."""
        import torch

        n = int(in_off.shape[0]) - 1
        if out_off is None:
            out_off = decode_offsets_torch(in_off)
        dev = in_blob.device
        if out_blob is None:
            out_blob = torch.empty(max(int(out_off[-1].item()), 1), dtype=torch.uint8, device=dev)
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self.decode_into(in_blob, in_off, out_blob, out_off, out_len, status, device=True, sync=sync)
        return out_blob, out_off, out_len, status

    def decode_compact(self, in_blob, in_off, out_blob=None, out_off=None, out_len=None, status=None, sync=False):
        """hpk_decode_batch_compact: torch cuda tensors -> (out_blob, out_off, out_len, status) with each
        literal's decoded bytes written exactly (the reference's exact-length outputs, huffman.rs:98, 160):
        literal i is out_blob[out_off[i] : out_off[i] + out_len[i]] and out_off[n] is the end of the span
        written to. out_off is an output (n + 1 entries; runs of literals in completion order, so not
        monotone). The span is not gap-free: listed (long / huge) literals keep their decoded bound, and
        the wave-fill kernel (every auto or wave batch) packs per workgroup, each share ending in an unwritten tail
        (include/hpk.h); shard.compact gathers the bytes end to end."""
        import torch

        n = int(in_off.shape[0]) - 1
        dev = in_blob.device
        need = compact_capacity(int(in_blob.numel()), n)
        if out_blob is None:
            out_blob = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
        if out_off is None:
            out_off = torch.empty(n + 1, dtype=torch.int32 if need < 2**31 else torch.uint32, device=dev)
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._call(self._L.hpk_decode_batch_compact, "hpk_decode_batch_compact", in_blob, in_off, out_blob, out_off,
                   out_len, status, True, sync)
        return out_blob, out_off, out_len, status

    def decode_packed(self, in_blob, in_off, out_blob=None, out_off=None, out_len=None, status=None, sync=False):
        """hpk_decode_batch_packed: torch cuda tensors -> (out_blob, out_off, out_len, status) with the decoded
        bytes end to end in literal order, what the reference's exact-length Vecs (huffman.rs:98, 160) would
        be, concatenated: out_off (n + 1 entries, an output) is the exclusive sum of out_len, literal i is
        out_blob[out_off[i] : out_off[i + 1]] and out_off[n] the decoded total; status and out_len as
        decode_device. out_blob may have any capacity: the bytes below it are written, and a synchronous call
        raises (HPK_E_NOSPACE) when out_off[n] passes it; after an async call compare out_off[n] yourself.
        out_blob=None allocates hpk_decoded_bound(in_blob) bytes, which always suffice, and with sync=True
        the blob comes back cut to out_blob[:total] (the one host read of out_off[n]; not made otherwise)."""
        import torch

        n = int(in_off.shape[0]) - 1
        dev = in_blob.device
        need = compact_capacity(int(in_blob.numel()), n)
        own = out_blob is None
        if own:
            out_blob = torch.empty(max((8 * int(in_blob.numel())) // 5, 1), dtype=torch.uint8, device=dev)
        if out_off is None:
            out_off = torch.empty(n + 1, dtype=torch.int32 if need < 2**31 else torch.uint32, device=dev)
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._call(self._L.hpk_decode_batch_packed, "hpk_decode_batch_packed", in_blob, in_off, out_blob, out_off,
                   out_len, status, True, sync)
        if own and sync:
            out_blob = out_blob[: int(out_off[n].item()) & 0xFFFFFFFF]
        return out_blob, out_off, out_len, status

    def pack(self, src_blob, src_off, src_len, dst_blob=None, dst_off=None, sync=False):
        """hpk_pack_batch: n = len(src_len) pieces src_blob[src_off[i] : src_off[i] + src_len[i]] (torch cuda
        tensors; the starts in any order, a region form's n + 1 offsets accepted as they are) laid end to end
        -> (dst_blob, dst_off), dst_off (n + 1 entries) the exclusive sum of src_len. A piece that passes
        src_blob counts 0 bytes and raises the sticky error. dst_blob=None allocates src_blob's size (the
        pieces of a decode result never sum to more), cut to dst_blob[:total] when sync=True; capacity
        rules as decode_packed."""
        import torch

        n = int(src_len.shape[0])
        if n >= 2**31 - 1:
            raise ValueError("too many pieces")
        dev = self.device
        ps, src_cap = _arg(src_blob, "src_blob", ("uint8",), 0, dev)
        pso, _ = _arg(src_off, "src_off", _OFF_DTYPES, n, dev)
        psl, _ = _arg(src_len, "src_len", _OFF_DTYPES, n, dev)
        own = dst_blob is None
        if own:
            dst_blob = torch.empty(max(int(src_blob.numel()), 1), dtype=torch.uint8, device=src_blob.device)
        if dst_off is None:
            dst_off = torch.empty(n + 1, dtype=torch.int32 if int(dst_blob.numel()) < 2**31 else torch.uint32,
                                  device=src_blob.device)
        pd, dst_cap = _arg(dst_blob, "dst_blob", ("uint8",), 0, dev)
        pdo, _ = _arg(dst_off, "dst_off", _OFF_DTYPES, n + 1, dev)
        self._follow()
        flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        rc = self._L.hpk_pack_batch(self._h, ps, src_cap, pso, psl, ctypes.c_uint32(n), pd, dst_cap, pdo, flags)
        _lib.check(rc, "hpk_pack_batch")
        if own and sync:
            dst_blob = dst_blob[: int(dst_off[n].item()) & 0xFFFFFFFF]
        return dst_blob, dst_off

    def encode_device(self, in_blob, in_off, out_off=None, out_blob=None, out_len=None, status=None, sync=False):
        import torch

        n = int(in_off.shape[0]) - 1
        if out_off is None:
            out_off = encode_offsets_torch(in_off)
        dev = in_blob.device
        if out_blob is None:
            out_blob = torch.empty(max(int(out_off[-1].item()), 1), dtype=torch.uint8, device=dev)
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self.encode_into(in_blob, in_off, out_blob, out_off, out_len, status, device=True, sync=sync)
        return out_blob, out_off, out_len, status


    def encoded_len_device(self, in_blob, in_off, out_len=None, sync=False):
        """hpk_encoded_len_batch: torch cuda tensors -> out_len, literal i's Huffman-encoded length in bytes
        (hpk_huffman_encoded_len of it: ceil(code bits / 8), 0 for an empty literal), with no byte encoded:
        the number the H-bit rule (RFC 7541 section 5.2, "Huffman only where strictly shorter") compares with
        the raw length. A literal with bad offsets counts 0 and raises the sticky error."""
        import torch

        n = int(in_off.shape[0]) - 1
        if n < 0:
            raise ValueError("in_off needs n+1 >= 1 entries")
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=in_blob.device)
        dev = self.device
        pi, in_cap = _arg(in_blob, "in_blob", ("uint8",), 0, dev)
        pio, _ = _arg(in_off, "in_off", _OFF_DTYPES, n + 1, dev)
        pl, _ = _arg(out_len, "out_len", _OFF_DTYPES, n, dev)
        self._follow()
        flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        rc = self._L.hpk_encoded_len_batch(self._h, pi, in_cap, pio, ctypes.c_uint32(n), pl, flags)
        _lib.check(rc, "hpk_encoded_len_batch")
        return out_len

    def encode_packed(self, in_blob, in_off, out_blob=None, out_off=None, out_len=None, status=None, sync=False):
        """hpk_encode_batch_packed: torch cuda tensors -> (out_blob, out_off, out_len, status) with the encoded
        bytes end to end in literal order: out_off (n + 1 entries, an output) is the exclusive sum of out_len,
        literal i is out_blob[out_off[i] : out_off[i + 1]] and out_off[n] the encoded total, so the result
        feeds decode_packed as it is. The bytes are encode_device's for regions that are large enough; status
        is 0, or 5 (bad offsets, out_len 0), never 4. out_blob may have any capacity: the bytes below it are
        written, and a synchronous call raises (HPK_E_NOSPACE) when out_off[n] passes it; after an async call
        compare out_off[n] yourself. out_blob=None with sync=True: the lengths are computed first
        (encoded_len_device) and one host read of their total sizes the blob exactly. out_blob=None otherwise:
        hpk_encoded_bound of the input, which always suffices."""
        import torch

        n = int(in_off.shape[0]) - 1
        dev = in_blob.device
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if out_blob is None:
            if sync and n > 0:
                # (synchronous: the total is read by torch on its current stream, which need not be the codec's)
                self.encoded_len_device(in_blob, in_off, out_len=out_len, sync=True)
                total = int((out_len[:n].to(torch.int64) & 0xFFFFFFFF).sum().item())
                if total > _lib.HPK_MAX_OFFSET:  # (the call voids such a batch and writes no byte)
                    total = 0
                out_blob = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
            else:
                out_blob = torch.empty(max((30 * int(in_blob.numel()) + 7) // 8, 1), dtype=torch.uint8, device=dev)
        if out_off is None:
            out_off = torch.empty(n + 1, dtype=torch.int32 if int(out_blob.numel()) < 2**31 else torch.uint32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._call(self._L.hpk_encode_batch_packed, "hpk_encode_batch_packed", in_blob, in_off, out_blob, out_off,
                   out_len, status, True, sync)
        return out_blob, out_off, out_len, status

    def _strings_call(self, in_blob, in_off, policy, out_blob, out_off, out_len, status, device, sync):
        dev = self.device if device else None
        n = int(in_off.shape[0]) - 1
        if n < 0:
            raise ValueError("in_off needs n+1 >= 1 entries")
        pi, in_cap = _arg(in_blob, "in_blob", ("uint8",), 0, dev)
        pio, _ = _arg(in_off, "in_off", _OFF_DTYPES, n + 1, dev)
        pp = None if policy is None else _arg(policy, "policy", ("uint8",), n, dev)[0]
        pl, _ = _arg(out_len, "out_len", _OFF_DTYPES, n, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        if out_blob is None:  # the lengths alone
            rc = self._L.hpk_string_len_batch(self._h, pi, in_cap, pio, ctypes.c_uint32(n), pp, pl, flags)
            _lib.check(rc, "hpk_string_len_batch")
            return
        po, out_cap = _arg(out_blob, "out_blob", ("uint8",), 0, dev)
        poo, _ = _arg(out_off, "out_off", _OFF_DTYPES, n + 1, dev)
        ps, _ = _arg(status, "status", ("uint8",), n, dev)
        rc = self._L.hpk_encode_strings_packed(self._h, pi, in_cap, pio, ctypes.c_uint32(n), pp, po, out_cap, poo, pl,
                                               ps, flags)
        _lib.check(rc, "hpk_encode_strings_packed")

    def string_len_device(self, in_blob, in_off, policy=None, out_len=None, sync=False):
        """hpk_string_len_batch: torch cuda tensors -> out_len, the bytes of literal i's RFC 7541 section 5.2
        representation under policy[i] (see encode_strings), prefix included, with no byte written. A literal
        with bad offsets or a policy above 3 counts 0 and raises the sticky error."""
        import torch

        n = int(in_off.shape[0]) - 1
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=in_blob.device)
        self._strings_call(in_blob, in_off, policy, None, None, out_len, None, True, sync)
        return out_len

    def encode_strings(self, in_blob, in_off, policy=None, out_blob=None, out_off=None, out_len=None, status=None,
                       sync=False):
        """hpk_encode_strings_packed: torch cuda tensors -> (out_blob, out_off, out_len, status) with every
        literal's string-literal representation (RFC 7541 section 5.2) end to end in literal order: the length
        prefix, 0x80 in its first octet for the Huffman form, then the payload. policy (uint8 per literal, or
        None = all 0): 0 Huffman where strictly shorter, else raw (hpack_ref.Encoder._string); 1 always raw;
        2 always Huffman; 3 the bytes as they are, no prefix. out_off (n + 1 entries, an output) is the
        exclusive sum of out_len, out_len the whole representation; status is 0, or 5 (bad offsets or policy,
        out_len 0). Capacity rules as encode_packed. out_blob=None with sync=True: the lengths are computed
        first (string_len_device) and one host read of their total sizes the blob exactly; out_blob=None
        otherwise: a bound that always suffices (6 bytes per literal plus the input, or hpk_encoded_bound of it
        when a policy array may force the Huffman form)."""
        import torch

        n = int(in_off.shape[0]) - 1
        dev = in_blob.device
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if out_blob is None:
            if sync and n > 0:
                self.string_len_device(in_blob, in_off, policy, out_len=out_len, sync=True)
                total = int((out_len[:n].to(torch.int64) & 0xFFFFFFFF).sum().item())
                if total > _lib.HPK_MAX_OFFSET:  # (the call voids such a batch and writes no byte)
                    total = 0
                out_blob = torch.empty(max(total, 1), dtype=torch.uint8, device=dev)[:total]
            else:
                nb = int(in_blob.numel())
                bound = (nb if policy is None else max(nb, (30 * nb + 7) // 8)) + 6 * max(n, 0)
                out_blob = torch.empty(max(bound, 1), dtype=torch.uint8, device=dev)
        if out_off is None:
            out_off = torch.empty(n + 1, dtype=torch.int32 if int(out_blob.numel()) < 2**31 else torch.uint32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._strings_call(in_blob, in_off, policy, out_blob, out_off, out_len, status, True, sync)
        return out_blob, out_off, out_len, status

    def encode_strings_host(self, in_blob, in_off, policy=None, out_cap=None):
        """hpk_encode_strings_packed with host pointers: numpy in -> (out_blob, out_off, out_len, status),
        staged through the context and synchronous. Offsets and policies are checked before anything is copied.
        out_cap: the output's capacity (default: a bound that always suffices); the blob comes back cut to the
        bytes written when the result fits, and the call raises (HPK_E_NOSPACE) when it does not."""
        in_blob = np.ascontiguousarray(in_blob, dtype=np.uint8)
        in_off = np.ascontiguousarray(in_off, dtype=U32)
        policy = None if policy is None else np.ascontiguousarray(policy, dtype=np.uint8)
        n = len(in_off) - 1
        if out_cap is None:
            out_cap = (in_blob.size if policy is None else max(in_blob.size, (30 * in_blob.size + 7) // 8)) + 6 * n
        out_blob = np.zeros(max(int(out_cap), 1), dtype=np.uint8)[: int(out_cap)]
        out_off = np.zeros(n + 1, dtype=U32)
        out_len = np.zeros(max(n, 1), dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if in_blob.size == 0:
            in_blob = np.zeros(1, dtype=np.uint8)[:0]
        self._strings_call(in_blob, in_off, policy, out_blob, out_off, out_len, status, False, True)
        return out_blob[: int(out_off[n])], out_off, out_len[:n], status[:n]

    def _decode_strings_call(self, in_blob, str_off, str_end, out_blob, out_off, out_len, consumed, status, device, sync):
        dev = self.device if device else None
        n = int(str_off.shape[0]) - (1 if str_end is None else 0)
        if n < 0:
            raise ValueError("str_off needs n+1 >= 1 entries when str_end is None")
        pi, in_cap = _arg(in_blob, "in_blob", ("uint8",), 0, dev)
        pso, _ = _arg(str_off, "str_off", _OFF_DTYPES, n + (1 if str_end is None else 0), dev)
        pse = None if str_end is None else _arg(str_end, "str_end", _OFF_DTYPES, n, dev)[0]
        po, out_cap = _arg(out_blob, "out_blob", ("uint8",), 0, dev)
        poo, _ = _arg(out_off, "out_off", _OFF_DTYPES, n + 1, dev)
        pl, _ = _arg(out_len, "out_len", _OFF_DTYPES, n, dev)
        pc = None if consumed is None else _arg(consumed, "consumed", _OFF_DTYPES, n, dev)[0]
        ps, _ = _arg(status, "status", ("uint8",), n, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        rc = self._L.hpk_decode_strings_packed(self._h, pi, in_cap, pso, pse, ctypes.c_uint32(n), po, out_cap, poo, pl, pc,
                                               ps, flags)
        _lib.check(rc, "hpk_decode_strings_packed")

    def decode_strings(self, in_blob, str_off, str_end=None, out_blob=None, out_off=None, out_len=None, consumed=None,
                       status=None, sync=False):
        """hpk_decode_strings_packed: torch cuda tensors -> (out_blob, out_off, out_len, consumed, status). String
        i is the reference's decode_string on the window in_blob[str_off[i] : str_end[i]] (RFC 7541 section 5.2:
        the 7-bit-prefix length, the H bit, then the raw or the Huffman payload); the window may be longer than
        the string, and windows may overlap. str_end=None is the mirror form: str_off has n + 1 entries and
        string i's window is [str_off[i], str_off[i + 1]), encode_strings' out_off as it stands. The decoded
        strings come back end to end: out_off (n + 1 entries, an output) is the exclusive sum of out_len. status
        is decode_device's for a Huffman payload, 0 for a raw string, 5 for a void window, or 6 / 7 / 8 (the
        length integer has too many octets / the window ends inside it / the payload passes the window), each
        with out_len 0; consumed is the prefix octets + the payload length where the prefix and the length check
        passed, else 0. Capacity rules as decode_packed. out_blob=None allocates hpk_decoded_bound(in_blob)
        bytes (enough unless windows overlap), cut to out_blob[:total] when sync=True."""
        import torch

        n = int(str_off.shape[0]) - (1 if str_end is None else 0)
        dev = in_blob.device
        own = out_blob is None
        if own:
            out_blob = torch.empty(max((8 * int(in_blob.numel())) // 5, 1), dtype=torch.uint8, device=dev)
        if out_off is None:
            out_off = torch.empty(n + 1, dtype=torch.int32 if int(out_blob.numel()) < 2**31 else torch.uint32, device=dev)
        if out_len is None:
            out_len = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if consumed is None:
            consumed = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._decode_strings_call(in_blob, str_off, str_end, out_blob, out_off, out_len, consumed, status, True, sync)
        if own and sync:
            out_blob = out_blob[: int(out_off[n].item()) & 0xFFFFFFFF]
        return out_blob, out_off, out_len, consumed, status

    def decode_strings_host(self, in_blob, str_off, str_end=None, out_cap=None):
        """hpk_decode_strings_packed with host pointers: numpy in -> (out_blob, out_off, out_len, consumed,
        status), staged through the context and synchronous. The windows are checked before anything is copied.
        out_cap: the output's capacity (default: the windows' decoded bounds, which always suffice); the blob
        comes back cut to the bytes written when the result fits, and the call raises (HPK_E_NOSPACE) when it
        does not."""
        in_blob = np.ascontiguousarray(in_blob, dtype=np.uint8)
        str_off = np.ascontiguousarray(str_off, dtype=U32)
        str_end = None if str_end is None else np.ascontiguousarray(str_end, dtype=U32)
        n = len(str_off) - (1 if str_end is None else 0)
        if out_cap is None:
            a = str_off[:n].astype(np.int64)
            e = (str_off[1:] if str_end is None else str_end).astype(np.int64)
            out_cap = int((np.maximum(e - a, 0) * 8 // 5).sum())
        out_blob = np.zeros(max(int(out_cap), 1), dtype=np.uint8)[: int(out_cap)]
        out_off = np.zeros(n + 1, dtype=U32)
        out_len = np.zeros(max(n, 1), dtype=U32)
        consumed = np.zeros(max(n, 1), dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if in_blob.size == 0:
            in_blob = np.zeros(1, dtype=np.uint8)[:0]
        self._decode_strings_call(in_blob, str_off, str_end, out_blob, out_off, out_len, consumed, status, False, True)
        return out_blob[: int(out_off[n])], out_off, out_len[:n], consumed[:n], status[:n]

    BLOCK_SCANS = {"host": _lib.HPK_BLOCK_SCAN_HOST, "device": _lib.HPK_BLOCK_SCAN_DEVICE}

    def set_block_scan(self, kind: str):
        """'host' (the default) or 'device' (hpk_ctx_set_block_scan): where hpack.decode_blocks and
        h2.read_frames scan this codec's header blocks. The same results; 'device' uploads the blocks as they are
        and runs scan_blocks' kernels and decode_strings' pipeline before the host applies the records."""
        if kind not in self.BLOCK_SCANS:
            raise ValueError(f"block scan {kind!r} not in {tuple(self.BLOCK_SCANS)}")
        _lib.check(self._L.hpk_ctx_set_block_scan(self._h, self.BLOCK_SCANS[kind]), "hpk_ctx_set_block_scan")

    def _scan_blocks_call(self, blocks, block_off, fields, field_off, str_off, str_end, str_blk_off, status, device, sync):
        dev = self.device if device else None
        n = int(block_off.shape[0]) - 1
        if n < 0:
            raise ValueError("block_off needs nblocks+1 >= 1 entries")
        pb, cap = _arg(blocks, "blocks", ("uint8",), 0, dev)
        pbo, _ = _arg(block_off, "block_off", _OFF_DTYPES, n + 1, dev)
        pf, fbytes = _arg(fields, "fields", ("uint8",), 0, dev)
        pfo, _ = _arg(field_off, "field_off", _OFF_DTYPES, n + 1, dev)
        pso, sbytes = _arg(str_off, "str_off", _OFF_DTYPES, 0, dev)
        pse, ebytes = _arg(str_end, "str_end", _OFF_DTYPES, 0, dev)
        psb, _ = _arg(str_blk_off, "str_blk_off", _OFF_DTYPES, n + 1, dev)
        pst, _ = _arg(status, "status", ("uint8",), n, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        rc = self._L.hpk_scan_blocks(self._h, pb, cap, pbo, ctypes.c_uint32(n), pf, fbytes // 16, pfo, pso, pse,
                                     min(sbytes, ebytes) // 4, psb, pst, flags)
        _lib.check(rc, "hpk_scan_blocks")

    def scan_blocks(self, blocks, block_off, fields=None, field_off=None, str_off=None, str_end=None, str_blk_off=None,
                    status=None, sync=False):
        """hpk_scan_blocks: torch cuda tensors -> (fields, field_off, str_off, str_end, str_blk_off, status). Block
        b is blocks[block_off[b] : block_off[b + 1]]; it is tokenised with no decoder in hand (the table-free half
        of Decoder::decode_with_cb). fields is a uint8 tensor of 16-byte hpk_field records (view it with
        FIELD_DTYPE on the host): block b's are records field_off[b] .. field_off[b + 1]. str_off / str_end are the
        exact windows of the listed strings, block b's from str_blk_off[b]: decode_strings' inputs as they stand.
        status[b] is 0, or 5 for a block with bad offsets. The capacities are the tensors' sizes (fields.numel() //
        16 records, min(str_off, str_end) windows); what is allocated here holds len(blocks) of each, which always
        suffices. With sync=True a list that does not fit raises (HPK_E_NOSPACE)."""
        import torch

        n = int(block_off.shape[0]) - 1
        dev = blocks.device
        m = max(int(blocks.numel()), 1)
        if fields is None:
            fields = torch.empty(16 * m, dtype=torch.uint8, device=dev)
        if field_off is None:
            field_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if str_off is None:
            str_off = torch.empty(m, dtype=torch.int32, device=dev)
        if str_end is None:
            str_end = torch.empty(m, dtype=torch.int32, device=dev)
        if str_blk_off is None:
            str_blk_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        self._scan_blocks_call(blocks, block_off, fields, field_off, str_off, str_end, str_blk_off, status, True, sync)
        return fields, field_off, str_off, str_end, str_blk_off, status

    def scan_blocks_host(self, blocks, block_off, fields_cap=None, strs_cap=None):
        """hpk_scan_blocks with host pointers: numpy in -> (fields, field_off, str_off, str_end, str_blk_off,
        status), staged through the context and synchronous; fields is a FIELD_DTYPE record array. The offsets are
        checked before anything is copied. fields_cap / strs_cap: the lists' capacities (default: the blocks'
        bytes, which always suffice); the lists come back cut to their totals when they fit, and the call raises
        (HPK_E_NOSPACE) when one does not."""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        block_off = np.ascontiguousarray(block_off, dtype=U32)
        n = len(block_off) - 1
        fcap = int(blocks.size if fields_cap is None else fields_cap)
        scap = int(blocks.size if strs_cap is None else strs_cap)
        fields = np.zeros(16 * max(fcap, 1), dtype=np.uint8)[: 16 * fcap]
        str_off = np.zeros(max(scap, 1), dtype=U32)[:scap]
        str_end = np.zeros(max(scap, 1), dtype=U32)[:scap]
        field_off = np.zeros(n + 1, dtype=U32)
        str_blk_off = np.zeros(n + 1, dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)
        if blocks.size == 0:
            blocks = np.zeros(1, dtype=np.uint8)[:0]
        self._scan_blocks_call(blocks, block_off, fields, field_off, str_off, str_end, str_blk_off, status, False, True)
        nf, ns = int(field_off[n]), int(str_blk_off[n])
        return fields[: 16 * nf].view(FIELD_DTYPE), field_off, str_off[:ns], str_end[:ns], str_blk_off, status[:n]

    FRAME_SCANS = {"host": _lib.HPK_FRAME_SCAN_HOST, "device": _lib.HPK_FRAME_SCAN_DEVICE}

    def set_frame_scan(self, kind: str):
        """'host' (the default) or 'device' (hpk_ctx_set_frame_scan): where h2.read_frames does its framing with
        this codec. The same results and connection states; 'device' uploads the call's bytes with the pending
        connections' held fragments behind them and runs scan_frames' and frame_blocks' kernels before the blocks
        are decoded."""
        if kind not in self.FRAME_SCANS:
            raise ValueError(f"frame scan {kind!r} not in {tuple(self.FRAME_SCANS)}")
        _lib.check(self._L.hpk_ctx_set_frame_scan(self._h, self.FRAME_SCANS[kind]), "hpk_ctx_set_frame_scan")

    def _scan_frames_call(self, data, off, conns, blocks, conn_blk_off, frag_off, frag_len, conn_frag_off, open_off, open_len,
                          conn_open_off, device, sync):
        dev = self.device if device else None
        n = int(off.shape[0]) - 1
        if n < 0:
            raise ValueError("off needs nconn+1 >= 1 entries")
        pb, cap = _arg(data, "bytes", ("uint8",), 0, dev)
        po, _ = _arg(off, "off", _OFF_DTYPES, n + 1, dev)
        pc, _ = _arg(conns, "conns", ("uint8",), 32 * n, dev)
        pk, kbytes = _arg(blocks, "blocks", ("uint8",), 0, dev)
        pcb, _ = _arg(conn_blk_off, "conn_blk_off", _OFF_DTYPES, n + 1, dev)
        pfo, fobytes = _arg(frag_off, "frag_off", _OFF_DTYPES, 0, dev)
        pfl, flbytes = _arg(frag_len, "frag_len", _OFF_DTYPES, 0, dev)
        pcf, _ = _arg(conn_frag_off, "conn_frag_off", _OFF_DTYPES, n + 1, dev)
        poo, oobytes = _arg(open_off, "open_off", _OFF_DTYPES, 0, dev)
        pol, olbytes = _arg(open_len, "open_len", _OFF_DTYPES, 0, dev)
        pco, _ = _arg(conn_open_off, "conn_open_off", _OFF_DTYPES, n + 1, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        rc = self._L.hpk_scan_frames(self._h, pb, cap, po, ctypes.c_uint32(n), pc, pk, kbytes // 16, pcb, pfo, pfl,
                                     min(fobytes, flbytes) // 4, pcf, poo, pol, min(oobytes, olbytes) // 4, pco, flags)
        _lib.check(rc, "hpk_scan_frames")

    def scan_frames(self, data, off, conns, blocks=None, conn_blk_off=None, frag_off=None, frag_len=None, conn_frag_off=None,
                    open_off=None, open_len=None, conn_open_off=None, sync=False):
        """hpk_scan_frames: torch cuda tensors -> (blocks, conn_blk_off, frag_off, frag_len, conn_frag_off, open_off,
        open_len, conn_open_off); conns is updated in place. Connection c's bytes are data[off[c] : off[c + 1]] and
        its frame state the 32-byte hpk_fconn record conns[32 c : 32 c + 32] (a uint8 tensor: view it with
        FCONN_DTYPE on the host). blocks is a uint8 tensor of 16-byte hpk_fblock records (FBLOCK_DTYPE), one per
        header block completed in the call, connection c's from conn_blk_off[c]: block b's bytes are the closed
        fragments frag .. frag + nfrag, fragment g being data[frag_off[g] : frag_off[g] + frag_len[g]]. The open list
        holds the fragments of blocks still pending, connection c's from conn_open_off[c]: the next call's carry.
        The capacities are the tensors' sizes; what is allocated here holds (off[-1] - off[0]) // 9 blocks and that
        plus nconn fragments of either list, which always suffices (it reads off[0] and off[-1] back for that). With
        sync=True a list that does not fit raises (HPK_E_NOSPACE)."""
        import torch

        n = int(off.shape[0]) - 1
        dev = data.device
        if blocks is None or frag_off is None or frag_len is None or open_off is None or open_len is None:
            span = ((int(off[n].item()) & 0xFFFFFFFF) - (int(off[0].item()) & 0xFFFFFFFF)) if n > 0 else 0
            mb = max(span, 0) // 9
            mf = mb + max(n, 0)
        if blocks is None:
            blocks = torch.empty(16 * max(mb, 1), dtype=torch.uint8, device=dev)[: 16 * mb]
        if frag_off is None:
            frag_off = torch.empty(max(mf, 1), dtype=torch.int32, device=dev)[:mf]
        if frag_len is None:
            frag_len = torch.empty(max(mf, 1), dtype=torch.int32, device=dev)[:mf]
        if open_off is None:
            open_off = torch.empty(max(mf, 1), dtype=torch.int32, device=dev)[:mf]
        if open_len is None:
            open_len = torch.empty(max(mf, 1), dtype=torch.int32, device=dev)[:mf]
        if conn_blk_off is None:
            conn_blk_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if conn_frag_off is None:
            conn_frag_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if conn_open_off is None:
            conn_open_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        self._scan_frames_call(data, off, conns, blocks, conn_blk_off, frag_off, frag_len, conn_frag_off, open_off, open_len,
                               conn_open_off, True, sync)
        return blocks, conn_blk_off, frag_off, frag_len, conn_frag_off, open_off, open_len, conn_open_off

    def scan_frames_host(self, data, off, conns, blocks_cap=None, frags_cap=None, opens_cap=None):
        """hpk_scan_frames with host pointers: numpy in -> (conns, blocks, conn_blk_off, frag_off, frag_len,
        conn_frag_off, open_off, open_len, conn_open_off), staged through the context and synchronous. conns is an
        FCONN_DTYPE record array (a copy comes back updated), blocks an FBLOCK_DTYPE one. The offsets and the carry
        windows are checked before anything is copied. The capacities default to what always suffices; the lists come
        back cut to their totals when they fit, and the call raises (HPK_E_NOSPACE) when one does not."""
        data = np.ascontiguousarray(data, dtype=np.uint8)
        off = np.ascontiguousarray(off, dtype=U32)
        conns = np.array(conns, dtype=FCONN_DTYPE, copy=True)
        n = len(off) - 1
        if len(conns) != n:
            raise ValueError(f"conns: {len(conns)} records for {n} connections")
        span = int(off[n]) - int(off[0]) if n > 0 else 0
        mb = max(span, 0) // 9
        bcap = int(mb if blocks_cap is None else blocks_cap)
        fcap = int(mb + n if frags_cap is None else frags_cap)
        ocap = int(mb + n if opens_cap is None else opens_cap)
        blocks = np.zeros(16 * max(bcap, 1), dtype=np.uint8)[: 16 * bcap]
        fo, fl = np.zeros(max(fcap, 1), dtype=U32)[:fcap], np.zeros(max(fcap, 1), dtype=U32)[:fcap]
        oo, ol = np.zeros(max(ocap, 1), dtype=U32)[:ocap], np.zeros(max(ocap, 1), dtype=U32)[:ocap]
        cb, cf, co = np.zeros(n + 1, dtype=U32), np.zeros(n + 1, dtype=U32), np.zeros(n + 1, dtype=U32)
        if data.size == 0:
            data = np.zeros(1, dtype=np.uint8)[:0]
        raw = conns.view(np.uint8).reshape(-1) if n else np.zeros(1, dtype=np.uint8)[:0]
        self._scan_frames_call(data, off, raw, blocks, cb, fo, fl, cf, oo, ol, co, False, True)
        nb, nf, no = int(cb[n]), int(cf[n]), int(co[n])
        return conns, blocks[: 16 * nb].view(FBLOCK_DTYPE), cb, fo[:nf], fl[:nf], cf, oo[:no], ol[:no], co

    def frame_blocks(self, data, frag_off, frag_len, blocks, nblocks=None, out_blob=None, block_off=None, sync=False):
        """hpk_frame_blocks: torch cuda tensors -> (out_blob, block_off): scan_frames' closed fragments (all of
        frag_off / frag_len as given: cut them to the total) laid end to end in out_blob, block b's bytes being
        out_blob[block_off[b] : block_off[b + 1]]: scan_blocks' inputs as they stand. blocks is scan_frames' uint8
        tensor of hpk_fblock records, nblocks of them (default: all of the tensor). out_blob=None allocates data's
        size (fragments of a scan never sum to more), cut to the total when sync=True; capacity rules as pack."""
        import torch

        nf = int(frag_len.shape[0])
        nb = int(blocks.numel()) // 16 if nblocks is None else int(nblocks)
        dev = self.device
        pd, cap = _arg(data, "bytes", ("uint8",), 0, dev)
        pfo, _ = _arg(frag_off, "frag_off", _OFF_DTYPES, nf, dev)
        pfl, _ = _arg(frag_len, "frag_len", _OFF_DTYPES, nf, dev)
        pk, _ = _arg(blocks, "blocks", ("uint8",), 16 * nb, dev)
        own = out_blob is None
        if own:
            out_blob = torch.empty(max(int(data.numel()), 1), dtype=torch.uint8, device=data.device)
        if block_off is None:
            block_off = torch.empty(nb + 1, dtype=torch.int32, device=data.device)
        po, out_cap = _arg(out_blob, "out_blob", ("uint8",), 0, dev)
        pbo, _ = _arg(block_off, "block_off", _OFF_DTYPES, nb + 1, dev)
        self._follow()
        flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        rc = self._L.hpk_frame_blocks(self._h, pd, cap, pfo, pfl, ctypes.c_uint32(nf), pk, ctypes.c_uint32(nb), po, out_cap, pbo, flags)
        _lib.check(rc, "hpk_frame_blocks")
        if own and sync:
            out_blob = out_blob[: int(block_off[nb].item()) & 0xFFFFFFFF]
        return out_blob, block_off

    FRAME_WRITES = {"host": _lib.HPK_FRAME_WRITE_HOST, "device": _lib.HPK_FRAME_WRITE_DEVICE}

    def set_frame_write(self, kind: str):
        """'host' (the default) or 'device' (hpk_ctx_set_frame_write): where h2.write_headers frames the encoded
        blocks with this codec. The same octets; 'device' runs write_frames' kernels on the staged blocks, and a
        failure of that step is answered by the host framing."""
        if kind not in self.FRAME_WRITES:
            raise ValueError(f"frame write {kind!r} not in {tuple(self.FRAME_WRITES)}")
        _lib.check(self._L.hpk_ctx_set_frame_write(self._h, self.FRAME_WRITES[kind]), "hpk_ctx_set_frame_write")

    def _write_frames_call(self, blocks, block_off, stream_id, max_frame, out_blob, wire_off, status, device, sync):
        dev = self.device if device else None
        n = int(block_off.shape[0]) - 1
        if n < 0:
            raise ValueError("block_off needs nblocks+1 >= 1 entries")
        pb, cap = _arg(blocks, "blocks", ("uint8",), 0, dev)
        po, _ = _arg(block_off, "block_off", _OFF_DTYPES, n + 1, dev)
        ps, _ = _arg(stream_id, "stream_id", _OFF_DTYPES, n, dev)
        pm, _ = _arg(max_frame, "max_frame", _OFF_DTYPES, n, dev)
        pout, out_cap = _arg(out_blob, "out_blob", ("uint8",), 0, dev)
        pw, _ = _arg(wire_off, "wire_off", _OFF_DTYPES, n + 1, dev)
        pst, _ = _arg(status, "status", ("uint8",), n, dev)
        if device:
            self._follow()
            flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        else:
            flags = _lib.HPK_PTR_HOST
        rc = self._L.hpk_write_frames(self._h, pb, cap, po, ctypes.c_uint32(n), ps, pm, pout, out_cap, pw, pst, flags)
        _lib.check(rc, "hpk_write_frames")

    def write_frames(self, blocks, block_off, stream_id, max_frame, out_blob=None, wire_off=None, status=None, sync=False):
        """hpk_write_frames: torch cuda tensors -> (out_blob, wire_off, status). Block b is
        blocks[block_off[b] : block_off[b + 1]]; it goes out as one HEADERS frame and the CONTINUATION frames that
        max_frame[b] (the peer's SETTINGS_MAX_FRAME_SIZE) demands, on stream stream_id[b] (bit 31: END_STREAM on the
        HEADERS frame, scan_frames' convention), at out_blob[wire_off[b] : wire_off[b + 1]]. out_blob=None allocates
        what always suffices when every frame size is at least 16 (blocks' size + 9 octets per 16 of it and per
        block), cut to the total when sync=True; pass one for smaller frame sizes. Capacity rules as encode_packed:
        the octets below the capacity are written, and with sync=True a total past it raises (HPK_E_NOSPACE)."""
        import torch

        n = int(block_off.shape[0]) - 1
        dev = blocks.device
        own = out_blob is None
        if own:
            size = int(blocks.numel())
            out_blob = torch.empty(max(size + 9 * (size // 16 + max(n, 0) + 1), 1), dtype=torch.uint8, device=dev)
        if wire_off is None:
            wire_off = torch.empty(n + 1, dtype=torch.int32, device=dev)
        if status is None:
            status = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)[: max(n, 0)]
        self._write_frames_call(blocks, block_off, stream_id, max_frame, out_blob, wire_off, status, True, sync)
        if own and sync:
            out_blob = out_blob[: int(wire_off[n].item()) & 0xFFFFFFFF]
        return out_blob, wire_off, status

    def write_frames_host(self, blocks, block_off, stream_id, max_frame, out_cap=None):
        """hpk_write_frames with host pointers: numpy in -> (out_blob, wire_off, status), staged through the context
        and synchronous. The offsets and the frame sizes are checked before anything is copied. out_cap defaults to
        the wire total (computed here); with a smaller one the call raises (HPK_E_NOSPACE)."""
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8)
        block_off = np.ascontiguousarray(block_off, dtype=U32)
        stream_id = np.ascontiguousarray(stream_id, dtype=U32)
        max_frame = np.ascontiguousarray(max_frame, dtype=U32)
        n = len(block_off) - 1
        if out_cap is None:
            lens = np.diff(block_off.astype(np.int64))
            m = np.maximum(max_frame.astype(np.int64), 1)
            out_cap = int((lens + 9 * np.maximum(-(-lens // m), 1)).sum()) if n > 0 else 0
        out = np.zeros(max(int(out_cap), 1), dtype=np.uint8)[: int(out_cap)]
        wire_off = np.zeros(n + 1, dtype=U32)
        status = np.zeros(max(n, 1), dtype=np.uint8)[: max(n, 0)]
        if blocks.size == 0:
            blocks = np.zeros(1, dtype=np.uint8)[:0]
        self._write_frames_call(blocks, block_off, stream_id, max_frame, out, wire_off, status, False, True)
        return out[: int(wire_off[n])], wire_off, status

    BLOCK_APPLIES = {"host": _lib.HPK_BLOCK_APPLY_HOST, "device": _lib.HPK_BLOCK_APPLY_DEVICE}

    def set_block_apply(self, kind: str):
        """'host' (the default) or 'device' (hpk_ctx_set_block_apply): where hpack.decode_blocks and
        h2.read_frames apply this codec's header blocks against the decoders' tables. 'device' selects the whole
        device pipeline whatever set_block_scan says: scan_blocks' kernels, decode_strings' pipeline and
        apply_blocks' kernel, the tables carried to the device and back. The same results and decoder states."""
        if kind not in self.BLOCK_APPLIES:
            raise ValueError(f"block apply {kind!r} not in {tuple(self.BLOCK_APPLIES)}")
        _lib.check(self._L.hpk_ctx_set_block_apply(self._h, self.BLOCK_APPLIES[kind]), "hpk_ctx_set_block_apply")

    def apply_blocks(self, fields, field_off, str_out_off, str_out_len, str_status, nstrs, str_base, static_base, dec_blk_off,
                     dec_blk, tabs, tab_ent, headers=None, results=None, sync=False):
        """hpk_apply_blocks: torch cuda tensors -> (headers, results); tabs and tab_ent are updated in place.
        fields / field_off are scan_blocks' outputs, str_out_off / str_out_len / str_status decode_strings' for the
        scan's string list (nstrs of them). Every offset is into one arena the caller defines and the call never
        reads: the static text (static_table()) at static_base, string s at str_base + str_out_off[s], the
        carried-in table entries wherever tab_ent says. Decoder d applies blocks dec_blk[dec_blk_off[d] :
        dec_blk_off[d + 1]] in order against tabs[d] (a uint8 tensor of 32-byte hpk_dtab records: view it with
        DTAB_DTYPE on the host), whose entries are the 16-byte hpk_header records tab_ent[ent : ent + count],
        newest first (tab_ent: a uint8 tensor, HEADER_DTYPE). headers (uint8, 16 bytes per record; capacity
        headers.numel() // 16, by default fields' record count) gets block b's headers at records field_off[b] ..
        field_off[b] + n_headers; results (uint8, 16 bytes per block, RESULT_DTYPE) the blocks' first_header,
        n_headers, error and detail. error 10 (HPK_BLK_DEFERRED): the block was not applied, tabs[d]['applied'] says
        how many of the decoder's list were. With sync=True bad inputs raise (HPK_E_INVAL), and so does a field total
        above the headers' capacity (HPK_E_NOSPACE)."""
        import torch

        dev = self.device
        n = int(field_off.shape[0]) - 1
        nd = int(dec_blk_off.shape[0]) - 1
        if n < 0 or nd < 0:
            raise ValueError("field_off and dec_blk_off need n+1 >= 1 entries")
        if headers is None:
            headers = torch.empty(max(int(fields.numel()), 16), dtype=torch.uint8, device=fields.device)[: int(fields.numel())]
        if results is None:
            results = torch.empty(16 * max(n, 1), dtype=torch.uint8, device=fields.device)
        pf, fbytes = _arg(fields, "fields", ("uint8",), 0, dev)
        pfo, _ = _arg(field_off, "field_off", _OFF_DTYPES, n + 1, dev)
        poo, _ = _arg(str_out_off, "str_out_off", _OFF_DTYPES, nstrs, dev)
        pol, _ = _arg(str_out_len, "str_out_len", _OFF_DTYPES, nstrs, dev)
        pst, _ = _arg(str_status, "str_status", ("uint8",), nstrs, dev)
        pdo, _ = _arg(dec_blk_off, "dec_blk_off", _OFF_DTYPES, nd + 1, dev)
        pdb, _ = _arg(dec_blk, "dec_blk", _OFF_DTYPES, 0, dev)
        pt, tbytes = _arg(tabs, "tabs", ("uint8",), 32 * nd, dev)
        pe, ebytes = _arg(tab_ent, "tab_ent", ("uint8",), 0, dev)
        ph, hbytes = _arg(headers, "headers", ("uint8",), 0, dev)
        pr, _ = _arg(results, "results", ("uint8",), 16 * n, dev)
        self._follow()
        flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        rc = self._L.hpk_apply_blocks(self._h, pf, pfo, ctypes.c_uint32(n), poo, pol, pst, ctypes.c_uint32(int(nstrs)),
                                      ctypes.c_uint32(int(str_base)), ctypes.c_uint32(int(static_base)), pdo, pdb,
                                      ctypes.c_uint32(nd), pt, pe, ebytes // 16, ph, hbytes // 16, pr, flags)
        _lib.check(rc, "hpk_apply_blocks")
        return headers, results

    BLOCK_PLANS = {"host": _lib.HPK_BLOCK_PLAN_HOST, "device": _lib.HPK_BLOCK_PLAN_DEVICE}

    def set_block_plan(self, kind: str):
        """'host' (the default) or 'device' (hpk_ctx_set_block_plan): where hpack.encode_blocks runs this codec's
        table logic. 'device' selects the whole device pipeline: plan_blocks' kernels against the encoders' tables
        carried to the device and back, pack's kernels over the items, encode_strings' steps. The same bytes and
        encoder states; a call holding an encoder whose table the device's ring cannot hold is answered by the
        host path."""
        if kind not in self.BLOCK_PLANS:
            raise ValueError(f"block plan {kind!r} not in {tuple(self.BLOCK_PLANS)}")
        _lib.check(self._L.hpk_ctx_set_block_plan(self._h, self.BLOCK_PLANS[kind]), "hpk_ctx_set_block_plan")

    def plan_blocks(self, arena, static_base, fields_base, prefix_base, field_off, hdr_off, enc_blk_off, enc_blk, enc_flags, tabs,
                    tab_ent, reps=None, item_off=None, item_len=None, item_policy=None, sync=False):
        """hpk_plan_blocks: torch cuda tensors -> (reps, item_off, item_len, item_policy); tabs, tab_ent and the
        arena's prefix area are updated in place. The encoder's table half for many encoders at once: arena (uint8)
        holds the static text (static_table()) at static_base, the headers' names and values end to end at
        fields_base (header j's name arena[fields_base + field_off[2j] : fields_base + field_off[2j + 1]], its value
        the next span; field_off has 2 * headers + 1 entries), 4 bytes per header at prefix_base for the
        representations' first octets, and the bytes of the carried-in table entries wherever tab_ent says. Block b
        is headers hdr_off[b] : hdr_off[b + 1]; encoder e plans blocks enc_blk[enc_blk_off[e] : enc_blk_off[e + 1]]
        in order against tabs[e] (32-byte hpk_dtab records, DTAB_DTYPE; entries 16-byte hpk_header records,
        HEADER_DTYPE, newest first); enc_flags[e] & 1: the encoder Huffman-codes. reps (uint8, 16 bytes per header,
        HREP_DTYPE) gets each header's kind, index and prefix octets; items 3j .. 3j + 2 of item_off / item_len /
        item_policy are header j's prefix octets and strings, pack()'s and encode_strings()' inputs as they stand.
        tabs[e]['applied'] says how many of the encoder's blocks were planned (0: deferred to the host). With
        sync=True bad inputs raise (HPK_E_INVAL)."""
        import torch

        dev = self.device
        nh = (int(field_off.shape[0]) - 1) // 2
        n = int(hdr_off.shape[0]) - 1
        ne = int(enc_blk_off.shape[0]) - 1
        if nh < 0 or n < 0 or ne < 0:
            raise ValueError("field_off, hdr_off and enc_blk_off need at least one entry")
        if reps is None:
            reps = torch.empty(16 * max(nh, 1), dtype=torch.uint8, device=arena.device)[: 16 * nh]
        if item_off is None:
            item_off = torch.empty(max(3 * nh, 1), dtype=torch.int32, device=arena.device)
        if item_len is None:
            item_len = torch.empty(max(3 * nh, 1), dtype=torch.int32, device=arena.device)
        if item_policy is None:
            item_policy = torch.empty(max(3 * nh, 1), dtype=torch.uint8, device=arena.device)
        pa, abytes = _arg(arena, "arena", ("uint8",), 0, dev)
        pfo, _ = _arg(field_off, "field_off", _OFF_DTYPES, 2 * nh + 1, dev)
        pho, _ = _arg(hdr_off, "hdr_off", _OFF_DTYPES, n + 1, dev)
        peo, _ = _arg(enc_blk_off, "enc_blk_off", _OFF_DTYPES, ne + 1, dev)
        peb, _ = _arg(enc_blk, "enc_blk", _OFF_DTYPES, 0, dev)
        pef, _ = _arg(enc_flags, "enc_flags", ("uint8",), ne, dev)
        pt, _ = _arg(tabs, "tabs", ("uint8",), 32 * ne, dev)
        pe, ebytes = _arg(tab_ent, "tab_ent", ("uint8",), 0, dev)
        pr, _ = _arg(reps, "reps", ("uint8",), 16 * nh, dev)
        pio, _ = _arg(item_off, "item_off", _OFF_DTYPES, 3 * nh, dev)
        pil, _ = _arg(item_len, "item_len", _OFF_DTYPES, 3 * nh, dev)
        pip, _ = _arg(item_policy, "item_policy", ("uint8",), 3 * nh, dev)
        self._follow()
        flags = _lib.HPK_PTR_DEVICE | (0 if sync else _lib.HPK_ASYNC)
        rc = self._L.hpk_plan_blocks(self._h, pa, abytes, ctypes.c_uint32(int(static_base)), ctypes.c_uint32(int(fields_base)),
                                     ctypes.c_uint32(int(prefix_base)), pfo, pho, ctypes.c_uint32(n), nh, peo, peb, pef,
                                     ctypes.c_uint32(ne), pt, pe, ebytes // 16, pr, pio, pil, pip, flags)
        _lib.check(rc, "hpk_plan_blocks")
        return reps, item_off, item_len, item_policy


def static_table():
    """hpk_static_table: RFC 7541 App. A as apply_blocks' kernel sees it -> (text, entries): the 61 names and
    values end to end (bytes) and a HEADER_DTYPE array of 61 records with offsets relative to the text."""
    L = _lib.lib()
    text, ent, ln = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    _lib.check(L.hpk_static_table(ctypes.byref(text), ctypes.byref(ln), ctypes.byref(ent)), "hpk_static_table")
    return ctypes.string_at(text.value, ln.value), np.frombuffer(ctypes.string_at(ent.value, 61 * 16), dtype=HEADER_DTYPE).copy()


def _bound_offsets_torch(in_off, num, den, add):
    import torch

    o = in_off.to(torch.int64)
    b = (((o[1:] - o[:-1]) * num + add) // den + 3) & ~3
    out = torch.zeros_like(o)
    torch.cumsum(b, 0, out=out[1:])
    if int(out[-1].item()) >= 2**32:
        raise ValueError("bound of the shard exceeds 4 GiB")
    return out.to(torch.int32) if int(out[-1].item()) < 2**31 else out.to(torch.uint32)


def compact_capacity(in_cap, n):
    """Output bytes hpk_decode_batch_compact needs: hpk_decoded_bound(in_cap) + 4 n."""
    return (8 * int(in_cap)) // 5 + 4 * int(n)


def decode_offsets_torch(in_off):
    return _bound_offsets_torch(in_off, 8, 5, 0)


def encode_offsets_torch(in_off):
    return _bound_offsets_torch(in_off, 30, 8, 7)


def _cpu_batch(fn_name, bound, in_blob, in_off, nthreads):
    L = _lib.lib()
    in_blob = np.ascontiguousarray(in_blob, dtype=np.uint8)
    in_off = np.ascontiguousarray(in_off, dtype=U32)
    out_off = bound(in_off)
    n = len(in_off) - 1
    out_blob = np.zeros(max(int(out_off[-1]), 1), dtype=np.uint8)
    out_len = np.zeros(max(n, 1), dtype=U32)
    status = np.zeros(max(n, 1), dtype=np.uint8)
    src = in_blob if in_blob.size else np.zeros(1, dtype=np.uint8)
    rc = getattr(L, fn_name)(src.ctypes.data, in_off.ctypes.data, n, out_blob.ctypes.data, out_off.ctypes.data,
                             out_len.ctypes.data, status.ctypes.data, int(nthreads))
    _lib.check(rc, fn_name)
    return out_blob, out_off, out_len[:n], status[:n]


def decode_batch_cpu(in_blob, in_off, nthreads=0):
    """The library's table-driven CPU batch decode (hpk_decode_batch_cpu): same layout and
    results as the device path, host threads over byte-balanced shards."""
    return _cpu_batch("hpk_decode_batch_cpu", decode_offsets_np, in_blob, in_off, nthreads)


def encode_batch_cpu(in_blob, in_off, nthreads=0):
    return _cpu_batch("hpk_encode_batch_cpu", encode_offsets_np, in_blob, in_off, nthreads)
