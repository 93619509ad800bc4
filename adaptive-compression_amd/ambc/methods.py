"""CompressionMethod plugins (the reference's operator interface).

Same contract as compression_methods.py:7-67: ``type_id``,
``compress(data) -> bytes``, ``decompress(data, original_length) -> bytes``,
``should_use(data, threshold=0.9) -> bool``, ``calculate_overhead() -> int``,
exceptions raised like the reference's.

* ids 1, 2, 3, 4, 9 (RLE, Dictionary, Huffman, Delta, LZ4) and 255 run on the
  GPU through libambc_hip (single-chunk calls of the same kernels the batched
  path uses; Dictionary emits the reference's own bytes for any window,
  lookahead and length);
* ids 5, 6, 7 are the reference's own stdlib library wrappers
  (advanced_compression.py:71-213) and id 8 its zstandard wrapper (:219-261,
  here over the system libzstd), registered so that reference-produced files
  holding such chunks decode.  When id 5 is among ``methods`` the batched engine
  selects and encodes it on the GPU with "ambc-deflate v1" (k_deflate: a valid
  zlib stream that this wrapper and the reference decode, not zlib level-9
  bytes); the per-chunk plugin itself keeps the reference's zlib.compress.

The batched engine (compressor.py) does not call these per chunk: it makes one
C-ABI call for the whole body.
"""
import bz2
import ctypes as C
import lzma
import operator
import os
import queue
import struct
import threading
import zlib
from abc import ABC, abstractmethod

import numpy as np

from . import _lib
from .container import MARKER_BYTES

_HDR = struct.Struct("<BBIII")
_END = MARKER_BYTES + b"\x00\x00" + b"\x00\x00" + b"\x00" * 8


class CompressionMethod(ABC):
    """compression_methods.py:7-67"""

    @property
    @abstractmethod
    def type_id(self):
        ...

    @abstractmethod
    def compress(self, data):
        ...

    @abstractmethod
    def decompress(self, data, original_length):
        ...

    def should_use(self, data, threshold=0.9):
        return True

    def calculate_overhead(self):
        return 0


def _ctx():
    return _lib.plugin_context()


def _gpu_encode_any(mid, data):
    """method.compress(data) past one chunk (RLE / Huffman / Delta / LZ4 at any
    length: ambc_encode_any, ambc_anylen.hip)."""
    n = len(data)
    ctx = _ctx()
    cap = 2 * n + 1344 if mid != 9 else n + n // 255 + 64 + 4 * (n // 65536 + 1)
    out = (C.c_uint8 * cap)()
    olen = C.c_uint64()
    with ctx.lock:
        rc = ctx.lib.ambc_encode_any(ctx.h, mid, _lib.addr(data), n, C.addressof(out), cap, C.byref(olen))
    if rc == _lib.AMBC_E_CODEC:
        raise ValueError(f"method {mid} cannot encode this input")
    if rc == _lib.AMBC_E_RANGE:
        # compression_methods.py:397: num_bits.to_bytes(4, 'little') past 2^32 bits
        raise OverflowError("int too big to convert")
    _lib.check(rc, ctx.lib)
    return C.string_at(C.addressof(out), olen.value)


def _gpu_encode(mid, data):
    data = bytes(data)
    n = len(data)
    if n == 0:
        return b""
    if n > _lib.MAX_CHUNK:
        return _gpu_encode_any(mid, data)
    ctx = _ctx()
    cap = 2 * n + 1344                    # RLE worst case 2n; Huffman table + ~1.13n bits
    out = (C.c_uint8 * cap)()
    olen = C.c_uint32()
    with ctx.lock:
        rc = ctx.lib.ambc_encode_method(ctx.h, mid, _lib.addr(data), n, C.addressof(out), cap,
                                        C.byref(olen))
    if rc == _lib.AMBC_E_CODEC:
        # the reference raises here (Huffman on 1 or 256 distinct symbols)
        raise ValueError(f"method {mid} cannot encode this input")
    _lib.check(rc, ctx.lib)
    return C.string_at(C.addressof(out), olen.value)


def _gpu_encode_lz4hc(data):
    """LZ4Compression(level="hc").compress: one chunk's "ambc-lz4 hc v1" frame."""
    data = bytes(data)
    n = len(data)
    if n == 0:
        return b""
    if n > _lib.LZ4HC_MAX_CHUNK:
        raise ValueError(f"LZ4Compression(level='hc') takes at most {_lib.LZ4HC_MAX_CHUNK} bytes (got {n})")
    ctx = _ctx()
    cap = n + 64
    out = (C.c_uint8 * cap)()
    olen = C.c_uint32()
    with ctx.lock:
        rc = ctx.lib.ambc_encode_method_ex(ctx.h, 9, _lib.FLAG_LZ4HC, _lib.addr(data), n, C.addressof(out), cap,
                                           C.byref(olen))
    _lib.check(rc, ctx.lib)
    return C.string_at(C.addressof(out), olen.value)


def _gpu_should_use(data):
    """should_use bits from the selector kernels: {1: RLE, 2: Dictionary, 3: Huffman, 4: Delta}."""
    data = bytes(data)
    n = len(data)
    if n == 0:
        return {1: False, 2: False, 3: False, 4: False}
    if n > _lib.MAX_CHUNK:
        return _gpu_should_use_any(data)
    from .compressor import entropy_terms
    ctx = _ctx()
    p = _lib.Params()
    p.chunk_size = (n + 15) & ~15
    p.method_mask = (1 << 1) | (1 << 3)
    for i in range(16):
        p.pref_min[i], p.pref_max[i] = 0, 0xFFFFFFFF
    tail = entropy_terms(n)
    p.ent_full = tail.ctypes.data if n == p.chunk_size else None
    p.ent_tail = tail.ctypes.data if n != p.chunk_size else None
    ids = (C.c_uint8 * 1)()
    pl = (C.c_uint32 * 1)()
    su = (C.c_uint8 * 1)()
    with ctx.lock:
        _lib.check(ctx.lib.ambc_analyze(ctx.h, _lib.addr(data), n, C.byref(p), C.addressof(ids),
                                        C.addressof(pl), C.addressof(su)), ctx.lib)
    return {1: bool(su[0] & 2), 2: bool(su[0] & 4), 3: bool(su[0] & 8), 4: bool(su[0] & 16)}


def _gpu_decode(mid, data, original_length):
    """method.decompress through the batched GPU decoder (one package).  The
    output is sized max(orig, 1): Huffman appends a symbol before it compares the
    length with original_length (compression_methods.py:462-468), so orig 0 still
    yields one byte; the other codecs produce nothing there."""
    data = bytes(data)
    body = MARKER_BYTES + _HDR.pack(mid, 0, original_length, original_length, len(data)) + data + _END
    ctx = _ctx()
    osz = max(1, original_length)
    out = (C.c_uint8 * osz)()
    st = _lib.Stats()
    reg = (C.c_uint64 * 4)()
    for t in (1, 2, 3, 4, 9, 255):
        reg[t >> 6] |= 1 << (t & 63)
    nh = C.c_uint32()
    with ctx.lock:
        _lib.check(ctx.lib.ambc_decompress_ex(ctx.h, _lib.addr(body), len(body), osz, reg,
                                              C.addressof(out), None, 0, C.byref(nh), C.byref(st)),
                   ctx.lib)
    produced = min(int(st.payload_bytes), osz)
    return C.string_at(C.addressof(out), produced)


def _gpu_should_use_any(data):
    """should_use past one chunk: the device's statistics (ambc_analyze_any: the
    sampled pairs of RLE / Delta, the byte counts and first positions), the
    reference's comparisons on them -- RLE (compression_methods.py:166-180) and
    Delta (:652-667) over 1000 samples, Huffman's entropy summed in Counter order
    with numpy's log2 (:562-574, the same float operations), Dictionary from the
    first 1003 bytes (:329-343 read no more)."""
    n = len(data)
    ctx = _ctx()
    step = max(1, n // 1000)
    st = (C.c_uint32 * 514)()
    with ctx.lock:
        _lib.check(ctx.lib.ambc_analyze_any(ctx.h, _lib.addr(data), n, step, st), ctx.lib)
    ss = min(1000, n)
    rle = n >= 4 and st[0] / (ss - 1) > 0.3
    delta = n >= 4 and st[1] / (ss - 1) > 0.5
    huff = False
    if n >= 100:
        present = sorted((st[258 + b], st[2 + b]) for b in range(256) if st[2 + b])
        entropy = 0
        for _, count in present:
            p = count / n
            entropy -= p * np.log2(p)
        huff = bool(entropy < 7.0)
    return {1: bool(rle), 2: _gpu_should_use(bytes(data[:1003]))[2], 3: huff, 4: bool(delta)}


class RLECompression(CompressionMethod):
    """compression_methods.py:70-180 on the GPU."""
    type_id = 1

    def compress(self, data):
        return _gpu_encode(1, data)

    def decompress(self, data, original_length):
        if not data:
            return b""
        return _gpu_decode(1, data, original_length)

    def should_use(self, data, threshold=0.9):
        return _gpu_should_use(data)[1]


def _gpu_dict_any(data, window, look):
    """DictionaryCompression(window, look).compress(data) on k_da_* (any window,
    lookahead and length)."""
    ctx = _ctx()
    n = len(data)
    cap = 2 * n + 16                      # every token covers >= 1 byte with <= 2 bytes per byte
    out = (C.c_uint8 * cap)()
    olen = C.c_uint64()
    clamp = lambda v: max(-(1 << 62), min(1 << 62, v))
    with ctx.lock:
        rc = ctx.lib.ambc_dict_encode(ctx.h, _lib.addr(data), n, clamp(window), clamp(look),
                                      C.addressof(out), cap, C.byref(olen))
    if rc == _lib.AMBC_E_CODEC:
        # compression_methods.py:227: bytearray.append(match_len) with a match > 255 bytes
        raise ValueError("byte must be in range(0, 256)")
    _lib.check(rc, ctx.lib)
    return C.string_at(C.addressof(out), olen.value)


class DictionaryCompression(CompressionMethod):
    """compression_methods.py:183-343 on the GPU, byte for byte.  The reference's
    defaults (window 4096, lookahead 32) on inputs up to 8192 bytes -- the
    method's preferred maximum chunk -- run k_dict (the batched engine's kernel);
    any other window, lookahead or length runs k_da_* (ambc_dictany.hip).  The
    window and lookahead must be integers (operator.index; the reference's own
    arithmetic raises TypeError for most other values as well)."""
    type_id = 2

    def __init__(self, window_size=4096, lookahead_size=32):
        self.window_size = window_size
        self.lookahead_size = lookahead_size

    def compress(self, data):
        data = bytes(data)
        if not data:
            return b""
        window = operator.index(self.window_size)
        look = operator.index(self.lookahead_size)
        if (window, look) == (4096, 32) and len(data) <= 8192:
            return _gpu_encode(2, data)
        return _gpu_dict_any(data, window, look)

    def decompress(self, data, original_length):
        if not data:
            return b""
        return _gpu_decode(2, data, original_length)

    def should_use(self, data, threshold=0.9):
        # :315-343 reads the first min(n, 1003) bytes, and from n >= 1003 on the
        # same 1000 3-grams over a 1000-byte sample: the prefix decides
        return _gpu_should_use(bytes(data[:1003]))[2]


class HuffmanCompression(CompressionMethod):
    """compression_methods.py:346-574 on the GPU."""
    type_id = 3

    def compress(self, data):
        return _gpu_encode(3, data)

    def decompress(self, data, original_length):
        if not data:
            return b""
        return _gpu_decode(3, data, original_length)

    def should_use(self, data, threshold=0.9):
        return _gpu_should_use(data)[3]


class DeltaCompression(CompressionMethod):
    """compression_methods.py:577-667 on the GPU (never selected: len == n)."""
    type_id = 4

    def compress(self, data):
        return _gpu_encode(4, data)

    def decompress(self, data, original_length):
        if not data:
            return b""
        return _gpu_decode(4, data, original_length)

    def should_use(self, data, threshold=0.9):
        return _gpu_should_use(data)[4]


class LZ4Compression(CompressionMethod):
    """advanced_compression.py:266-307 -- LZ4 frame from the gfx950 encoder
    ("ambc-lz4 greedy v2" block parse, LZ4F one-block frame layout).
    level="hc": "ambc-lz4 hc v1" (hash chains, lazy parse) for inputs up to 16384
    bytes; longer inputs raise ValueError (the any-length path is greedy only)."""
    type_id = 9

    def __init__(self, level="greedy"):
        if level not in ("greedy", "hc"):
            raise ValueError("level must be 'greedy' or 'hc'")
        self.level = level

    def compress(self, data):
        if self.level == "hc":
            return _gpu_encode_lz4hc(data)
        return _gpu_encode(9, data)

    def decompress(self, data, original_length):
        if not data:
            return b""
        return _gpu_decode(9, data, original_length)

    def should_use(self, data, threshold=0.9):
        # advanced_compression.py:298-307: entropy > 8.1 is impossible for bytes
        return len(data) >= 1024


class NoCompression(CompressionMethod):
    """compression_methods.py:670-713"""
    type_id = 255

    def compress(self, data):
        return bytes(data)

    def decompress(self, data, original_length):
        if len(data) < original_length:
            return bytes(data) + b"\x00" * (original_length - len(data))
        return bytes(data[:original_length])


# ---- the reference's stdlib library wrappers (decode of ids 5/6/7; ids 6/7 --
# bz2 / lzma, no GPU encoder -- also host-scored in the walk, hostcodecs.py) ----
def _fit(b, n):
    return b[:n] if len(b) > n else b + bytes(n - len(b))


def calculate_entropy(data):
    """advanced_compression.py:48-57: numpy's Shannon entropy of the byte counts,
    in the same order of operations (the should_use gates compare it with 7.7 / 8.0)."""
    if not data:
        return 0.0
    counts = np.bincount(np.frombuffer(bytes(data), dtype=np.uint8), minlength=256)
    probs = counts / len(data)
    probs = probs[probs > 0]
    return -np.sum(probs * np.log2(probs))


class DeflateCompression(CompressionMethod):
    """advanced_compression.py:71-107"""
    type_id = 5

    def compress(self, data, level=9):
        return zlib.compress(data, level=level) if data else b""

    def should_use(self, data, threshold=0.9):
        # advanced_compression.py:98-107
        return len(data) >= 64 and calculate_entropy(data) < 8.0

    def decompress(self, data, original_length):
        if not data:
            return b""
        try:
            return _fit(zlib.decompress(data), original_length)
        except Exception:  # noqa: BLE001 -- reference returns zeros on error
            return bytes(original_length)


class Bzip2Compression(CompressionMethod):
    """advanced_compression.py:112-150"""
    type_id = 6

    def compress(self, data, level=9):
        return bz2.compress(data, compresslevel=level) if data else b""

    def should_use(self, data, threshold=0.9):
        # advanced_compression.py:139-150
        return len(data) >= 1024 and calculate_entropy(data) < 7.7

    def decompress(self, data, original_length):
        if not data:
            return b""
        try:
            return _fit(bz2.decompress(data), original_length)
        except Exception:  # noqa: BLE001
            return bytes(original_length)


class _XZEncoders:
    """The reference's LZMA call -- ``lzma.LZMACompressor(format=FORMAT_XZ,
    check=CHECK_CRC64, filters=[{"id": FILTER_LZMA2, "dict_size": 1 << 24}])``,
    advanced_compression.py:163-182 -- made through the liblzma that Python's
    own ``_lzma`` module links, on encoders that are kept and re-initialised
    instead of built per call: a fresh encoder faults in ~190 MiB of match-finder
    state each time (8 KiB chunk: 25 -> 10 ms; the walk scores LZMA at every
    candidate size of 8 KiB and more).  Same library, same filter chain (preset
    6 with the 16 MiB dictionary: what _lzma builds from that spec), same
    check, one LZMA_FINISH pass: the same bytes -- checked against Python's lzma
    on a probe when the pool is first used; a mismatch (or no liblzma) leaves
    Python's lzma in charge.  At most size() encoders exist -- set by a memory
    budget (AMBC_LZMA_MEM bytes, default a quarter of the host's memory capped at
    8 GiB, ~190 MiB per encoder), at most 64 -- and a caller waits for one (the
    Python fallback is bounded the same way).  release() ends the idle encoders
    (lzma_end): the host scorer calls it when a walk is done, so the ~190 MiB each
    are not kept between calls."""

    ENC_BYTES = 190 << 20

    class _Stream(C.Structure):          # lzma_stream (LZMA_STREAM_INIT: all zeros)
        _fields_ = [("next_in", C.c_void_p), ("avail_in", C.c_size_t), ("total_in", C.c_uint64),
                    ("next_out", C.c_void_p), ("avail_out", C.c_size_t), ("total_out", C.c_uint64),
                    ("allocator", C.c_void_p), ("internal", C.c_void_p), ("reserved", C.c_uint8 * 128)]

    class _Filter(C.Structure):          # lzma_filter
        _fields_ = [("id", C.c_uint64), ("options", C.c_void_p)]

    _pool = None
    _lock = threading.Lock()
    _size = None
    _sem = None

    @classmethod
    def size(cls):
        """encoders at once, from the memory budget"""
        if cls._size is None:
            budget = os.environ.get("AMBC_LZMA_MEM")
            if budget:
                budget = int(budget)
            else:
                try:
                    phys = os.sysconf("SC_PHYS_PAGES") * os.sysconf("SC_PAGE_SIZE")
                except (ValueError, OSError):
                    phys = 8 << 30
                budget = min(8 << 30, phys // 4)
            cls._size = max(1, min(64, budget // cls.ENC_BYTES))
            cls._sem = threading.BoundedSemaphore(cls._size)
        return cls._size

    @classmethod
    def pool(cls):
        """the encoder pool, or None when the liblzma path is unavailable"""
        with cls._lock:
            cls.size()
            if cls._pool is None:
                cls._pool = False
                try:
                    lib = C.CDLL("liblzma.so.5")
                    lib.lzma_lzma_preset.argtypes = [C.c_void_p, C.c_uint32]
                    lib.lzma_lzma_preset.restype = C.c_int
                    lib.lzma_stream_encoder.argtypes = [C.POINTER(cls._Stream), C.c_void_p, C.c_int]
                    lib.lzma_stream_encoder.restype = C.c_int
                    lib.lzma_code.argtypes = [C.POINTER(cls._Stream), C.c_int]
                    lib.lzma_code.restype = C.c_int
                    lib.lzma_stream_buffer_bound.argtypes = [C.c_size_t]
                    lib.lzma_stream_buffer_bound.restype = C.c_size_t
                    lib.lzma_end.argtypes = [C.POINTER(cls._Stream)]
                    cls.lib = lib
                    free = queue.LifoQueue()
                    for _ in range(cls._size):
                        free.put(cls())
                    probe = bytes(range(256)) * 40 + b"abcabcabd" * 300
                    if cls._encode(free, probe) == cls._python(probe):
                        cls._pool = free
                except (OSError, AttributeError, RuntimeError):
                    cls._pool = False
            return cls._pool or None

    def __init__(self):
        lib = type(self).lib
        self.opt = (C.c_uint8 * 512)()        # lzma_options_lzma (and slack)
        if lib.lzma_lzma_preset(self.opt, 6):
            raise RuntimeError("lzma_lzma_preset")
        C.c_uint32.from_buffer(self.opt, 0).value = 1 << 24     # dict_size, the struct's first field
        self.flt = (self._Filter * 2)(self._Filter(0x21, C.addressof(self.opt)),   # LZMA_FILTER_LZMA2
                                      self._Filter((1 << 64) - 1, None))           # LZMA_VLI_UNKNOWN
        self.strm = self._Stream()

    def end(self):
        """free the encoder's state (lzma_end); the next run() builds it again"""
        type(self).lib.lzma_end(C.byref(self.strm))
        self.strm = self._Stream()

    def run(self, data):
        lib = type(self).lib
        if lib.lzma_stream_encoder(C.byref(self.strm), self.flt, 4):      # LZMA_CHECK_CRC64
            raise RuntimeError("lzma_stream_encoder")
        cap = lib.lzma_stream_buffer_bound(len(data))
        out = C.create_string_buffer(cap)
        src = C.c_char_p(data)
        self.strm.next_in, self.strm.avail_in = C.cast(src, C.c_void_p), len(data)
        self.strm.next_out, self.strm.avail_out = C.addressof(out), cap
        if lib.lzma_code(C.byref(self.strm), 3) != 1:                    # LZMA_FINISH -> LZMA_STREAM_END
            raise RuntimeError("lzma_code")
        return out.raw[:cap - self.strm.avail_out]

    @staticmethod
    def _encode(free, data):
        enc = free.get()
        try:
            return enc.run(data)
        finally:
            free.put(enc)

    @staticmethod
    def _python(data):
        c = lzma.LZMACompressor(format=lzma.FORMAT_XZ, check=lzma.CHECK_CRC64,
                                filters=[{"id": lzma.FILTER_LZMA2, "dict_size": 1 << 24}])
        return c.compress(data) + c.flush()

    @classmethod
    def compress(cls, data):
        free = cls.pool()
        data = bytes(data)
        if free is not None:
            return cls._encode(free, data)
        with cls._sem:
            return cls._python(data)

    @classmethod
    def release(cls):
        """lzma_end on every idle pooled encoder (their memory goes back now)"""
        free = cls._pool
        if not free:
            return
        held = []
        while True:
            try:
                held.append(free.get_nowait())
            except queue.Empty:
                break
        for enc in held:
            enc.end()
            free.put(enc)


class LZMACompression(CompressionMethod):
    """advanced_compression.py:155-213"""
    type_id = 7

    def compress(self, data):
        if not data:
            return b""
        try:
            return _XZEncoders.compress(data)
        except Exception:  # noqa: BLE001 -- advanced_compression.py:183-185 returns the input
            return data

    def should_use(self, data, threshold=0.9):
        # advanced_compression.py:202-213
        return len(data) >= 8192 and calculate_entropy(data) < 8.0

    def decompress(self, data, original_length):
        if not data:
            return b""
        try:
            return _fit(lzma.decompress(data), original_length)
        except Exception:  # noqa: BLE001
            return bytes(original_length)


class _Zstd:
    """The system libzstd (ctypes) with python-zstandard's call semantics -- the
    reference's id 8 wraps ``zstandard`` (requirements.txt: >=0.15.0), which is
    not installed here.  Bytes are libzstd's own at level 19; parity unpinned (no
    reference fixture holds a zstd package)."""

    CONTENTSIZE_UNKNOWN = (1 << 64) - 1
    CONTENTSIZE_ERROR = (1 << 64) - 2

    class _Buf(C.Structure):               # ZSTD_inBuffer / ZSTD_outBuffer
        _fields_ = [("ptr", C.c_void_p), ("size", C.c_size_t), ("pos", C.c_size_t)]

    _lib = None

    @classmethod
    def lib(cls):
        if cls._lib is None:
            lib = C.CDLL("libzstd.so.1")
            lib.ZSTD_compressBound.restype = C.c_size_t
            lib.ZSTD_compressBound.argtypes = [C.c_size_t]
            lib.ZSTD_compress.restype = C.c_size_t
            lib.ZSTD_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
            lib.ZSTD_isError.restype = C.c_uint
            lib.ZSTD_isError.argtypes = [C.c_size_t]
            lib.ZSTD_getFrameContentSize.restype = C.c_ulonglong
            lib.ZSTD_getFrameContentSize.argtypes = [C.c_void_p, C.c_size_t]
            lib.ZSTD_createDCtx.restype = C.c_void_p
            lib.ZSTD_freeDCtx.argtypes = [C.c_void_p]
            lib.ZSTD_decompressStream.restype = C.c_size_t
            lib.ZSTD_decompressStream.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
            cls._lib = lib
        return cls._lib

    @classmethod
    def available(cls):
        try:
            cls.lib()
            return True
        except OSError:
            return False

    @classmethod
    def compress(cls, data, level):
        """ZstdCompressor(level=level).compress(data): one frame with its content size."""
        lib = cls.lib()
        src = bytes(data)
        cap = lib.ZSTD_compressBound(len(src))
        dst = C.create_string_buffer(cap)
        r = lib.ZSTD_compress(dst, cap, src, len(src), level)
        if lib.ZSTD_isError(r):
            raise RuntimeError("zstd compress error")
        return dst.raw[:r]

    @classmethod
    def decompress(cls, data, max_output_size):
        """ZstdDecompressor().decompress(data, max_output_size=...): the first frame;
        its header's content size when present, else at most max_output_size
        bytes; raises where python-zstandard raises ZstdError."""
        lib = cls.lib()
        src = bytes(data)
        size = lib.ZSTD_getFrameContentSize(src, len(src))
        if size == cls.CONTENTSIZE_ERROR:
            raise ValueError("error determining content size from frame header")
        if size == 0:
            return b""
        if size == cls.CONTENTSIZE_UNKNOWN:
            if max_output_size == 0:
                raise ValueError("could not determine content size in frame header")
            cap, expect = max_output_size, 0
        else:
            cap, expect = size, size
        dst = C.create_string_buffer(max(cap, 1))
        inb = cls._Buf(C.cast(C.c_char_p(src), C.c_void_p), len(src), 0)
        outb = cls._Buf(C.cast(dst, C.c_void_p), cap, 0)
        dctx = lib.ZSTD_createDCtx()
        if not dctx:
            raise MemoryError("ZSTD_createDCtx")
        try:
            r = lib.ZSTD_decompressStream(dctx, C.byref(outb), C.byref(inb))
        finally:
            lib.ZSTD_freeDCtx(dctx)
        if lib.ZSTD_isError(r):
            raise ValueError("zstd decompression error")
        if r:
            raise ValueError("decompression error: did not decompress full frame")
        if expect and outb.pos != expect:
            raise ValueError("decompression error: decompressed size mismatch")
        return dst.raw[:outb.pos]


class ZstdCompression(CompressionMethod):
    """advanced_compression.py:219-261 (registered when the reference's
    ``zstandard`` would be: here, when the system libzstd loads)."""
    type_id = 8

    def compress(self, data):
        if not data:
            return b""
        try:
            return _Zstd.compress(data, 19)
        except Exception:  # noqa: BLE001 -- advanced_compression.py:232-234 returns the input
            return bytes(data)

    def decompress(self, data, original_length):
        if not data:
            return b""
        try:
            return _fit(_Zstd.decompress(data, original_length), original_length)
        except Exception:  # noqa: BLE001 -- reference returns zeros on error
            return bytes(original_length)

    def should_use(self, data, threshold=0.9):
        # advanced_compression.py:252-261 (entropy > 8.2 is impossible for bytes)
        return len(data) >= 512 and calculate_entropy(data) <= 8.2


GPU_METHODS = {1: RLECompression, 2: DictionaryCompression, 3: HuffmanCompression,
               4: DeltaCompression, 5: DeflateCompression, 9: LZ4Compression}
DECODE_METHODS = {1: RLECompression, 2: DictionaryCompression, 3: HuffmanCompression,
                  4: DeltaCompression, 5: DeflateCompression, 6: Bzip2Compression,
                  7: LZMACompression, 9: LZ4Compression, 255: NoCompression}
HAS_ZSTD = _Zstd.available()
if HAS_ZSTD:
    DECODE_METHODS[8] = ZstdCompression
