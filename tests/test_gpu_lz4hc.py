"""id 9 as "ambc-lz4 hc v1" on the GPU (AMBC_FLAG_LZ4HC, AdaptiveCompressor(lz4="hc"),
LZ4Compression(level="hc"), main.py compress --lz4 hc): k_lz4hc's frames are
ambc_lz4hc_model's byte for byte, id 9 takes a chunk iff its frame + 18 is strictly
below the best of the lower ids, the pipelined-segment path gives the one-range
body, and the default encoder is untouched.  Integer / byte work: no tolerance."""
import ctypes as C
import os
import struct
import subprocess
import sys

import pytest

from conftest import PKG_DIR, REPO
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

MARKER = b"\xff\xff\x00\x00"
END = MARKER + bytes(12)
WIDE = (1, 999999999)


@pytest.fixture(scope="module")
def ctx(hip_lib):
    from ambc import _lib
    return _lib.default_context()


def _compressor(**kw):
    from ambc import AdaptiveCompressor
    return AdaptiveCompressor(**kw)


_MODEL = {}


def model(d):
    d = bytes(d)
    fr = _MODEL.get(d)
    if fr is None:
        from ambc import _lib
        lib = _lib.load()
        out = (C.c_uint8 * (len(d) + 64))()
        ln = C.c_uint32()
        assert lib.ambc_lz4hc_model(_lib.addr(d), len(d), C.addressof(out), len(d) + 64, C.byref(ln)) == 0
        fr = _MODEL[d] = bytes(out[:ln.value])
    return fr


def packages(body):
    """body -> [(id, orig, payload)], the end chunk checked"""
    out, p = [], 0
    while True:
        assert body[p:p + 4] == MARKER
        mid, kv = body[p + 4], body[p + 5]
        if mid == 0 and kv == 0 and body[p:p + 16] == END and p + 16 == len(body):
            return out
        used, orig, clen = struct.unpack_from("<III", body, p + 6)
        assert used == orig
        out.append((mid, orig, body[p + 18:p + 18 + clen]))
        p += 18 + clen


def pkg(mid, n, payload):
    return MARKER + struct.pack("<BBIII", mid, 0, n, n, len(payload)) + payload


def mixed(n):
    return orc.synth(n, 20250418)


def content(kind, n):
    if kind == "mixed":
        # (a stretch of the stream that holds text, random and zero chunks at these sizes)
        return mixed(n + (1 << 20))[(1 << 20) - n // 2:][:n]
    if kind == "zero":
        return bytes(n)
    if kind == "period7":
        return (b"abcdefg" * (n // 7 + 1))[:n]
    return orc.random_bytes(n, 11)


# ---------------------------------------------------------------------------
# kernel == model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("csize", [16, 64, 1024, 4096, 16384])
def test_kernel_frames_equal_the_model(ctx, csize):
    """{9} alone, prefs wide open: every id-9 payload is the model's frame of its
    chunk, and a chunk stays raw only where the model's frame + 18 is not below n"""
    comp = _compressor(chunk_size=csize, methods=(9,), lz4="hc")
    comp.method_chunk_prefs[9] = WIDE
    n9 = 0
    for kind in ("mixed", "zero", "period7", "random"):
        for n in (csize, 3 * csize + 5, 4 * csize - 1):
            data = content(kind, n)
            pk = packages(comp._adaptive_compress(data))
            assert len(pk) == (n + csize - 1) // csize
            pos = 0
            for mid, orig, payload in pk:
                chunk = data[pos:pos + orig]
                pos += orig
                fr = model(chunk)
                if mid == 9:
                    assert payload == fr, (kind, n, pos)
                    assert len(fr) + 18 < orig
                    n9 += 1
                else:
                    assert mid == 255 and payload == chunk
                    assert len(fr) + 18 >= orig, (kind, n, pos)
            assert pos == n
    assert n9 >= (3 if csize >= 64 else 0)


# ---------------------------------------------------------------------------
# selection order
# ---------------------------------------------------------------------------
def tie_chunk():
    """Huffman's payload and the hc frame are both 1062 bytes: id 3 keeps the chunk"""
    c = bytes(3076) + bytes(b & 15 for b in orc.random_bytes(4096, 1))[:1020]
    assert len(orc.huff_encode(c)) == len(model(c)) == 1062
    return c


def expected_body(data, csize, mode, methods):
    """the selection in Python: the oracle's verdict over the lower ids, then id 9
    (the model's frame) iff len + 18 is strictly below it and the prefs admit it"""
    n = len(data)
    low = tuple(m for m in methods if m != 9)
    p = orc.make_params(csize, "native", low, n_total=n, deflate="gd")
    ids, pls = orc.decide_all(data, p)
    lo9, hi9 = orc.PREFS[9]
    enc = {1: orc.rle_encode, 3: orc.huff_encode, 5: orc.gdeflate_encode}
    body, sel = b"", []
    for k, (mid, pl) in enumerate(zip(ids, pls)):
        chunk = data[k * csize:(k + 1) * csize]
        m = len(chunk)
        best = m if mid == 255 else pl + 18
        if lo9 <= m <= hi9 and len(model(chunk)) + 18 < best:
            mid = 9
        if mid == 255 and mode == "reference":      # the rest of the file as one raw chunk
            rest = data[k * csize:]
            sel.append(255)
            body += pkg(255, len(rest), rest)
            break
        payload = model(chunk) if mid == 9 else chunk if mid == 255 else enc[mid](chunk)
        assert mid in (9, 255) or len(payload) == pl
        sel.append(mid)
        body += pkg(mid, m, payload)
    return body + END, sel


def selection_input():
    d = bytearray(mixed(2 << 20)[(1 << 20) - 32 * 4096:][:64 * 4096])
    d[5 * 4096:6 * 4096] = tie_chunk()
    return bytes(d)


@pytest.mark.parametrize("mode", ["native", "reference"])
def test_selection_order(ctx, mode):
    data = selection_input()
    comp = _compressor(chunk_size=4096, mode=mode, methods=(1, 3, 4, 9), lz4="hc")
    body = comp._adaptive_compress(data)
    want, sel = expected_body(data, 4096, mode, (1, 3, 4, 9))
    assert [p[0] for p in packages(body)] == sel
    assert body == want
    assert sel[5] == 3                              # the tie: Huffman, the lower id
    if mode == "native":
        assert {1, 3, 9, 255} <= set(sel)
    out = (C.c_uint8 * len(data))()
    from ambc import _lib
    st = _lib.Stats()
    _lib.check(ctx.lib.ambc_decompress_batch(ctx.h, _lib.addr(body), len(body), len(data), C.addressof(out),
                                             C.byref(st)), ctx.lib)
    assert bytes(out) == data


def test_selection_order_with_deflate(ctx):
    """{1, 3, 4, 5, 9}: k_deflate, then k_lz4hc, then the pending RLE / Huffman payloads"""
    data = selection_input()
    comp = _compressor(chunk_size=4096, methods=(1, 3, 4, 5, 9), lz4="hc")
    body = comp._adaptive_compress(data)
    want, sel = expected_body(data, 4096, "native", (1, 3, 4, 5, 9))
    assert [p[0] for p in packages(body)] == sel
    assert body == want
    assert 5 in sel
    assert comp._adaptive_decompress(body, len(data)) == data


def test_hc_takes_over_a_dictionary_payload(ctx):
    """{2, 9}: id 2's payload lies in the slot when k_lz4hc runs; where id 9 wins
    its frame replaces it, where it loses the Dictionary payload stays whole"""
    data = selection_input()[:16 * 4096]
    comp = _compressor(chunk_size=4096, methods=(2, 9), lz4="hc")
    pk = packages(comp._adaptive_compress(data))
    only2 = packages(_compressor(chunk_size=4096, methods=(2,))._adaptive_compress(data))
    for k, ((mid, orig, payload), (m2, _, p2)) in enumerate(zip(pk, only2)):
        chunk = data[k * 4096:(k + 1) * 4096]
        best = orig if m2 == 255 else len(p2) + 18
        if len(model(chunk)) + 18 < best:
            assert (mid, payload) == (9, model(chunk)), k
        else:
            assert (mid, payload) == (m2, p2), k
    assert comp._adaptive_decompress(comp._adaptive_compress(data), len(data)) == data


# ---------------------------------------------------------------------------
# pipelined segments
# ---------------------------------------------------------------------------
_ONE_RANGE = """
import hashlib, sys
sys.path[:0] = [%r, %r]
from ambc import AdaptiveCompressor
from oracle import oracle as orc
data = orc.synth(16 << 20, 20250418)
body = AdaptiveCompressor(chunk_size=1024, methods=(1, 3, 4, 9), lz4="hc")._adaptive_compress(data)
print("BODY", len(body), hashlib.sha256(body).hexdigest())
"""


def test_segmented_path_equals_one_range(ctx):
    import hashlib
    data = mixed(16 << 20)                          # 16384 chunks of 1024: pipelined segments
    comp = _compressor(chunk_size=1024, methods=(1, 3, 4, 9), lz4="hc")
    body = comp._adaptive_compress(data)
    nl = C.c_uint32()
    assert ctx.lib.ambc_last_encode_launches(ctx.h, 0, C.byref(nl)) == 0 and nl.value > 1
    env = dict(os.environ, AMBC_NSEG="1")
    r = subprocess.run([sys.executable, "-c", _ONE_RANGE % (REPO, PKG_DIR)], env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("BODY")][0].split()
    assert (int(line[1]), line[2]) == (len(body), hashlib.sha256(body).hexdigest())
    assert comp._adaptive_decompress(body, len(data)) == data


# ---------------------------------------------------------------------------
# the default encoder, errors, plugin, CLI, an external decoder
# ---------------------------------------------------------------------------
def test_default_is_untouched(ctx):
    data = selection_input()
    base = _compressor(chunk_size=4096, methods=(1, 3, 4, 9))._adaptive_compress(data)
    for v in (None, "greedy"):
        assert _compressor(chunk_size=4096, methods=(1, 3, 4, 9), lz4=v)._adaptive_compress(data) == base
    ref, _ = orc.compress_body(data, orc.make_params(4096, "native", (1, 3, 4, 9), n_total=len(data)))
    assert base == ref
    assert _compressor(chunk_size=4096, methods=(1, 3, 4, 9), lz4="hc")._adaptive_compress(data) != base


def test_error_paths(ctx):
    from ambc import _lib
    data = mixed(1 << 16)
    with pytest.raises(ValueError):
        _compressor(lz4="fast")
    with pytest.raises(ValueError, match="16384"):
        _compressor(chunk_size=32768, methods=(1, 3, 4, 9), lz4="hc")._adaptive_compress(data)
    comp = _compressor(methods=(1, 3, 4, 9), lz4="hc")
    comp.CHUNK_SIZE_CANDIDATES = [1024, 4096]
    with pytest.raises(ValueError, match="walk"):
        comp._adaptive_compress(data)
    # the C ABI itself
    p = _lib.Params()
    p.chunk_size = 32768
    p.method_mask = 1 << 9
    p.flags = _lib.FLAG_LZ4HC
    for i in range(16):
        p.pref_min[i], p.pref_max[i] = 1, 0xFFFFFFFF
    cap = ctx.lib.ambc_compress_bound(len(data), 32768)
    out = bytearray(cap)
    olen = C.c_uint64()
    st = _lib.Stats()
    rc = ctx.lib.ambc_compress_batch(ctx.h, _lib.addr(data), len(data), C.byref(p), _lib.addr(out), cap,
                                     C.byref(olen), C.byref(st))
    assert rc == _lib.AMBC_E_INVAL and "16384" in _lib.last_error(ctx.lib)
    p.chunk_size = 4096
    cands = (C.c_uint32 * 2)(1024, 4096)
    rc = ctx.lib.ambc_compress_multisize(ctx.h, _lib.addr(data), len(data), C.byref(p), cands, 2, None, None, 0,
                                         _lib.addr(out), cap, C.byref(olen), C.byref(st))
    assert rc == _lib.AMBC_E_INVAL and "multi-size walk" in _lib.last_error(ctx.lib)
    ln = C.c_uint32()
    big = bytes(16400)
    rc = ctx.lib.ambc_encode_method_ex(ctx.h, 9, _lib.FLAG_LZ4HC, _lib.addr(big), len(big), _lib.addr(out), cap,
                                       C.byref(ln))
    assert rc == _lib.AMBC_E_INVAL


def test_plugin(ctx):
    from ambc import LZ4Compression
    from ambc import _lib
    with pytest.raises(ValueError):
        LZ4Compression(level="fast")
    hc = LZ4Compression(level="hc")
    tail = mixed(2 << 20)[(1 << 20) - 2048:]
    for x in (tail[:4096], tail[:100], bytes(16384), orc.random_bytes(1000, 3), b"abc", tie_chunk()):
        fr = hc.compress(x)
        assert fr == model(x)
        assert hc.decompress(fr, len(x)) == x
    assert hc.compress(b"") == b""
    with pytest.raises(ValueError):
        hc.compress(bytes(16385))
    # flags = 0 is ambc_encode_method
    x = tail[:4096]
    out = (C.c_uint8 * 8192)()
    ln = C.c_uint32()
    pc = _lib.plugin_context()
    _lib.check(pc.lib.ambc_encode_method_ex(pc.h, 9, 0, _lib.addr(x), len(x), C.addressof(out), 8192, C.byref(ln)))
    assert bytes(out[:ln.value]) == LZ4Compression().compress(x) == orc.lz4_frame_encode(x)


def test_cli_round_trip(ctx, tmp_path):
    data = mixed(2 << 20)[(1 << 20) - 32768:][:65536]
    src, amb, back = tmp_path / "in.bin", tmp_path / "out.ambc", tmp_path / "back.bin"
    src.write_bytes(data)
    main = os.path.join(PKG_DIR, "main.py")
    for argv in (["compress", str(src), str(amb), "--lz4", "hc", "--history", ""],
                 ["decompress", str(amb), str(back)]):
        r = subprocess.run([sys.executable, main] + argv, capture_output=True, text=True, timeout=300, cwd=tmp_path)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert back.read_bytes() == data
    blob, _ = _compressor(chunk_size=4096, methods=(1, 3, 4, 9), lz4="hc").compress_bytes(data)
    assert amb.read_bytes() == blob


def test_id9_payloads_decode_with_system_liblz4(ctx):
    try:
        lz = C.CDLL("liblz4.so.1")
    except OSError:
        pytest.skip("system liblz4 not present")
    lz.LZ4_decompress_safe.argtypes = [C.c_char_p, C.c_void_p, C.c_int, C.c_int]
    lz.LZ4_decompress_safe.restype = C.c_int
    data = selection_input()
    body = _compressor(chunk_size=4096, methods=(1, 3, 4, 9), lz4="hc")._adaptive_compress(data)
    pos = n9 = 0
    for mid, orig, fr in packages(body):
        if mid == 9:
            assert fr[:6] == b"\x04\x22\x4d\x18\x68\x40" and fr[-4:] == bytes(4)
            bs = int.from_bytes(fr[15:19], "little")
            assert bs == len(fr) - 23
            out = C.create_string_buffer(orig + 16)
            r = lz.LZ4_decompress_safe(fr[19:19 + bs], out, bs, orig + 16)
            assert r == orig and out.raw[:r] == data[pos:pos + orig]
            n9 += 1
        pos += orig
    assert n9 >= 10
