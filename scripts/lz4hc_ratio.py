#!/usr/bin/env python3
"""What a better id-9 parse is worth on the headline stream, measured on the CPU.

The first 16 MiB of the headline stream (ambc-mixed, seed 20250418) go through
the oracle's per-chunk selection over {1, 3, 4, 9} (native mode, the reference's
prefs) at C = 1024, 4096 and 16384, with id 9 sized three ways:

* greedy   "ambc-lz4 greedy v2" (oracle.lz4_frame_encode), the default encoder;
* hc       "ambc-lz4 hc v1" (ambc_lz4hc_model), the AMBC_FLAG_LZ4HC encoder;
* liblz4   the system liblz4's LZ4F_compressFrame at level 9 (the reference's
           lz4.frame.compress(data, compression_level=9)); left out when the
           library is absent.

ratio = body bytes / input bytes (18-byte chunk headers and the end chunk
included).  Chunks are also split by class (zero: one byte value; random: byte
entropy >= 7.5 bits; text: the rest).  --sweep adds the hc ratio at C = 4096 for
other hash widths and chain depths (ambc_lz4hc_model_ex): the measurement the
constants in csrc/ambc_consts.h were chosen by.

Needs no GPU.  One JSON document on stdout (profiles/r7_lz4hc_ratio.json).
"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "adaptive-compression_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

from ambc import _lib                 # noqa: E402
from oracle import oracle as orc      # noqa: E402

SEED = 20250418
TARGET_4096 = 0.48                    # the hc selection ratio to reach at C = 4096


def liblz4():
    try:
        lz = C.CDLL("liblz4.so.1")
    except OSError:
        return None
    lz.LZ4F_compressFrameBound.restype = C.c_size_t
    lz.LZ4F_compressFrameBound.argtypes = [C.c_size_t, C.c_void_p]
    lz.LZ4F_compressFrame.restype = C.c_size_t
    lz.LZ4F_compressFrame.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]
    lz.LZ4_versionString.restype = C.c_char_p
    return lz


class _FrameInfo(C.Structure):
    _fields_ = [("blockSizeID", C.c_int), ("blockMode", C.c_int), ("contentChecksumFlag", C.c_int),
                ("frameType", C.c_int), ("contentSize", C.c_ulonglong), ("dictID", C.c_uint),
                ("blockChecksumFlag", C.c_int)]


class _Prefs(C.Structure):
    _fields_ = [("frameInfo", _FrameInfo), ("compressionLevel", C.c_int), ("autoFlush", C.c_uint),
                ("favorDecSpeed", C.c_uint), ("reserved", C.c_uint * 3)]


def liblz4_frame_len(lz, chunk):
    """len(lz4.frame.compress(chunk, compression_level=9)): python-lz4's defaults
    (64 KiB blocks, linked, content size stored, no checksums)."""
    pr = _Prefs()
    pr.frameInfo.contentSize = len(chunk)
    pr.compressionLevel = 9
    cap = lz.LZ4F_compressFrameBound(len(chunk), C.byref(pr))
    out = C.create_string_buffer(cap)
    r = lz.LZ4F_compressFrame(out, cap, chunk, len(chunk), C.byref(pr))
    if r > cap:
        raise RuntimeError("LZ4F_compressFrame failed")
    return r


def hc_frame_len(lib, chunk, hb=None, depth=None):
    ln = C.c_uint32()
    src = _lib.addr(chunk)
    if hb is None:
        rc = lib.ambc_lz4hc_model(src, len(chunk), None, 0, C.byref(ln))
    else:
        rc = lib.ambc_lz4hc_model_ex(src, len(chunk), hb, depth, None, 0, C.byref(ln))
    if rc not in (_lib.AMBC_OK, _lib.AMBC_E_CAPACITY):
        raise RuntimeError(_lib.last_error(lib))
    return ln.value


def chunk_class(chunk):
    if len(set(chunk)) == 1:
        return "zero"
    return "random" if orc.np_entropy(chunk) >= 7.5 else "text"


def measure(data, csize, sizers):
    """sizers: {name: chunk -> id-9 frame length}.  Returns per name the body
    bytes, the ratio, the id-9 wins and the per-class (input, body) bytes."""
    n = len(data)
    params = orc.make_params(csize, "native", (1, 3, 4), n_total=n)
    ids, plens = orc.decide_all(data, params)
    lo9, hi9 = orc.PREFS[9]
    res = {k: {"body": 16, "id9": 0, "classes": {}} for k in sizers}
    for k, (mid, pl) in enumerate(zip(ids, plens)):
        chunk = data[k * csize:(k + 1) * csize]
        m = len(chunk)
        best = m if mid == 255 else pl + 18
        cls = chunk_class(chunk)
        ok9 = lo9 <= m <= hi9 and m >= 1024          # prefs and LZ4Compression.should_use
        for name, fn in sizers.items():
            size = m + 18 if mid == 255 else pl + 18  # the package without id 9
            if ok9:
                l9 = fn(chunk)
                if l9 + 18 < best:                    # ascending ids, strict "<": id 9 is last
                    size = l9 + 18
                    res[name]["id9"] += 1
            r = res[name]
            r["body"] += size
            c = r["classes"].setdefault(cls, {"chunks": 0, "input": 0, "body": 0})
            c["chunks"] += 1
            c["input"] += m
            c["body"] += size
    for r in res.values():
        r["ratio"] = round(r["body"] / n, 4)
        for c in r["classes"].values():
            c["ratio"] = round(c["body"] / c["input"], 4)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--mib", type=int, default=16, help="MiB of the headline stream (default 16)")
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 4096, 16384])
    ap.add_argument("--sweep", action="store_true", help="hc at C = 4096 over hash bits x chain depths")
    a = ap.parse_args()
    lib = _lib.load()
    lz = liblz4()
    data = orc.synth(a.mib << 20, SEED)
    sizers = {"greedy": lambda c: len(orc.lz4_frame_encode(c)), "hc": lambda c: hc_frame_len(lib, c)}
    if lz is not None:
        sizers["liblz4_hc9"] = lambda c: liblz4_frame_len(lz, c)
    out = {"stream": "ambc-mixed", "seed": SEED, "bytes": len(data), "methods": [1, 3, 4, 9],
           "liblz4": lz.LZ4_versionString().decode() if lz is not None else None, "sizes": {}}
    for cs in a.sizes:
        out["sizes"][str(cs)] = measure(data, cs, sizers)
    if "4096" in out["sizes"]:
        r = out["sizes"]["4096"]["hc"]["ratio"]
        out["target_4096"] = {"bound": TARGET_4096, "hc_ratio": r, "met": r <= TARGET_4096}
    if a.sweep:
        grid = {}
        for hb in (10, 11, 12, 13):
            sw = {f"hb{hb}_k{k}": (lambda c, hb=hb, k=k: hc_frame_len(lib, c, hb, k)) for k in (4, 8, 16, 32, 64)}
            for name, r in measure(data, 4096, sw).items():
                grid[name] = r["ratio"]
        out["sweep_4096"] = grid
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
