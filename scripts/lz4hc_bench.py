#!/usr/bin/env python3
"""The two id-9 encoders as (GB/s, ratio) points: a device-resident compress of
the ambc-mixed stream (chunk 4096, native mode, methods {1, 3, 4, 9}) with
"ambc-lz4 greedy v2" and then with "ambc-lz4 hc v1" (AMBC_FLAG_LZ4HC), same
process, same input buffer, the legs alternating step by step.

    python scripts/lz4hc_bench.py [--size BYTES] [--steps K] [--warmup W]

Times are the library's hipEvent times: kernel_ms spans the call's device work
(encode, scan, compaction, statistics), encode_ms the encoder launches
(ambc_last_kernel_times).  GB/s = input bytes / median kernel_ms.  The hc body
is decoded on the device and compared with the input.  One JSON line on stdout
(profiles/r7_lz4hc_bench.json)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "adaptive-compression_amd")]

from ambc import _lib  # noqa: E402
from ambc.compressor import entropy_terms  # noqa: E402
from ambc.registry import METHOD_CHUNK_PREFS, method_mask  # noqa: E402

SEED = 20250418
METHODS = (1, 3, 4, 9)


def params(chunk, flags, tab):
    p = _lib.Params()
    p.chunk_size = chunk
    p.flags = flags | _lib.FLAG_INPUT_PADDED
    p.method_mask = method_mask(METHODS)
    for i in range(16):
        lo, hi = METHOD_CHUNK_PREFS.get(i, (1, 0))
        p.pref_min[i], p.pref_max[i] = lo, min(hi, 0xFFFFFFFF)
    p.ent_full = tab.ctypes.data
    return p


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--size", type=int, default=1 << 30)
    ap.add_argument("--chunk", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    if a.size % a.chunk:
        ap.error("--size must be a multiple of --chunk")
    a.steps = max(a.steps, 10)
    ctx = _lib.Context()
    lib = ctx.lib
    n = a.size
    cap = lib.ambc_compress_bound(n, a.chunk)
    d_in = lib.ambc_device_alloc(ctx.h, 0, n + 64)
    d_out = lib.ambc_device_alloc(ctx.h, 0, cap)
    d_back = lib.ambc_device_alloc(ctx.h, 0, n + 64)
    if not d_in or not d_out or not d_back:
        raise SystemExit("device allocation failed")
    _lib.check(lib.ambc_synth_device(ctx.h, 0, d_in, n, SEED), lib)
    tab = entropy_terms(a.chunk)
    legs = {"greedy": params(a.chunk, 0, tab), "hc": params(a.chunk, _lib.FLAG_LZ4HC, tab)}
    times = {k: {"kernel": [], "encode": []} for k in legs}
    res = {}

    def step(name, record):
        olen, st, e = C.c_uint64(), _lib.Stats(), C.c_uint64()
        _lib.check(lib.ambc_compress_device(ctx.h, 0, d_in, n, C.byref(legs[name]), d_out, cap, C.byref(olen),
                                            C.byref(st), None), lib)
        lib.ambc_last_kernel_times(ctx.h, 0, C.byref(e), None, None)
        if record:
            times[name]["kernel"].append(st.kernel_ns / 1e6)
            times[name]["encode"].append(e.value / 1e6)
        res[name] = (olen.value, st)

    for i in range(a.warmup + a.steps):
        for name in legs:
            step(name, i >= a.warmup)
    # the hc body is the one in d_out now: back to the host, decoded into device
    # memory, compared with the input on the device
    blen = res["hc"][0]
    body = bytearray(blen)
    _lib.check(lib.ambc_memcpy_d2h(ctx.h, 0, _lib.addr(body), d_out, blen), lib)
    reg = (C.c_uint64 * 4)()
    for t in METHODS + (255,):
        reg[t >> 6] |= 1 << (t & 63)
    ds, eq = _lib.Stats(), C.c_int(0)
    _lib.check(lib.ambc_decompress_device(ctx.h, 0, _lib.addr(body), blen, n, reg, d_back, C.byref(ds)), lib)
    _lib.check(lib.ambc_device_equal(ctx.h, 0, d_back, d_in, n, C.byref(eq)), lib)
    out = {"bench": "lz4hc", "stream": "ambc-mixed", "seed": SEED, "bytes": n, "chunk": a.chunk,
           "mode": "native", "methods": list(METHODS), "steps": a.steps, "warmup": a.warmup,
           "timing": "hipEvent (ambc_stats.kernel_ns, ambc_last_kernel_times), median of steps, legs alternating"}
    for name in legs:
        blen_k, st = res[name]
        k = statistics.median(times[name]["kernel"])
        e = statistics.median(times[name]["encode"])
        out[name] = {"GBps": round(n / k / 1e6, 2), "ratio": round(blen_k / n, 4), "body_bytes": blen_k,
                     "kernel_ms": round(k, 3), "kernel_ms_min": round(min(times[name]["kernel"]), 3),
                     "kernel_ms_max": round(max(times[name]["kernel"]), 3), "encode_ms": round(e, 3),
                     "kernel_ms_per_GiB": round(k * (1 << 30) / n, 3),
                     "usage": {str(m): int(st.method_usage[m]) for m in METHODS if st.method_usage[m]}}
    out["hc"]["round_trip_bit_exact"] = bool(eq.value) and ds.payload_bytes == n
    for ptr in (d_in, d_out, d_back):
        lib.ambc_device_free(ctx.h, 0, ptr)
    print(json.dumps(out))
    return 0 if out["hc"]["round_trip_bit_exact"] else 1


if __name__ == "__main__":
    sys.exit(main())
