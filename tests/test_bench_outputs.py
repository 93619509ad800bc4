"""bench.py --dump-outputs / --full.

* dump_outputs on the CPU over a stand-in device buffer: every file float32 /
  float64, the CRC-32 of every MiB, the sampled blocks equal to the body at their
  offsets, whole small bodies, the seeded sample of a large one (more than 2048
  blocks, more than one 64 MiB copy), under 64 MB in all.
* on the GPU: a plain run times exactly --steps steps, runs no other leg, and its
  dump is the oracle's body of the same stream (length, every CRC, the sample,
  method usage, statistics)."""
import json
import os
import random
import subprocess
import sys
import zlib

import numpy as np
import pytest

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402

NAMES = ["body_crc32", "body_len", "body_sample", "body_sample_offsets", "method_usage", "stats"]


class _HostBuffer:
    """DeviceBuffer.download's signature over host bytes"""

    def __init__(self, data):
        self.data = data

    def download(self, n, offset, out):
        out[:n] = self.data[offset:offset + n]


def _load(d):
    assert sorted(os.listdir(d)) == [n + ".npy" for n in NAMES]
    a = {n: np.load(os.path.join(d, n + ".npy")) for n in NAMES}
    assert a["body_sample"].dtype == np.float32
    assert all(a[n].dtype == np.float64 for n in NAMES if n != "body_sample")
    assert sum(v.nbytes for v in a.values()) <= 64 * 1000 * 1000
    return a


def _check_body(a, body):
    assert a["body_len"].tolist() == [len(body)]
    assert a["body_crc32"].tolist() == [zlib.crc32(body[o:o + (1 << 20)]) for o in range(0, len(body), 1 << 20)]
    nblk = -(-len(body) // 4096)
    offs = a["body_sample_offsets"].astype(np.int64).tolist()
    assert len(offs) == min(nblk, 2048) and offs == sorted(set(offs)) and all(o % 4096 == 0 for o in offs)
    assert a["body_sample"].shape == (len(offs), 4096)
    for o, blk in zip(offs, a["body_sample"]):
        assert o < len(body)
        assert bytes(blk.astype(np.uint8)) == bytes(body[o:o + 4096]).ljust(4096, b"\0")
    return offs


@pytest.mark.parametrize("n", [0, 5, 4096, 100000, (64 << 20) + 4096 + 5])
def test_dump_outputs_host(tmp_path, n):
    from ambc import _lib
    body = random.Random(n).randbytes(n)
    st = _lib.Stats()
    st.method_usage[3], st.method_usage[255] = 7, 2
    st.total_chunks, st.overhead_bytes, st.kernel_ns = 9, 162, 12345
    picks = []
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), "", _HostBuffer(body), n, st, 11)
        a = _load(str(tmp_path / d))
        picks.append(_check_body(a, body))
        assert a["method_usage"][3] == 7 and a["method_usage"][255] == 2 and a["method_usage"].sum() == 9
        assert a["stats"].tolist() == [9, 0, 0, 0, 0, 162]
    assert picks[0] == picks[1]                       # the sample is a function of (length, seed)
    if n > 2048 * 4096:
        bench.dump_outputs(str(tmp_path / "c"), "", _HostBuffer(body), n, st, 12)
        assert _check_body(_load(str(tmp_path / "c")), body) != picks[0]


@pytest.mark.gpu
def test_plain_bench_dump_is_the_oracle_body(hip_lib, tmp_path):
    from oracle import oracle as orc
    n, chunk, seed, steps = 24 << 20, 4096, 20250418, 3
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps),
                        "--warmup", "1", "--size", str(n), "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    # "steps" is the number of step times the timed loop collected, not the argument echoed
    assert line["steps"] == steps and line["full"] is False and line["ms_per_step"] > 0
    assert line["unit"] == "GB/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    cfg = line["config"]
    assert line["cpu_baseline"] is None and cfg["round_trip_bit_exact"] is None and cfg["decode"] is None
    assert cfg["e2e_pinned_host"] is None and cfg["api_file"] is None and cfg["alt_method_sets"] == []
    assert cfg["multisize_walk"] == [] and cfg["like_reference_walk"] is None
    assert cfg["like_reference_full_walk"] is None
    ref, st = orc.compress_body(orc.synth(n, seed), orc.make_params(chunk, "native", (1, 3, 4, 9), n_total=n))
    a = _load(str(tmp_path / "d"))
    assert len(_check_body(a, ref)) == 2048
    assert cfg["ratio"] == round(len(ref) / n, 5)
    assert a["method_usage"].tolist() == [st.method_usage[i] for i in range(256)]
    assert [a["stats"][i] for i in (1, 3, 4)] == [st.compressed_chunks, st.bytes_saved, st.payload_bytes]
