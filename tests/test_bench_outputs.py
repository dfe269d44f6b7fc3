"""bench.py --dump-outputs: the arrays of a step, the seeded resident sample and the files written
(host side only; the step itself is the GPU suite's subject)."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


class _Shard:
    """read_flat / eager_bits over host arrays, with the device calls' range rules."""

    def __init__(self, n):
        self.u = (np.arange(n) % 251).astype(np.uint8)
        self.bits = (np.arange((n + 7) // 8) % 13).astype(np.uint8)

    def read_flat(self, a, n):
        assert 0 <= a and a + n <= self.u.size
        return self.u[a:a + n]

    def eager_bits(self, a, b):
        assert a % 8 == 0 and a <= b <= self.u.size
        return self.bits[a // 8:(b + 7) // 8]


def test_step_arrays_split_virtual_offsets_exactly():
    v = np.array([(123456789012 << 16) | 65535, 0], dtype=np.uint64)
    a = bench.step_arrays(889, -1, dict(count=7, n_true=8, flat_bytes=3002924681), np.array([0, 2], np.int32), v,
                          np.array([7, 0], np.uint64))
    assert all(x.dtype == np.float64 for x in a.values())
    assert a["result"].tolist() == [0, 889, 7, 8, 3002924681, -1, -1]
    assert a["split_first_block_pos"].tolist() == [123456789012, 0]
    assert a["split_first_offset"].tolist() == [65535, 0]
    assert a["split_status"].tolist() == [0, 2] and a["split_count"].tolist() == [7, 0]


@pytest.mark.parametrize("n", [0, 5, 1000, bench.DUMP_CHUNKS * bench.DUMP_CHUNK + 11, 10_000_003])
def test_resident_sample_is_fixed_and_in_range(n):
    sh = _Shard(n)
    s, s2 = bench.resident_sample(sh, 3, n), bench.resident_sample(sh, 3, n)
    assert all(np.array_equal(s[k], s2[k]) for k in s)
    b, e = s["sample_flat_begin"].astype(np.int64), s["sample_flat_end"].astype(np.int64)
    assert np.all(b % 8 == 0) and np.all(b < e) and np.all(e <= n) and np.all(b[1:] >= e[:-1])
    assert len(b) <= bench.DUMP_CHUNKS + 1
    want = np.concatenate([sh.u[x:y] for x, y in zip(b, e)] or [np.zeros(0, np.uint8)])
    assert s["sample_inflated_bytes"].dtype == np.float32 and np.array_equal(s["sample_inflated_bytes"], want)
    assert s["sample_eager_bitmap_bytes"].size == sum((y - x + 7) // 8 for x, y in zip(b, e))
    assert sum(x.nbytes for x in s.values()) <= bench.DUMP_MAX_BYTES // 2


def test_dump_outputs_files_and_limit(tmp_path):
    arrays = {"result": np.arange(7, dtype=np.float64), "sample": np.ones(9, dtype=np.float32)}
    d = str(tmp_path / "out" / "dir")
    bench.dump_outputs(d, 0, arrays)
    bench.dump_outputs(d, 1, arrays)
    assert sorted(os.listdir(d)) == ["result.npy", "result_rank1.npy", "sample.npy", "sample_rank1.npy"]
    assert np.array_equal(np.load(os.path.join(d, "result.npy")), arrays["result"])
    with pytest.raises(RuntimeError):
        bench.dump_outputs(d, 0, {"big": np.zeros(bench.DUMP_MAX_BYTES // 8 + 1, dtype=np.float64)})
