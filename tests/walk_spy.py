"""A spy on api._iter_windows' walk, shared by the tests of the windowed entries (flagstat, idxstats,
stats, fastq, depth, pileup): which windows an entry loaded, and which of them it loaded twice."""
from pkg import sb
from test_record_conformance_gpu import call


def walked(fn, path, ctx, halo=None, header_shards=2, **kw):
    """fn(path, ctx=ctx, **kw), and the walk it made: (file offset, resident bytes) of every window
    attempt -- a window that ran again with a larger halo shows as its offset twice.  halo: the walk's
    first halo (the entries take none of their own; default 4 MiB, more than these files hold).
    header_shards: the shards that read the header before the first window -- the entry's own and the
    walk's; 1 for an entry that reads none itself (fastq)."""
    attempts = []
    index, walk = sb.device.Shard.index, sb.api._iter_windows

    def spy(self, *a, **k):
        attempts.append((self.file_offset, self.n))
        return index(self, *a, **k)

    sb.device.Shard.index = spy
    if halo is not None:
        sb.api._iter_windows = lambda data, deliver, window=None, **k: walk(data, deliver, window, halo=halo, **k)
    try:
        r = call(fn, path, ctx=ctx, **kw)
    finally:
        sb.device.Shard.index, sb.api._iter_windows = index, walk
    return r, attempts[header_shards:]
