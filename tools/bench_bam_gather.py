#!/usr/bin/env python3
"""The BAM gather against the full record decode over the same records, one run.

Input: the benchmark's config-B corpus (tools/synth, seed 0x5B4D0001: 100 bp short reads,
coordinate-sorted, BGZF level 6, 12.4 M records ~ 1 GiB compressed), resident in HBM, after the
hot path (sbh_run_shard) has left the flat bytes, the block table and the eager bitmap on the
device.  Calls over the whole record range [first record, stream end), alternating:

  records_scan  sbh_records_scan: record starts from the bitmap, then every column of every record
                (records.hip) -- the yardstick: it reads the flat bytes once and writes more than it
                read (bases expand from 4 bits to a byte)
  bam_scan      sbh_records_bam_scan over the rows that scan left, no filter, the BAM header as head,
                the stream left on the device: it reads the flat bytes once and writes them once,
                plus 24 bytes of offsets per record, so the bar has no margin:
                bam_scan <= records_scan
  bam_dup       the same with -F 0x400 (runs of some tens of records)      } no bar
  bam_alt       the same with every other row kept (runs of one record)    }

Each library call runs on the shard's own stream and synchronises it before returning, so a call's
time is the time between its entry and its return, host round trips included.  It is taken twice:
by a pair of events recorded on torch's (idle) current stream just before and after the call, and
by the host clock.  After warm-up the medians are reported.

With --e2e-records N (default 400 000) the whole api.view_bam call is timed once per level (5 and
the fast coder) against api.htsjdk_rewrite(read_ranges = all rows) -- the host gather -- on a
smaller corpus of the same shape, and the outputs compared.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

SEED = 0x5B4D0001


def corpus(synth, records):
    p = synth.params(SEED, shape=0, level=6, threads=min(16, os.cpu_count() or 1))
    seg = synth.Segment(p, records, 1, 0, halo_blocks=16, log=lambda *a: print(*a, file=sys.stderr, flush=True))
    seg.set_offsets([seg.own_csize])
    return seg.comp, int(seg.file_size)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-records", type=int, default=400_000, help="records of the view_bam / htsjdk_rewrite corpus (0: skip)")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_bam_gather: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_bam_gather: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    header = np.frombuffer(synth.header_bytes(), dtype=np.uint8)
    _, contig_len, header_end = sb.parse_bam_header(synth.header_bytes())
    header = np.ascontiguousarray(header[:header_end])

    ctx = sb.Context(0)
    sh = ctx.shard(comp, file_offset=0, file_size=size)
    sh.set_contigs(contig_len)
    r = sh.run(0, size)
    if r["status"] or r["count"] != args.records:
        raise SystemExit(f"bench_bam_gather: the hot path found {r['count']} records (status {r['status']})")
    first = sh.flat_of(r["first_vpos"] >> 16, r["first_vpos"] & 0xFFFF)
    end = sh.flat_bound(size)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t = time.perf_counter()
        out = fn()
        wall = time.perf_counter() - t
        b.record()
        b.synchronize()
        return a.elapsed_time(b), wall * 1e3, out

    rsz = sb._lib.SbhRecordsSizes()
    bsz = sb._lib.SbhBamSizes()
    hp = header.ctypes.data_as(C.c_void_p)

    def decode():
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        return rsz.n

    def gather(filt, rows=None):
        f, keep = sb.records.record_filter(filt)
        if rows is not None:  # (row ranges as arrays: begins, ends)
            f, keep = sb._lib.SbhRecordFilter(0, 0, 0, 0, rows[0].ctypes.data, rows[1].ctypes.data, int(rows[0].size)), rows

        def call():
            sh._c(sb.lib().sbh_records_bam_scan(sh.h, hp, int(header.size), C.byref(f) if f is not None else None,
                                                C.byref(bsz)))
            return bsz.n_kept, bsz.bytes, keep
        return call

    even = np.arange(0, args.records, 2, dtype=np.uint64)
    calls = (("records_scan", decode), ("bam_scan", gather(None)), ("bam_dup", gather({"flag_exclude": 0x400})),
             ("bam_alt", gather(None, (even, even + np.uint64(1)))))
    ev = {k: [] for k, _ in calls}
    wl = {k: [] for k, _ in calls}
    last = {}
    for s in range(args.warmup + args.runs):
        for name, fn in calls:  # alternating
            e, w, got = timed(fn)
            last[name] = got if name == "records_scan" else got[:2]
            if s >= args.warmup:
                ev[name].append(e)
                wl[name].append(w)
    if last["records_scan"] != args.records or last["bam_scan"][0] != args.records:
        raise SystemExit(f"bench_bam_gather: record counts differ: {last}")
    stream_bytes = int(last["bam_scan"][1])
    if stream_bytes != int(header.size) + int(end - first):
        raise SystemExit(f"bench_bam_gather: {stream_bytes} stream bytes for {end - first} record bytes")
    # the unfiltered stream is the flat stream from the first record on, behind the header
    gather(None)()
    k = min(1 << 20, int(end - first))
    same = bool(np.array_equal(sh.bam_read(stream_bytes - k, stream_bytes), sh.read_flat(end - k, k)))

    med = {k: statistics.median(v) for k, v in ev.items()}
    out = {"bench": "bam_gather", "data": f"synthetic config B (tools/synth_bam.c, seed {SEED:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": int(end), "stream_bytes": stream_bytes,
           "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median",
           "records_scan_ms": round(med["records_scan"], 3), "bam_scan_ms": round(med["bam_scan"], 3),
           "ratio_bam_over_decode": round(med["bam_scan"] / med["records_scan"], 4),
           "bar": "bam_scan <= records_scan", "bar_met": bool(med["bam_scan"] <= med["records_scan"]),
           "bam_stream_GB_per_s": round(stream_bytes / (med["bam_scan"] * 1e-3) / 1e9, 2),
           "bam_records_per_s": round(args.records / (med["bam_scan"] * 1e-3)),
           "bam_dup_ms": round(med["bam_dup"], 3), "bam_dup_kept": int(last["bam_dup"][0]),
           "bam_dup_GB_per_s": round(int(last["bam_dup"][1]) / (med["bam_dup"] * 1e-3) / 1e9, 2),
           "bam_alt_ms": round(med["bam_alt"], 3), "bam_alt_kept": int(last["bam_alt"][0]),
           "bam_alt_GB_per_s": round(int(last["bam_alt"][1]) / (med["bam_alt"] * 1e-3) / 1e9, 2),
           "bam_alt_note": "the call uploads one row range per kept row (16 bytes each)",
           "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
           "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()},
           "stream_tail_equals_flat": same}
    sh.close()

    if args.e2e_records:
        small, _ = corpus(synth, args.e2e_records)
        e2e = {"records": args.e2e_records, "comp_bytes": int(small.size), "runs": 1,
               "note": "whole api calls by the host clock, file load and inflate included"}
        for label, level in (("level5", 5), ("fast", sb._lib.LEVEL_FAST)):
            sb.view_bam(small, level=level, ctx=ctx)  # (warm: allocations, code objects)
            t = time.perf_counter()
            a = sb.view_bam(small, level=level, ctx=ctx)
            ta = time.perf_counter() - t
            t = time.perf_counter()
            b = sb.htsjdk_rewrite(small, read_ranges=range(args.e2e_records), ctx=ctx, level=level)
            tb = time.perf_counter() - t
            e2e[label] = {"view_bam_s": round(ta, 3), "htsjdk_rewrite_all_rows_s": round(tb, 3),
                          "same_bytes": bool(a == b.tobytes()), "out_bytes": len(a)}
        out["view_bam_vs_htsjdk_rewrite"] = e2e
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not same:
        raise SystemExit("bench_bam_gather: the stream's tail differs from the flat bytes")


if __name__ == "__main__":
    main()
