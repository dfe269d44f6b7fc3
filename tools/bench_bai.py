#!/usr/bin/env python3
"""BAI scan against the full record decode over the same records, one run.

Input: the benchmark's config-B corpus (tools/synth, seed 0x5B4D0001: 100 bp short reads,
coordinate-sorted, BGZF level 6, 12.4 M records ~ 1 GiB compressed), resident in HBM, after the
hot path (sbh_run_shard) has left the flat bytes, the block table and the eager bitmap on the
device.  Two calls over the whole record range [first record, stream end):

  bai_scan      sbh_bai_scan: record starts from the bitmap, keys / windows / virtual offsets per
                record, one scan, the runs and the linear-index minima (bai.hip)
  records_scan  sbh_records_scan: the same record starts, then every column of every record
                (records.hip) -- the yardstick: the scan reads a subset of what the decode reads
                and writes far less, so it must not take longer (ratio <= 1.0)

Each library call runs on the shard's own stream and synchronises it before returning, so a call's
time is the time between its entry and its return, host round trips included.  It is taken twice:
by a pair of events recorded on torch's (idle) current stream just before and after the call,
and by the host clock; the two agree and neither isolates kernel time.  The calls alternate,
after warm-up, and the medians are reported.  bai_build_ms is the host
finisher (sbh_bai_build) on the scan's result.  Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_bai: at least 10 timed runs")

    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    bai_mod = __import__(sb.__name__ + ".bai", fromlist=["x"])
    if not torch.cuda.is_available():
        raise SystemExit("bench_bai: no GPU (a measurement needs one; there is no fallback)")

    seed = 0x5B4D0001
    t0 = time.time()
    p = synth.params(seed, shape=0, level=6, threads=min(16, os.cpu_count() or 1))
    seg = synth.Segment(p, args.records, 1, 0, halo_blocks=16, log=lambda *a: None)
    seg.set_offsets([seg.own_csize])
    comp, size = seg.comp, int(seg.file_size)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    _, contig_len, _ = sb.parse_bam_header(synth.header_bytes())

    ctx = sb.Context(0)
    sh = ctx.shard(comp, file_offset=0, file_size=size)
    sh.set_contigs(contig_len)
    r = sh.run(0, size)
    if r["status"] or r["count"] != args.records:
        raise SystemExit(f"bench_bai: the hot path found {r['count']} records (status {r['status']})")
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

    ev = {"bai_scan": [], "records_scan": []}
    wl = {"bai_scan": [], "records_scan": []}
    last = {}
    sz = sb._lib.SbhRecordsSizes()
    import ctypes as C

    def decode():
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(sz)))
        return sz.n

    bsz = sb._lib.SbhBaiSizes()

    def scan():
        sh._c(sb.lib().sbh_bai_scan(sh.h, first, end, C.byref(bsz)))
        return bsz.n_records

    for s in range(args.warmup + args.runs):
        for name, fn in (("bai_scan", scan), ("records_scan", decode)):  # alternating
            e, w, n = timed(fn)
            last[name] = int(n)
            if s >= args.warmup:
                ev[name].append(e)
                wl[name].append(w)
    if last["bai_scan"] != args.records or last["records_scan"] != args.records:
        raise SystemExit(f"bench_bai: record counts differ: {last}")
    runs, lin, n_no_coor = sh.bai_scan(first, end)
    t = time.perf_counter()
    bai = bai_mod.bai_build(runs, lin, contig_len, n_no_coor)
    build_ms = (time.perf_counter() - t) * 1e3
    idx = sb.read_bai(bai)
    mapped = sum(x.metadata.num_mapped + x.metadata.num_unmapped for x in idx.references if x.metadata)
    med = {k: statistics.median(v) for k, v in ev.items()}
    out = {"bench": "bai", "data": f"synthetic config B (tools/synth_bam.c, seed {seed:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": int(end), "timed_calls": args.runs,
           "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median",
           "bai_scan_ms": round(med["bai_scan"], 3), "records_scan_ms": round(med["records_scan"], 3),
           "ratio_scan_over_decode": round(med["bai_scan"] / med["records_scan"], 4),
           "bar": "ratio <= 1.0", "bar_met": bool(med["bai_scan"] <= med["records_scan"]),
           "bai_scan_records_per_s": round(args.records / (med["bai_scan"] * 1e-3)),
           "bai_scan_ms_min_max": [round(min(ev["bai_scan"]), 3), round(max(ev["bai_scan"]), 3)],
           "records_scan_ms_min_max": [round(min(ev["records_scan"]), 3), round(max(ev["records_scan"]), 3)],
           "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()},
           "bai_runs": int(runs.size), "lin_size": int(lin.size), "n_no_coor": int(n_no_coor),
           "bai_bytes": len(bai), "bai_build_ms": round(build_ms, 3), "indexed_records": int(mapped + n_no_coor)}
    sh.close()
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if out["indexed_records"] != args.records:
        raise SystemExit("bench_bai: the index does not account for every record")


if __name__ == "__main__":
    main()
