#!/usr/bin/env python3
"""SAM rendering against the full record decode over the same records, one run.

Input: the benchmark's config-B corpus (tools/synth, seed 0x5B4D0001: 100 bp short reads,
coordinate-sorted, BGZF level 6, 12.4 M records ~ 1 GiB compressed), resident in HBM, after the
hot path (sbh_run_shard) has left the flat bytes, the block table and the eager bitmap on the
device.  Two calls over the whole record range [first record, stream end), alternating:

  records_scan  sbh_records_scan: record starts from the bitmap, then every column of every record
                (records.hip) -- the yardstick: it reads each record once and writes about as many
                bytes
  sam_scan      sbh_records_sam_scan over the rows that decode left: size pass, scan, emit pass
                (sam.hip); the text stays on the device, nothing is fetched.  It reads each record
                twice and writes about 1.1 x the record bytes, so the bar is
                sam_scan <= 2.0 x records_scan

Each library call runs on the shard's own stream and synchronises it before returning, so a call's
time is the time between its entry and its return, host round trips included.  It is taken twice:
by a pair of events recorded on torch's (idle) current stream just before and after the call, and
by the host clock.  After warm-up the medians are reported.  For scale, Reads.sam_lines (the
Python renderer) is timed on the host over a sample of the same records.  Prints one JSON line.
"""
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-sample", type=int, default=100_000, help="records Reads.sam_lines is timed on")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.runs < 10:
        raise SystemExit("bench_sam: at least 10 timed runs")

    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sam: no GPU (a measurement needs one; there is no fallback)")

    seed = 0x5B4D0001
    t0 = time.time()
    p = synth.params(seed, shape=0, level=6, threads=min(16, os.cpu_count() or 1))
    seg = synth.Segment(p, args.records, 1, 0, halo_blocks=16, log=lambda *a: None)
    seg.set_offsets([seg.own_csize])
    comp, size = seg.comp, int(seg.file_size)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    names, contig_len, _ = sb.parse_bam_header(synth.header_bytes())
    packed, off = sb.records.pack_ref_names(names)

    ctx = sb.Context(0)
    sh = ctx.shard(comp, file_offset=0, file_size=size)
    sh.set_contigs(contig_len)
    r = sh.run(0, size)
    if r["status"] or r["count"] != args.records:
        raise SystemExit(f"bench_sam: the hot path found {r['count']} records (status {r['status']})")
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
    ssz = sb._lib.SbhSamSizes()

    def decode():
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        return rsz.n

    def sam():
        sh._c(sb.lib().sbh_records_sam_scan(sh.h, packed.ctypes.data_as(C.c_void_p), off.ctypes.data_as(C.c_void_p),
                                            int(off.size - 1), C.byref(ssz)))
        return ssz.n

    ev = {"records_scan": [], "sam_scan": []}
    wl = {"records_scan": [], "sam_scan": []}
    last = {}
    for s in range(args.warmup + args.runs):
        for name, fn in (("records_scan", decode), ("sam_scan", sam)):  # alternating
            e, w, n = timed(fn)
            last[name] = int(n)
            if s >= args.warmup:
                ev[name].append(e)
                wl[name].append(w)
    if last["records_scan"] != args.records or last["sam_scan"] != args.records:
        raise SystemExit(f"bench_sam: record counts differ: {last}")
    text_bytes, n_host = int(ssz.text_bytes), int(ssz.n_host)
    rec_bytes = int(rsz.name_bytes + 4 * rsz.cigar_ops + (rsz.bases + 1) // 2 + rsz.bases + rsz.aux_bytes
                    + 36 * rsz.n)

    # the Python renderer on a sample of the same records, and the device text of those rows against it
    k = min(args.host_sample, args.records)
    cols = sh.records(first, min(end, first + 400 * k))
    k = min(k, int(cols["flat"].size))
    sample = sb.Reads(sb.records.slice_columns(cols, 0, k), names)
    t = time.perf_counter()
    lines = sample.sam_lines()
    host_s = time.perf_counter() - t
    text, line_off = sh.records_sam(names)
    same = bytes(text[:int(line_off[k])]) == ("\n".join(lines) + "\n").encode("latin-1")

    med = {k_: statistics.median(v) for k_, v in ev.items()}
    out = {"bench": "sam", "data": f"synthetic config B (tools/synth_bam.c, seed {seed:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": int(end), "record_bytes": rec_bytes,
           "text_bytes": text_bytes, "n_host": n_host, "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median",
           "records_scan_ms": round(med["records_scan"], 3), "sam_scan_ms": round(med["sam_scan"], 3),
           "ratio_sam_over_decode": round(med["sam_scan"] / med["records_scan"], 4),
           "bar": "ratio <= 2.0", "bar_met": bool(med["sam_scan"] <= 2.0 * med["records_scan"]),
           "sam_text_GB_per_s": round(text_bytes / (med["sam_scan"] * 1e-3) / 1e9, 2),
           "sam_records_per_s": round(args.records / (med["sam_scan"] * 1e-3)),
           "sam_scan_ms_min_max": [round(min(ev["sam_scan"]), 3), round(max(ev["sam_scan"]), 3)],
           "records_scan_ms_min_max": [round(min(ev["records_scan"]), 3), round(max(ev["records_scan"]), 3)],
           "host_wall_ms_median": {k_: round(statistics.median(v), 3) for k_, v in wl.items()},
           "python_sam_lines_records": k, "python_sam_lines_s": round(host_s, 3),
           "python_sam_lines_s_extrapolated": round(host_s * args.records / max(k, 1), 1),
           "sample_text_equals_python": bool(same)}
    sh.close()
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not same:
        raise SystemExit("bench_sam: the device text of the sample differs from Reads.sam_lines")


if __name__ == "__main__":
    main()
