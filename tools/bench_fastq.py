#!/usr/bin/env python3
"""The FASTQ text (sbh_records_fastq_scan) against its yardstick, one run.

Input, resident in HBM after the hot path (sbh_run_shard), as tools/bench_tally.py builds it: the
benchmark's config-B corpus (12.4 M coordinate-sorted 100 bp reads).

Whole synchronous calls, alternating, each timed by a pair of events on torch's (idle) current
stream and by the host clock; medians of --runs calls after --warmup:

  the scan         sbh_records_fastq_scan of every record, all kept, one stream in row order with
                   /1 /2 suffixes, the text left on the device (two memsets, k_fastq_sizes, two scans,
                   k_fastq_index, one round trip, k_fastq_emit), against sbh_records_scan of the same
                   records.  The bar, with no margin: fastq_scan <= records_scan.
  split            the same with SBH_FASTQ_SPLIT (three columns, six scans); reported, no bar
  fasta            the same with SBH_FASTQ_FASTA; reported, no bar
  half reversed    the same records with flag 0x10 cleared in every even row and set in every odd row
                   (patched in HBM; the record starts do not move); reported, no bar

A child process under `rocprofv3 --kernel-trace --stats` repeats the scan; the kernels of its last
scan are listed by name.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import shutil
import sqlite3
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def kernel_split(db):
    """Every kernel of the trace's last FASTQ scan (from its k_fastq_sizes on), ms by name."""
    from prof_gaps import load, short
    ks = load(sqlite3.connect(db))
    begin = max(s for s, _, n in ks if short(n) == "k_fastq_sizes")
    out = {}
    for s, e, n in ks:
        if s >= begin:
            out[short(n)] = round(out.get(short(n), 0.0) + (e - s) / 1e6, 4)
    out["launches"] = sum(1 for s, _, _ in ks if s >= begin)
    return out


def trace_child(path):
    """Under rocprofv3: the file resident, one decode, three scans."""
    import numpy as np
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    comp = np.load(path)
    _, contig_len, _ = sb.parse_bam_header(synth.header_bytes())
    with sb.Context(0) as ctx:
        sh = ctx.shard(comp, file_offset=0, file_size=int(comp.size))
        sh.set_contigs(contig_len)
        r = sh.run(0, int(comp.size))
        first, end = sh.flat_of(r["first_vpos"] >> 16, r["first_vpos"] & 0xFFFF), sh.flat_bound(int(comp.size))
        sh.records_scan(first, end)
        for _ in range(3):
            sh.records_fastq(want_text=False)
        sh.close()


class _DeviceBytes:
    """n bytes at a device pointer, for torch.as_tensor."""

    def __init__(self, ptr, n):
        self.__cuda_array_interface__ = {"shape": (int(n),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.runs < 10:
        raise SystemExit("bench_fastq: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    import bench_sort
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fastq: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = bench_sort.corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    _, contig_len, _ = sb.parse_bam_header(synth.header_bytes())
    ctx = sb.Context(0)

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

    def rounds(calls):
        """Alternating timed calls."""
        ev, wl, last = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
        for s in range(args.warmup + args.runs):
            for name, fn in calls:
                e, w, last[name] = timed(fn)
                if s >= args.warmup:
                    ev[name].append(e)
                    wl[name].append(w)
        return {k: statistics.median(v) for k, v in ev.items()}, ev, wl, last

    sh, first, end = bench_sort.resident(sb, ctx, comp, size, contig_len, args.records)
    rsz = sb._lib.SbhRecordsSizes()

    def decode():
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        return rsz.n

    def scan(**kw):
        def fn():
            sh.records_fastq(want_text=False, **kw)
            return dict(sh.fastq_sizes)
        return fn

    def digest():
        """Of the text on the device: its byte sum and newline count (torch, on the GPU)."""
        t = torch.as_tensor(_DeviceBytes(sh.fastq_ptr(), sh.fastq_sizes["text_bytes"]), device="cuda")
        return int(t.sum(dtype=torch.int64)), int((t == 10).sum())

    def measure(calls):
        decode()
        med, ev, wl, last = rounds([("records_scan", decode)] + calls)
        out = {"records_scan_ms": round(med["records_scan"], 3)}
        for name, _ in calls:
            sz = last[name]
            if sz["n"] != args.records or sz["n_kept"] != args.records:
                raise SystemExit(f"bench_fastq: {name} kept {sz}")
            out[name] = {"ms": round(med[name], 3), "ratio_over_decode": round(med[name] / med["records_scan"], 4),
                         "text_bytes": sz["text_bytes"], "part_rows": sz["part_rows"],
                         "text_GB_per_s": round(sz["text_bytes"] / (med[name] * 1e-3) / 1e9, 1)}
        out["ms_min_max"] = {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()}
        out["host_wall_ms_median"] = {k: round(statistics.median(v), 3) for k, v in wl.items()}
        return out

    record_bytes = int(end - first)
    out = {"bench": "fastq", "data": f"synthetic config B (tools/synth_bam.c, seed {bench_sort.SEED:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "record_bytes": record_bytes, "timed_calls": args.runs,
           "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median"}
    o = measure([("fastq_scan", scan()), ("fastq_scan_split", scan(split=True)), ("fastq_scan_fasta", scan(fasta=True))])
    o["text_bytes_over_record_bytes"] = round(o["fastq_scan"]["text_bytes"] / record_bytes, 4)
    o["split_extra_ms"] = round(o["fastq_scan_split"]["ms"] - o["fastq_scan"]["ms"], 3)
    o["bar"] = "fastq_scan <= records_scan"
    o["bar_met"] = bool(o["fastq_scan"]["ms"] <= o["records_scan_ms"])
    out["as_generated"] = o

    # ---- the same records, half of them reverse-strand (reported, no bar)
    try:
        decode()
        both = np.empty(2 * rsz.n, np.uint64)
        ro = sb._lib.SbhRecordsOut(flat=both.ctypes.data, vpos=both[rsz.n:].ctypes.data)
        sh._c(sb.lib().sbh_records_fetch(sh.h, C.byref(ro)))
        starts = both[:rsz.n].astype(np.int64)
        flat = torch.as_tensor(_DeviceBytes(sh.flat_ptr(), int(end)), device="cuda")
        at = torch.from_numpy(starts + 18).cuda()
        before = int(((flat[at] & 0x10) != 0).sum())
        scan()()
        sum_before = digest()
        flat[at[0::2]] &= 0xEF
        flat[at[1::2]] |= 0x10
        torch.cuda.synchronize()
        h = measure([("fastq_scan", scan())])
        h["reverse_rows_as_generated"], h["reverse_rows_now"] = before, int(((flat[at] & 0x10) != 0).sum())
        # the text changed, its size and line count did not
        sum_after = digest()
        h["text_changed"] = bool(sum_after[0] != sum_before[0])
        h["newlines"] = [sum_before[1], sum_after[1]]
        out["half_reversed"] = h
        del flat, at
    except Exception as err:  # (a torch without __cuda_array_interface__ import: not measured)
        out["half_reversed"] = {"not_measured": repr(err)[:300]}
    sh.close()
    torch.cuda.empty_cache()
    ctx.close()

    # ---- the kernel trace, in a process of its own
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_fastq_")
        try:
            np.save(os.path.join(tmp, "ordered.npy"), comp)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", os.path.join(tmp, "ordered.npy")],
                               capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            if r.returncode == 0 and dbs:
                out["as_generated"]["kernel_ms_of_one_scan"] = kernel_split(dbs[0])
            else:
                out["as_generated"]["kernel_trace_error"] = (r.stderr or "no database")[-400:]
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
