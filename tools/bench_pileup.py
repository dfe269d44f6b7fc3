#!/usr/bin/env python3
"""Per-base allele counts against their yardsticks, one run.

Inputs, resident in HBM after the hot path (sbh_run_shard), as tools/bench_depth.py builds them:
  ordered   the benchmark's config-B corpus (12.4 M coordinate-sorted 100 bp reads, 3 bases apart)
  shuffled  the same records in a fixed random order (the atomics scatter); reported, no bar

Whole synchronous calls, alternating, each timed by a pair of events on torch's (idle) current
stream and by the host clock; medians of --runs calls after --warmup:

  the add     sbh_records_pileup_add (check, one round trip, events) of every record, all kept, into
              one span over the stretch of reference 0 the records reach, against sbh_records_scan
              of the same records.  The bar, with no margin: add <= records_scan.  The ratio to
              sbh_records_depth_add in the same run is reported, no bar.  Adds per second and added
              bytes per second (4 bytes an add) stand next to the float-atomic rate of the
              microarchitecture notes; that comparison is across types (integer against float).
  the finish  sbh_pileup_finish (calls, fold, scan, intervals) against a device-to-device
              hipMemcpyAsync of the counter array (32 bytes a position).  The bar: finish <= 1.0 x
              the copy.  Every timed finish follows a reset and an add outside the timed region.

Config B keeps every read on one sorted reference; the shuffled run is the only one that shows what
scattered rows cost.  A child process under `rocprofv3 --kernel-trace --stats` repeats reset / add /
finish on the ordered shard; the k_pile_* kernels and the scans of its last round are listed.
Prints one JSON line."""
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

KERNELS = ("k_pile_check", "k_pile_events", "k_pile_calls", "k_pile_fold", "k_pile_intervals", "k_scan_local", "k_scan_add")
FLOAT_ATOMIC_BYTES_PER_S = 1.3e12  # the measured chip-wide rate of no-return float atomic adds, added bytes


def kernel_split(db):
    """The pileup kernels of the trace's last round (from its k_pile_check on), ms each."""
    from prof_gaps import load, short
    ks = load(sqlite3.connect(db))
    begin = max(s for s, _, n in ks if short(n) == "k_pile_check")
    call = [(e - s, short(n)) for s, e, n in ks if s >= begin]
    out = {k: round(sum(d for d, n in call if n == k) / 1e6, 3) for k in KERNELS}
    out["launches"] = len(call)
    return out


def trace_child(path):
    """Under rocprofv3: the ordered file resident, one decode, three rounds of reset / add / finish."""
    import numpy as np
    import synth
    from bench_depth import reach
    from __graft_entry__ import load_package
    sb = load_package()
    comp = np.load(path)
    _, contig_len, _ = sb.parse_bam_header(synth.header_bytes())
    with sb.Context(0) as ctx:
        sh = ctx.shard(comp, file_offset=0, file_size=int(comp.size))
        sh.set_contigs(contig_len)
        r = sh.run(0, int(comp.size))
        first, end = sh.flat_of(r["first_vpos"] >> 16, r["first_vpos"] & 0xFFFF), sh.flat_bound(int(comp.size))
        n = sh.records_scan(first, end)
        beg, stop, _ = reach(sb, sh, n)
        acc = ctx.pileup([(0, beg, stop)], len(contig_len))
        for _ in range(3):
            acc.reset()
            acc.add(sh)
            acc.finish()
        acc.close()
        sh.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--shuffle-records", type=int, default=0, help="records of the shuffled shard (0: all of them)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--min-baseq", type=int, default=0)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.runs < 10:
        raise SystemExit("bench_pileup: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    import bench_sort
    from bench_depth import reach
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pileup: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = bench_sort.corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    header = np.frombuffer(synth.header_bytes(), dtype=np.uint8)
    _, contig_len, header_end = sb.parse_bam_header(synth.header_bytes())
    header = np.ascontiguousarray(header[:header_end])
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

    def rounds(calls, before=None):
        """Alternating timed calls; `before` runs untimed ahead of every round."""
        ev, wl, last = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
        for s in range(args.warmup + args.runs):
            if before:
                before()
            for name, fn in calls:
                e, w, last[name] = timed(fn)
                if s >= args.warmup:
                    ev[name].append(e)
                    wl[name].append(w)
        return {k: statistics.median(v) for k, v in ev.items()}, ev, wl, last

    def copy_of(nbytes):
        src = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
        dst = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        # (contiguous, one dtype, one device: torch issues hipMemcpyAsync device-to-device on its stream)
        def copy():
            dst.copy_(src, non_blocking=True)
        return copy

    def spread(ev, wl):
        return {"ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
                "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}

    def measure(sh, first, end, n_records, with_finish):
        rsz = sb._lib.SbhRecordsSizes()
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        beg, stop, on0 = reach(sb, sh, rsz.n)
        acc = ctx.pileup([(0, beg, stop)], len(contig_len), args.min_baseq)
        dep = ctx.depth([(0, beg, stop)], len(contig_len))

        def decode():
            sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
            return rsz.n

        med, ev, wl, last = rounds((("records_scan", decode), ("depth_add", lambda: dep.add(sh)),
                                    ("pileup_add", lambda: acc.add(sh))))
        dep.close()
        add = last["pileup_add"]
        if add["n_kept"] != n_records or add["n_counted"] != on0:
            raise SystemExit(f"bench_pileup: the add kept {add}")
        adds = sum(add["totals"])
        if adds - add["totals"][5] - add["totals"][6] != last["depth_add"]["cov_bases"]:
            raise SystemExit(f"bench_pileup: {add} does not add up to depth's {last['depth_add']}")
        s = med["pileup_add"] * 1e-3
        out = {"records": n_records, "span": [0, beg, stop], "positions": stop - beg, "add": add,
               "records_scan_ms": round(med["records_scan"], 3), "depth_add_ms": round(med["depth_add"], 3),
               "pileup_add_ms": round(med["pileup_add"], 3),
               "ratio_add_over_decode": round(med["pileup_add"] / med["records_scan"], 4),
               "ratio_add_over_depth_add": round(med["pileup_add"] / med["depth_add"], 3),
               "adds": adds, "adds_per_s": round(adds / s), "added_bytes_per_s": round(4 * adds / s),
               "float_atomic_added_bytes_per_s_for_comparison_across_types": FLOAT_ATOMIC_BYTES_PER_S,
               "add_records_per_s": round(n_records / s), **spread(ev, wl)}
        if with_finish:
            def fresh():
                acc.reset()
                acc.add(sh)
            copy = copy_of(32 * (stop - beg))
            med, ev, wl, last = rounds((("pileup_finish", acc.finish), ("copy", copy)), before=fresh)
            sizes = last["pileup_finish"]
            if sizes["totals"] != add["totals"]:
                raise SystemExit(f"bench_pileup: the finish saw {sizes['totals']}, the add put in {add['totals']}")
            met = bool(med["pileup_finish"] <= med["copy"])
            out["finish"] = {"sizes": sizes, "pileup_finish_ms": round(med["pileup_finish"], 3),
                             "copy_ms": round(med["copy"], 4), "copy_bytes": 32 * (stop - beg),
                             "ratio_finish_over_copy": round(med["pileup_finish"] / med["copy"], 3),
                             "bar": "pileup_finish <= 1.0 x copy", "bar_met": met, **spread(ev, wl)}
            print("finish bar (finish <= copy): %s" % ("met" if met else "missed"), file=sys.stderr)
        acc.close()
        return out

    # ---- the ordered shard
    sh, first, end = bench_sort.resident(sb, ctx, comp, size, contig_len, args.records)
    out = {"bench": "pileup", "data": f"synthetic config B (tools/synth_bam.c, seed {bench_sort.SEED:#x}), resident in HBM",
           "comp_bytes": int(comp.size), "flat_bytes": int(end), "timed_calls": args.runs, "warmup": args.warmup,
           "min_baseq": args.min_baseq, "layout": "position-major, uint32 [positions][8]",
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median"}
    out["ordered"] = measure(sh, first, end, args.records, True)
    out["ordered"]["bar"] = "pileup_add <= records_scan"
    out["ordered"]["bar_met"] = bool(out["ordered"]["pileup_add_ms"] <= out["ordered"]["records_scan_ms"])
    print("add bar (add <= decode): %s" % ("met" if out["ordered"]["bar_met"] else "missed"), file=sys.stderr)

    # ---- the same records shuffled (reported, no bar)
    n_sh = args.shuffle_records or args.records
    comp2, _ = bench_sort.shuffle_file(sb, ctx, sh, first, end, header, n_sh, seed=bench_sort.SEED & 0xFFFF)
    sh.close()
    torch.cuda.empty_cache()
    sh, first2, end2 = bench_sort.resident(sb, ctx, comp2, int(comp2.size), contig_len, n_sh)
    out["shuffled"] = measure(sh, first2, end2, n_sh, False)
    sh.close()
    del comp2
    torch.cuda.empty_cache()
    ctx.close()

    # ---- the kernel trace, in a process of its own
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_pileup_")
        try:
            np.save(os.path.join(tmp, "ordered.npy"), comp)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", os.path.join(tmp, "ordered.npy")],
                               capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            if r.returncode == 0 and dbs:
                out["ordered"]["kernel_ms_of_one_add_and_finish"] = kernel_split(dbs[0])
            else:
                out["ordered"]["kernel_trace_error"] = (r.stderr or "no database")[-400:]
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
