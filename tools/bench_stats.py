#!/usr/bin/env python3
"""The read-level statistics (sbh_records_stats_add) against their yardstick, one run.

Inputs, resident in HBM after the hot path (sbh_run_shard), as tools/bench_tally.py builds them:
  ordered   the benchmark's config-B corpus (12.4 M coordinate-sorted 100 bp reads)
  shuffled  the same records in a fixed random order; reported, no bar

Whole synchronous calls, alternating, each timed by a pair of events on torch's (idle) current
stream and by the host clock; medians of --runs calls after --warmup:

  the add          sbh_records_stats_add of every record, all kept, at the default parameters (two
                   memsets, k_stats_rows, k_stats_bases, one round trip, k_stats_commit), against
                   sbh_records_scan of the same records.  The bar, with no margin: add <= records_scan.
  cycles 8         the same add into an accumulator of 8 cycles: nearly every base lands in the
                   overflow row of the per-cycle tables, a wave's 64 adds in the cells of one row --
                   the worst contention the definition allows; reported, no bar

An increment is one add of one into a table: per counted read its read_len, mapq (mapped), isize (one
of a pair) and gc entries, per base its base entry and, with qualities, its qual entry -- counted from
the fetched tables.  A child process under `rocprofv3 --kernel-trace --stats` repeats the add on the
ordered shard; the k_stats_* kernels of its last add are listed.  Prints one JSON line."""
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

KERNELS = ("k_stats_rows", "k_stats_bases", "k_stats_commit")
WORST_CYCLES = 8


def kernel_split(db):
    """The stats kernels of the trace's last add (from its k_stats_rows on), ms each."""
    from prof_gaps import load, short
    ks = load(sqlite3.connect(db))
    begin = max(s for s, _, n in ks if short(n) == "k_stats_rows")
    call = [(e - s, short(n)) for s, e, n in ks if s >= begin]
    out = {k: round(sum(d for d, n in call if n == k) / 1e6, 4) for k in KERNELS}
    out["launches"] = len(call)
    return out


def trace_child(path):
    """Under rocprofv3: the ordered file resident, one decode, three adds."""
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
        acc = ctx.stats()
        for _ in range(3):
            acc.add(sh)
        acc.close()
        sh.close()


def increments(t):
    return int(t["read_len"].sum() + t["mapq"].sum() + t["isize"].sum() + t["gc"].sum() + t["base"].sum() + t["qual"].sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--shuffle-records", type=int, default=0, help="records of the shuffled shard (0: all of them)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-shuffle", action="store_true", help="skip the shuffled shard")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.runs < 10:
        raise SystemExit("bench_stats: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    import bench_sort
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stats: no GPU (a measurement needs one; there is no fallback)")

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

    def measure(sh, first, end, n_records):
        rsz = sb._lib.SbhRecordsSizes()
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        acc, worst = ctx.stats(), ctx.stats(WORST_CYCLES, 8000)

        def decode():
            sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
            return rsz.n

        med, ev, wl, last = rounds([("records_scan", decode), ("stats_add", lambda: acc.add(sh)),
                                    ("stats_add_cycles_8", lambda: worst.add(sh))])
        if last["stats_add"]["n_kept"] != n_records or last["stats_add_cycles_8"] != last["stats_add"]:
            raise SystemExit(f"bench_stats: the add kept {last['stats_add']}")
        t, tw = acc.counts(), worst.counts()
        calls_made = args.warmup + args.runs
        sn = dict(zip(sb.SN_ROWS, (int(x) for x in t["sn"])))
        # every add of the run counted every record and every base, on either accumulator
        if sn["sequences"] != calls_made * last["stats_add"]["n_counted"] or int(t["base"].sum()) != sn["total_length"] \
                or int(tw["base"].sum()) != sn["total_length"] or not np.array_equal(t["gc"], tw["gc"]) \
                or not np.array_equal(t["qual"].sum(axis=1), tw["qual"].sum(axis=1)) or not np.array_equal(t["isize"], tw["isize"]):
            raise SystemExit("bench_stats: the tables of the run do not add up")
        inc = increments(t) // calls_made
        out = {"records": n_records, "add": last["stats_add"], "cycles": acc.cycles, "max_insert": acc.max_insert,
               "sn_of_one_add": {k: (v // calls_made if k != "max_length" else v) for k, v in sn.items()},
               "records_scan_ms": round(med["records_scan"], 3), "stats_add_ms": round(med["stats_add"], 3),
               "ratio_add_over_decode": round(med["stats_add"] / med["records_scan"], 4),
               "increments": inc, "increments_per_s": round(inc / (med["stats_add"] * 1e-3)),
               "add_records_per_s": round(n_records / (med["stats_add"] * 1e-3)),
               "stats_add_cycles_8_ms": round(med["stats_add_cycles_8"], 3),
               "ratio_cycles_8_over_decode": round(med["stats_add_cycles_8"] / med["records_scan"], 4),
               "bases_in_the_overflow_row_at_cycles_8": int(tw["base"][WORST_CYCLES].sum()) // calls_made,
               "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
               "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}
        acc.close()
        worst.close()
        return out

    # ---- the ordered shard
    sh, first, end = bench_sort.resident(sb, ctx, comp, size, contig_len, args.records)
    out = {"bench": "stats", "data": f"synthetic config B (tools/synth_bam.c, seed {bench_sort.SEED:#x}), resident in HBM",
           "comp_bytes": int(comp.size), "flat_bytes": int(end), "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median"}
    out["ordered"] = measure(sh, first, end, args.records)
    out["ordered"]["bar"] = "stats_add <= records_scan"
    out["ordered"]["bar_met"] = bool(out["ordered"]["stats_add_ms"] <= out["ordered"]["records_scan_ms"])
    try:
        with open(os.path.join(ROOT, "profiles", "pileup_bench.json")) as f:
            out["pileup_add_ms_of_profiles_pileup_bench_json"] = json.load(f)["ordered"]["pileup_add_ms"]
    except (OSError, KeyError, ValueError):
        pass

    # ---- the same records shuffled (reported, no bar)
    if not args.no_shuffle:
        n_sh = args.shuffle_records or args.records
        comp2, _ = bench_sort.shuffle_file(sb, ctx, sh, first, end, header, n_sh, seed=bench_sort.SEED & 0xFFFF)
        sh.close()
        torch.cuda.empty_cache()
        sh, first2, end2 = bench_sort.resident(sb, ctx, comp2, int(comp2.size), contig_len, n_sh)
        out["shuffled"] = measure(sh, first2, end2, n_sh)
        del comp2
    sh.close()
    torch.cuda.empty_cache()
    ctx.close()

    # ---- the kernel trace, in a process of its own
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_stats_")
        try:
            np.save(os.path.join(tmp, "ordered.npy"), comp)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", os.path.join(tmp, "ordered.npy")],
                               capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            if r.returncode == 0 and dbs:
                out["ordered"]["kernel_ms_of_one_add"] = kernel_split(dbs[0])
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
