#!/usr/bin/env python3
"""The flag and per-reference counts (sbh_records_tally_add) against their yardsticks, one run.

Inputs, resident in HBM after the hot path (sbh_run_shard), as tools/bench_depth.py builds them:
  ordered   the benchmark's config-B corpus (12.4 M coordinate-sorted 100 bp reads): nearly every
            wave sits on one reference, the wave-uniform path
  shuffled  the same records in a fixed random order; reported, no bar

Whole synchronous calls, alternating, each timed by a pair of events on torch's (idle) current
stream and by the host clock; medians of --runs calls after --warmup:

  the add          sbh_records_tally_add of every record, all kept (two memsets, k_tally_rows, one
                   round trip, k_tally_commit), against sbh_records_scan of the same records.  The
                   bar, with no margin: add <= records_scan.
  against depth    the same add against sbh_records_depth_add into one span over the stretch of
                   reference 0 the records reach; reported, no bar
  many references  the same add into an accumulator of 200 000 references, where 2 (n_ref + 1)
                   counters do not fit the LDS budget and mixed waves count by global atomics;
                   reported, no bar

A child process under `rocprofv3 --kernel-trace --stats` repeats the add on the ordered shard; the
k_tally_* kernels of its last add are listed.  Prints one JSON line."""
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

KERNELS = ("k_tally_rows", "k_tally_commit")
MANY_REFS = 200_000


def kernel_split(db):
    """The tally kernels of the trace's last add (from its k_tally_rows on), ms each."""
    from prof_gaps import load, short
    ks = load(sqlite3.connect(db))
    begin = max(s for s, _, n in ks if short(n) == "k_tally_rows")
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
        acc = ctx.tally(len(contig_len))
        for _ in range(3):
            acc.add(sh)
        acc.close()
        sh.close()


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
        raise SystemExit("bench_tally: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    import bench_sort
    from bench_depth import reach
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tally: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = bench_sort.corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    header = np.frombuffer(synth.header_bytes(), dtype=np.uint8)
    _, contig_len, header_end = sb.parse_bam_header(synth.header_bytes())
    header = np.ascontiguousarray(header[:header_end])
    n_ref = len(contig_len)
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

    def measure(sh, first, end, n_records, full):
        rsz = sb._lib.SbhRecordsSizes()
        sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
        acc, many = ctx.tally(n_ref), ctx.tally(MANY_REFS)

        def decode():
            sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
            return rsz.n

        calls = [("records_scan", decode), ("tally_add", lambda: acc.add(sh)), ("tally_add_many_refs", lambda: many.add(sh))]
        dep = None
        if full:
            beg, stop, _ = reach(sb, sh, rsz.n)
            dep = ctx.depth([(0, beg, stop)], n_ref)
            calls.append(("depth_add", lambda: dep.add(sh)))
        med, ev, wl, last = rounds(calls)
        if last["tally_add"] != {"n": n_records, "n_kept": n_records} or last["tally_add_many_refs"] != last["tally_add"]:
            raise SystemExit(f"bench_tally: the add kept {last['tally_add']}")
        flag, ref = acc.counts()
        _, ref_many = many.counts()
        calls_made = args.warmup + args.runs
        # every add of the run counted every record, on either path
        if int(flag[0].sum()) != calls_made * n_records or int(ref.sum()) != calls_made * n_records \
                or not np.array_equal(ref[:-1], ref_many[:n_ref]) or not np.array_equal(ref[-1], ref_many[-1]):
            raise SystemExit("bench_tally: the counts of the run do not add up")
        out = {"records": n_records, "references": n_ref, "add": last["tally_add"],
               "flag_counts_of_one_add": (flag // calls_made).tolist(),
               "references_in_use": int((ref.sum(axis=1) > 0).sum()),
               "records_scan_ms": round(med["records_scan"], 3), "tally_add_ms": round(med["tally_add"], 3),
               "ratio_add_over_decode": round(med["tally_add"] / med["records_scan"], 4),
               "add_records_per_s": round(n_records / (med["tally_add"] * 1e-3)),
               "tally_add_many_refs_ms": round(med["tally_add_many_refs"], 3), "many_refs": MANY_REFS,
               "ratio_many_refs_over_decode": round(med["tally_add_many_refs"] / med["records_scan"], 4),
               "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
               "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}
        if dep is not None:
            out["depth_add_ms"] = round(med["depth_add"], 3)
            out["ratio_add_over_depth_add"] = round(med["tally_add"] / med["depth_add"], 4)
            dep.close()
        acc.close()
        many.close()
        return out

    # ---- the ordered shard
    sh, first, end = bench_sort.resident(sb, ctx, comp, size, contig_len, args.records)
    out = {"bench": "tally", "data": f"synthetic config B (tools/synth_bam.c, seed {bench_sort.SEED:#x}), resident in HBM",
           "comp_bytes": int(comp.size), "flat_bytes": int(end), "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median"}
    out["ordered"] = measure(sh, first, end, args.records, True)
    out["ordered"]["bar"] = "tally_add <= records_scan"
    out["ordered"]["bar_met"] = bool(out["ordered"]["tally_add_ms"] <= out["ordered"]["records_scan_ms"])

    # ---- the same records shuffled (reported, no bar)
    if not args.no_shuffle:
        n_sh = args.shuffle_records or args.records
        comp2, _ = bench_sort.shuffle_file(sb, ctx, sh, first, end, header, n_sh, seed=bench_sort.SEED & 0xFFFF)
        sh.close()
        torch.cuda.empty_cache()
        sh, first2, end2 = bench_sort.resident(sb, ctx, comp2, int(comp2.size), contig_len, n_sh)
        out["shuffled"] = measure(sh, first2, end2, n_sh, False)
        del comp2
    sh.close()
    torch.cuda.empty_cache()
    ctx.close()

    # ---- the kernel trace, in a process of its own
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_tally_")
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
