#!/usr/bin/env python3
"""The read-name sort against the coordinate sort and the full record decode, one run.

The corpus and its shuffle are tools/bench_sort.py's, by import: config B (tools/synth, seed
0x5B4D0001, 12.4 M records), resident in HBM after the hot path, first in its own (coordinate)
order, then with the same records in a fixed random order.  On each shard, whole synchronous calls
over [first record, stream end), alternating, each timed by a pair of events on torch's (idle)
current stream and by the host clock; medians after warm-up:

  records_scan   sbh_records_scan (the decode of every column: the standing yardstick)
  bam_sorted     sbh_records_bam_scan_order(COORDINATE)
  bam_named      sbh_records_bam_scan_names; max_name, chunks_run, passes_run of its summary

Names are in order on neither shard (the ordered one is in coordinate order), so the name call sorts
on both.  A child process under `rocprofv3 --kernel-trace --stats` runs three coordinate calls and
three name calls on the shuffled shard; the kernels of the last call of each kind are summed by
stage.  The yardstick is the coordinate call of the same run:

  predicted = bam_sorted + (passes_named - passes_sorted) * per_pass + chunks_run * name_keys
  per_pass  = the coordinate call's histogram + scan + scatter kernel time / its passes
  name_keys = the name call's k_name_keys kernel time / its launches

and the bar is bam_named <= 1.5 * predicted; the ratio to records_scan is reported beside it.
Prints one JSON line; --out also writes it to a file (profiles/name_sort_bench.json)."""
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

from bench_sort import SEED, corpus, resident, shuffle_file  # noqa: E402

STAGES = (("key", ("k_sort_keys",)), ("name_scan", ("k_name_scan",)), ("name_keys", ("k_name_keys",)),
          ("name_groups", ("k_name_groups",)), ("histogram", ("k_sort_hist",)), ("scan", ("k_scan_local", "k_scan_add")),
          ("scatter", ("k_sort_scatter",)), ("apply", ("k_sort_apply", "k_sort_rows")), ("copy", ("k_bam_copy",)),
          ("keep_heads_index", ("k_bam_keep", "k_bam_heads", "k_bam_index")))


def kernel_split(db):
    """The kernels of the trace's last coordinate call and last name call, summed by stage (ms).  A
    call begins at its k_bam_keep; a name call is one that launches k_name_scan."""
    from prof_gaps import load, short
    ks = [(s, e, short(n)) for s, e, n in load(sqlite3.connect(db))]
    begins = [s for s, _, n in ks if n == "k_bam_keep"] + [max(e for _, e, _ in ks) + 1]
    out = {}
    for a, b in zip(begins, begins[1:]):
        call = [(e - s, n) for s, e, n in ks if a <= s < b]
        kind = "named" if any(n == "k_name_scan" for _, n in call) else "sorted"
        split = {label: round(sum(d for d, n in call if n in names) / 1e6, 3) for label, names in STAGES}
        known = {n for _, names in STAGES for n in names}
        split["other"] = round(sum(d for d, n in call if n not in known) / 1e6, 3)
        split["launches"] = len(call)
        split["hist_launches"] = sum(1 for _, n in call if n == "k_sort_hist")
        split["name_keys_launches"] = sum(1 for _, n in call if n == "k_name_keys")
        out[kind] = split  # (the last of its kind stays)
    return out


def trace_child(path):
    """Under rocprofv3: the shuffled file resident, one decode, three calls of each order."""
    import numpy as np
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    comp = np.load(path)
    header = np.frombuffer(synth.header_bytes(), dtype=np.uint8)
    _, contig_len, header_end = sb.parse_bam_header(synth.header_bytes())
    header = np.ascontiguousarray(header[:header_end])
    with sb.Context(0) as ctx:
        sh = ctx.shard(comp, file_offset=0, file_size=int(comp.size))
        sh.set_contigs(contig_len)
        r = sh.run(0, int(comp.size))
        first, end = sh.flat_of(r["first_vpos"] >> 16, r["first_vpos"] & 0xFFFF), sh.flat_bound(int(comp.size))
        sh.records_scan(first, end)
        for order in ("coordinate", "name"):
            for _ in range(3):
                sh.records_bam(header.tobytes(), None, want_bytes=False, order=order)
        sh.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--shuffle-records", type=int, default=0, help="records of the shuffled shard (0: all of them)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.runs < 10:
        raise SystemExit("bench_name_sort: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_name_sort: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr, flush=True)
    header = np.frombuffer(synth.header_bytes(), dtype=np.uint8)
    _, contig_len, header_end = sb.parse_bam_header(synth.header_bytes())
    header = np.ascontiguousarray(header[:header_end])
    hp = header.ctypes.data_as(C.c_void_p)
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

    def measure(sh, first, end):
        rsz, bsz, info = sb._lib.SbhRecordsSizes(), sb._lib.SbhBamSizes(), sb._lib.SbhBamNameInfo()

        def decode():
            sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
            return rsz.n

        def coordinate():
            sh._c(sb.lib().sbh_records_bam_scan_order(sh.h, hp, int(header.size), None, sb._lib.ORDER_COORDINATE,
                                                      C.byref(bsz)))
            return bsz.n_kept, bsz.bytes

        def named():
            sh._c(sb.lib().sbh_records_bam_scan_names(sh.h, hp, int(header.size), None, C.byref(bsz)))
            return bsz.n_kept, bsz.bytes

        calls = (("records_scan", decode), ("bam_sorted", coordinate), ("bam_named", named))
        ev, wl, last = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
        for s in range(args.warmup + args.runs):
            for name, fn in calls:  # alternating
                e, w, last[name] = timed(fn)
                if s >= args.warmup:
                    ev[name].append(e)
                    wl[name].append(w)
        if last["bam_named"] != last["bam_sorted"]:
            raise SystemExit(f"bench_name_sort: the two orders disagree on the stream's size: {last}")
        sh._c(sb.lib().sbh_records_bam_name_info(sh.h, C.byref(info)))  # (the name call ran last)
        summary = {k: int(getattr(info, k)) for k, _ in sb._lib.SbhBamNameInfo._fields_}
        med = {k: statistics.median(v) for k, v in ev.items()}
        return {"records_scan_ms": round(med["records_scan"], 3), "bam_sorted_ms": round(med["bam_sorted"], 3),
                "bam_named_ms": round(med["bam_named"], 3),
                "ratio_named_over_sorted": round(med["bam_named"] / med["bam_sorted"], 4),
                "ratio_named_over_decode": round(med["bam_named"] / med["records_scan"], 4),
                "stream_bytes": int(last["bam_named"][1]), "name_info": summary,
                "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
                "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}

    def names_ascend(sh, n):
        """The name-order stream's probed names ascend (the exact order is the tests' business)."""
        rec_off = np.zeros(n + 1, np.uint64)
        sh._c(sb.lib().sbh_records_bam_fetch(sh.h, None, rec_off.ctypes.data_as(C.c_void_p), None))
        probe = rec_off[:: max(1, n // 4096)][:-1].astype(np.int64)
        names = []
        for p in probe:
            l_read_name = int(sh.bam_read(int(p) + 12, int(p) + 13)[0])
            names.append(sh.bam_read(int(p) + 36, int(p) + 36 + max(l_read_name - 1, 0)).tobytes())
        return all(a <= b for a, b in zip(names, names[1:]))

    # ---- the ordered shard (coordinate order: the names are not in order)
    sh, first, end = resident(sb, ctx, comp, size, contig_len, args.records)
    out = {"bench": "name_sort", "data": f"synthetic config B (tools/synth_bam.c, seed {SEED:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": int(end),
           "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median",
           "ordered": measure(sh, first, end)}
    ascending = names_ascend(sh, args.records)
    out["ordered"]["probed_names_ascend"] = ascending

    # ---- the same records shuffled
    n_sh = args.shuffle_records or args.records
    t0 = time.time()
    comp2, passes = shuffle_file(sb, ctx, sh, first, end, header, n_sh, seed=SEED & 0xFFFF)
    sh.close()
    del comp
    torch.cuda.empty_cache()
    print(f"shuffled: {n_sh} records, {comp2.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr,
          flush=True)
    sh, first, end = resident(sb, ctx, comp2, int(comp2.size), contig_len, n_sh)
    out["shuffled"] = dict(measure(sh, first, end), shuffled_records=n_sh, comp_bytes=int(comp2.size),
                           passes_sorted=passes)
    ok = names_ascend(sh, n_sh)
    out["shuffled"]["probed_names_ascend"] = ok
    ascending = ascending and ok
    sh.close()
    ctx.close()

    # ---- the kernel trace of both calls, in a process of its own, and the prediction
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_name_sort_")
        try:
            np.save(os.path.join(tmp, "shuffled.npy"), comp2)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", os.path.join(tmp, "shuffled.npy")],
                               capture_output=True, text=True, timeout=900)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            if r.returncode == 0 and dbs:
                split = kernel_split(dbs[0])
                out["shuffled"]["kernel_ms_of_one_call"] = split
                S, N, m = split.get("sorted"), split.get("named"), out["shuffled"]
                if S and N and S["hist_launches"] and N["name_keys_launches"]:
                    per_pass = (S["histogram"] + S["scan"] + S["scatter"]) / S["hist_launches"]
                    keys = N["name_keys"] / N["name_keys_launches"]
                    info = m["name_info"]
                    predicted = (m["bam_sorted_ms"] + (info["passes_run"] - S["hist_launches"]) * per_pass
                                 + info["chunks_run"] * keys)
                    m["prediction"] = {"per_pass_ms": round(per_pass, 4), "name_keys_ms": round(keys, 4),
                                       "predicted_ms": round(predicted, 3), "bar": "bam_named <= 1.5 * predicted",
                                       "ratio_named_over_predicted": round(m["bam_named_ms"] / predicted, 4),
                                       "bar_met": bool(m["bam_named_ms"] <= 1.5 * predicted)}
            else:
                out["shuffled"]["kernel_trace_error"] = (r.stderr or "no database")[-400:]
        finally:
            shutil.rmtree(tmp, ignore_errors=True)

    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not ascending:
        raise SystemExit("bench_name_sort: the name-order stream's probed names do not ascend")


if __name__ == "__main__":
    main()
