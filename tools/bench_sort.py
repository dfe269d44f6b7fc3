#!/usr/bin/env python3
"""The coordinate sort against the plain gather and the full record decode, one run.

Inputs, both resident in HBM after the hot path (sbh_run_shard):
  ordered   the benchmark's config-B corpus (tools/synth, seed 0x5B4D0001: 100 bp short reads,
            coordinate-sorted, BGZF level 6, 12.4 M records ~ 1 GiB compressed)
  shuffled  the same records laid out in a fixed random order behind the same header (a gather on
            the device by torch, outside every timed region) and compressed by the library's fast
            coder; `shuffled_records` records the size used (--shuffle-records caps it)

Whole synchronous calls over [first record, stream end), alternating, each timed by a pair of
events on torch's (idle) current stream and by the host clock; medians after warm-up:

  ordered:   records_scan   sbh_records_scan (the decode of every column: the standing yardstick)
             bam_scan       sbh_records_bam_scan, no filter, the BAM header as head
             bam_sorted     sbh_records_bam_scan_order(COORDINATE): no descent, so the key pass and
                            nothing else on top of bam_scan -- the difference is reported
  shuffled:  records_scan   the decode of the same records in their shuffled layout
             bam_scan       the plain gather (one run: the layout is contiguous)
             bam_sorted     the sort: keys, the passes that run, apply, then the gather of runs of
                            about one record.  The bar, with no margin: bam_sorted <= records_scan

A child process under `rocprofv3 --kernel-trace --stats` repeats the sorted call on the shuffled
shard; the kernels of its last call, from k_bam_keep to k_bam_copy, are summed by stage.  With
--e2e-records N the whole api.sort_bam call is timed on a smaller shuffled corpus by the host
clock and its records checked.  Prints one JSON line."""
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

SEED = 0x5B4D0001
STAGES = (("key", ("k_sort_keys",)), ("histogram", ("k_sort_hist",)), ("scan", ("k_scan_local", "k_scan_add")),
          ("scatter", ("k_sort_scatter",)), ("apply", ("k_sort_apply", "k_sort_rows")), ("copy", ("k_bam_copy",)),
          ("keep_heads_index", ("k_bam_keep", "k_bam_heads", "k_bam_index")))


def corpus(synth, records):
    p = synth.params(SEED, shape=0, level=6, threads=min(16, os.cpu_count() or 1))
    seg = synth.Segment(p, records, 1, 0, halo_blocks=16, log=lambda *a: print(*a, file=sys.stderr, flush=True))
    seg.set_offsets([seg.own_csize])
    return seg.comp, int(seg.file_size)


def resident(sb, ctx, comp, size, contig_len, records):
    sh = ctx.shard(comp, file_offset=0, file_size=size)
    sh.set_contigs(contig_len)
    r = sh.run(0, size)
    if r["status"] or r["count"] != records:
        raise SystemExit(f"bench_sort: the hot path found {r['count']} records (status {r['status']})")
    return sh, sh.flat_of(r["first_vpos"] >> 16, r["first_vpos"] & 0xFFFF), sh.flat_bound(size)


def shuffle_file(sb, ctx, sh, first, end, header, n_records, seed):
    """The first n_records records of the shard in a fixed random order, behind the header,
    compressed: (file bytes, the keys' differing digits = passes the sort will run)."""
    import numpy as np
    import torch
    bsz = sb._lib.SbhBamSizes()
    sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(sb._lib.SbhRecordsSizes())))
    sh._c(sb.lib().sbh_records_bam_scan(sh.h, None, 0, None, C.byref(bsz)))
    off = np.zeros(bsz.n_kept + 1, np.uint64)
    sh._c(sb.lib().sbh_records_bam_fetch(sh.h, None, off.ctypes.data_as(C.c_void_p), None))
    off = off[:n_records + 1].astype(np.int64)
    dev = torch.device("cuda")
    flat = torch.from_numpy(sh.bam_read(0, int(off[-1]))).to(dev)  # (head_bytes = 0: the records alone)
    starts, lens = torch.from_numpy(off[:-1]).to(dev), torch.from_numpy(np.diff(off)).to(dev)
    perm = torch.randperm(n_records, generator=torch.Generator().manual_seed(seed)).to(dev)
    out = torch.empty(int(header.size) + int(off[-1]), dtype=torch.uint8, device=dev)
    out[:header.size] = torch.from_numpy(header).to(dev)
    at = int(header.size)
    for a in range(0, n_records, 1 << 20):  # (an index per byte: 2 GB of them per million records)
        p = perm[a:a + (1 << 20)]
        ln, st = lens[p], starts[p]
        dst = torch.cumsum(ln, 0) - ln
        total = int(ln.sum())
        idx = torch.repeat_interleave(st - dst, ln) + torch.arange(total, device=dev)
        out[at:at + total] = flat[idx]
        at += total
        del idx
    torch.cuda.synchronize()
    # the digits that differ among the keys (csrc/bam_sort_core.h), from the fixed fields
    f = flat[(starts[:, None] + torch.arange(4, 20, device=dev)[None, :])].to(torch.int64)
    ref = f[:, 0] | f[:, 1] << 8 | f[:, 2] << 16 | f[:, 3] << 24
    pos1 = ((f[:, 4] | f[:, 5] << 8 | f[:, 6] << 16 | f[:, 7] << 24) + 1) & 0xFFFFFFFF
    ref = torch.where(ref >= 2 ** 31, torch.full_like(ref, 0x7FFFFFFF), ref)
    key = ref << 33 | pos1 << 1 | (f[:, 14] >> 4) & 1  # (< 2^63: fits the signed type)
    differ = 0  # OR & ~AND, bit by bit
    for b in range(63):
        col = (key >> b) & 1
        if int(col.min()) != int(col.max()):
            differ |= 1 << b
    passes = sum(1 for d in range(8) if (differ >> (8 * d)) & 0xFF)
    comp = ctx.bgzf_compress(out.data_ptr(), int(out.numel()), level=sb._lib.LEVEL_FAST)[0]
    return np.ascontiguousarray(comp), passes


def kernel_split(db):
    """The kernels of the trace's last sorted call, summed by stage (ms)."""
    from prof_gaps import load, short
    ks = load(sqlite3.connect(db))
    begin = max(s for s, _, n in ks if short(n) == "k_bam_keep")
    call = [(e - s, short(n)) for s, e, n in ks if s >= begin]
    out = {label: round(sum(d for d, n in call if n in names) / 1e6, 3) for label, names in STAGES}
    known = {n for _, names in STAGES for n in names}
    out["other"] = round(sum(d for d, n in call if n not in known) / 1e6, 3)
    out["launches"] = len(call)
    out["hist_launches"] = sum(1 for _, n in call if n == "k_sort_hist")
    return out


def trace_child(path):
    """Under rocprofv3: the shuffled file resident, one decode, three sorted calls."""
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
        for _ in range(3):
            sh.records_bam(header.tobytes(), None, want_bytes=False, order="coordinate")
        sh.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--shuffle-records", type=int, default=0, help="records of the shuffled shard (0: all of them)")
    ap.add_argument("--runs", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--e2e-records", type=int, default=400_000, help="records of the sort_bam corpus (0: skip)")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 child")
    ap.add_argument("--trace-child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()
    if args.trace_child:
        return trace_child(args.trace_child)
    if args.runs < 10:
        raise SystemExit("bench_sort: at least 10 timed runs")

    import numpy as np
    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sort: no GPU (a measurement needs one; there is no fallback)")

    t0 = time.time()
    comp, size = corpus(synth, args.records)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
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
        rsz, bsz, already = sb._lib.SbhRecordsSizes(), sb._lib.SbhBamSizes(), C.c_int()

        def decode():
            sh._c(sb.lib().sbh_records_scan(sh.h, first, end, C.byref(rsz)))
            return rsz.n

        def plain():
            sh._c(sb.lib().sbh_records_bam_scan(sh.h, hp, int(header.size), None, C.byref(bsz)))
            return bsz.n_kept, bsz.bytes

        def coordinate():
            sh._c(sb.lib().sbh_records_bam_scan_order(sh.h, hp, int(header.size), None, sb._lib.ORDER_COORDINATE,
                                                      C.byref(bsz)))
            sh._c(sb.lib().sbh_records_bam_sorted(sh.h, C.byref(already)))
            return bsz.n_kept, bsz.bytes, already.value

        calls = (("records_scan", decode), ("bam_scan", plain), ("bam_sorted", coordinate))
        ev, wl, last = {k: [] for k, _ in calls}, {k: [] for k, _ in calls}, {}
        for s in range(args.warmup + args.runs):
            for name, fn in calls:  # alternating
                e, w, last[name] = timed(fn)
                if s >= args.warmup:
                    ev[name].append(e)
                    wl[name].append(w)
        med = {k: statistics.median(v) for k, v in ev.items()}
        return med, ev, wl, last

    # ---- the ordered shard
    sh, first, end = resident(sb, ctx, comp, size, contig_len, args.records)
    med, ev, wl, last = measure(sh, first, end)
    if last["bam_sorted"][2] != 1 or last["bam_sorted"][:2] != last["bam_scan"]:
        raise SystemExit(f"bench_sort: the ordered shard was not found in order: {last}")
    out = {"bench": "sort", "data": f"synthetic config B (tools/synth_bam.c, seed {SEED:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": int(end),
           "timed_calls": args.runs, "warmup": args.warmup,
           "timing": "whole synchronous call, host round trips included: events on an idle stream around it; median",
           "ordered": {"records_scan_ms": round(med["records_scan"], 3), "bam_scan_ms": round(med["bam_scan"], 3),
                       "bam_sorted_ms": round(med["bam_sorted"], 3),
                       "fast_path_over_plain_gather_ms": round(med["bam_sorted"] - med["bam_scan"], 3),
                       "already_in_order": True,
                       "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
                       "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}}

    # ---- the same records shuffled
    n_sh = args.shuffle_records or args.records
    t0 = time.time()
    comp2, passes = shuffle_file(sb, ctx, sh, first, end, header, n_sh, seed=SEED & 0xFFFF)
    sh.close()
    del comp
    torch.cuda.empty_cache()
    print(f"shuffled: {n_sh} records, {comp2.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    sh, first, end = resident(sb, ctx, comp2, int(comp2.size), contig_len, n_sh)
    med, ev, wl, last = measure(sh, first, end)
    if last["bam_sorted"][2] != 0 or last["bam_sorted"][:2] != last["bam_scan"]:
        raise SystemExit(f"bench_sort: the shuffled shard: {last}")
    # the sorted stream's keys ascend (the exact order is the tests' business)
    rec_off = np.zeros(n_sh + 1, np.uint64)
    sh._c(sb.lib().sbh_records_bam_fetch(sh.h, None, rec_off.ctypes.data_as(C.c_void_p), None))
    probe = rec_off[:: max(1, n_sh // 4096)][:-1].astype(np.int64)
    fixed = np.stack([sh.bam_read(int(p) + 4, int(p) + 12).view("<i4") for p in probe])
    ref = np.where(fixed[:, 0] < 0, 2 ** 31 - 1, fixed[:, 0]).astype(np.int64)
    probe_key = ref << 33 | ((fixed[:, 1].astype(np.int64) + 1) & 0xFFFFFFFF) << 1
    ascending = bool((np.diff(probe_key) >= 0).all())
    stream_bytes = int(last["bam_sorted"][1])
    out["shuffled"] = {"shuffled_records": n_sh, "comp_bytes": int(comp2.size), "stream_bytes": stream_bytes,
                       "passes_run": passes,
                       "records_scan_ms": round(med["records_scan"], 3), "bam_scan_ms": round(med["bam_scan"], 3),
                       "bam_sorted_ms": round(med["bam_sorted"], 3),
                       "ratio_sorted_over_decode": round(med["bam_sorted"] / med["records_scan"], 4),
                       "bar": "bam_sorted <= records_scan", "bar_met": bool(med["bam_sorted"] <= med["records_scan"]),
                       "sorted_stream_GB_per_s": round(stream_bytes / (med["bam_sorted"] * 1e-3) / 1e9, 2),
                       "sorted_records_per_s": round(n_sh / (med["bam_sorted"] * 1e-3)),
                       "probed_keys_ascend": ascending,
                       "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in ev.items()},
                       "host_wall_ms_median": {k: round(statistics.median(v), 3) for k, v in wl.items()}}
    sh.close()

    # ---- sort_bam end to end, host clock
    if args.e2e_records:
        small, ssize = corpus(synth, args.e2e_records)
        shs, f2, e2 = resident(sb, ctx, small, ssize, contig_len, args.e2e_records)
        small2, _ = shuffle_file(sb, ctx, shs, f2, e2, header, args.e2e_records, seed=7)
        shs.close()
        sb.sort_bam(small2, level=sb._lib.LEVEL_FAST, ctx=ctx)  # (warm: allocations, code objects)
        e2e = {"records": args.e2e_records, "comp_bytes": int(small2.size), "runs": 1,
               "note": "whole api.sort_bam calls by the host clock: load, inflate, eager check, decode, sort, compress"}
        for label, level in (("level5", 5), ("fast", sb._lib.LEVEL_FAST)):
            t = time.perf_counter()
            a = sb.sort_bam(small2, level=level, ctx=ctx)
            e2e[label] = {"sort_bam_s": round(time.perf_counter() - t, 3), "out_bytes": len(a)}
        t = time.perf_counter()
        sb.build_bai(a, ctx=ctx)  # (raises SBH_E_UNSORTED if the output were not in order)
        e2e["build_bai_of_the_output_s"] = round(time.perf_counter() - t, 3)
        out["sort_bam"] = e2e
    ctx.close()

    # ---- the kernel trace of the sorted call, in a process of its own
    if not args.no_trace and shutil.which("rocprofv3"):
        tmp = tempfile.mkdtemp(prefix="bench_sort_")
        try:
            np.save(os.path.join(tmp, "shuffled.npy"), comp2)
            r = subprocess.run(["rocprofv3", "--kernel-trace", "--stats", "-d", tmp, "-o", "run", "--", sys.executable,
                                os.path.abspath(__file__), "--trace-child", os.path.join(tmp, "shuffled.npy")],
                               capture_output=True, text=True, timeout=600)
            dbs = [os.path.join(d, f) for d, _, fs in os.walk(tmp) for f in fs if f.endswith(".db")]
            if r.returncode == 0 and dbs:
                out["shuffled"]["kernel_ms_of_one_sorted_call"] = kernel_split(dbs[0])
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
        raise SystemExit("bench_sort: the sorted stream's probed keys do not ascend")


if __name__ == "__main__":
    main()
