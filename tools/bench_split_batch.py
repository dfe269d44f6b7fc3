#!/usr/bin/env python3
"""Record delivery per FileSplit against batched delivery (sbh_split_records_batch), one run.

Input: the benchmark's config-B corpus (tools/synth, seed 0x5B4D0001: 100 bp short reads, BGZF
level 6, 12.4 M records ~ 1 GiB compressed), resident in HBM, cut into 32 MiB Hadoop FileSplits.
Every path delivers every split's record starts and their virtual positions (decode = 0, what
jni/Native.scala's record iterator asks for; --decode adds the decoded columns) through
spark_bam_amd.canloadbam.SplitWorker, the twin of the Scala task's worker:

  per_split_t1 / per_split_tN   one sbh_split_records per split (SplitWorker.split), one task
                                thread / N task threads sharing the context
  batch8                        SplitWorker.split_batch over 8 consecutive splits at a time, one thread
  batch8_tM                     the same groups of 8 taken by M task threads (M = groups, at most N)
  batch_all                     one split_batch over every split
  step                          the single-shard step for scale: sbh_run_shard over the resident file +
                                sbh_split_starts for all splits (counts only: no record starts)

The paths alternate inside every step (warm-up steps first, so each worker's device buffers have
reached their size); times are host-clock walls around calls that end in a stream synchronise.
The batched lines carry their host-side breakdown, summed over the groups of the last timed
step: the library call, the copy-out of the starts, the per-split copies.
The per-split counts of all paths must agree.  Prints one JSON line.
"""
import argparse
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--records", type=int, default=12_400_000, help="records of the corpus (config B: 12.4 M)")
    ap.add_argument("--split", type=int, default=32 << 20, help="FileSplit size in compressed bytes")
    ap.add_argument("--threads", type=int, default=8, help="task threads of the threaded per-split line")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--decode", action="store_true", help="deliver the decoded columns, not only the starts")
    ap.add_argument("--out", help="also write the JSON line to this file")
    args = ap.parse_args()

    import torch
    import synth
    from __graft_entry__ import load_package
    sb = load_package()
    clb = __import__(sb.__name__ + ".canloadbam", fromlist=["x"])
    sharded = __import__(sb.__name__ + ".sharded", fromlist=["x"])
    if not torch.cuda.is_available():
        raise SystemExit("bench_split_batch: no GPU (a measurement needs one; there is no fallback)")

    seed = 0x5B4D0001
    t0 = time.time()
    p = synth.params(seed, shape=0, level=6, threads=min(16, os.cpu_count() or 1))
    seg = synth.Segment(p, args.records, 1, 0, halo_blocks=16, log=lambda *a: None)
    seg.set_offsets([seg.own_csize])
    comp, size = seg.comp, int(seg.file_size)
    print(f"corpus: {comp.size / 2**30:.3f} GiB compressed in {time.time() - t0:.1f}s", file=sys.stderr)
    _, contig_len, _ = sb.parse_bam_header(synth.header_bytes())
    splits = sb.file_splits(size, args.split)
    read = sharded.bytes_reader(comp)
    decode = bool(args.decode)

    ctx = sb.Context(0)
    dev = torch.from_numpy(comp).to("cuda")
    torch.cuda.synchronize()
    dptr = dev.data_ptr()
    pool = [clb.SplitWorker(ctx, size, contig_len, device_file=dptr) for _ in range(args.threads)]
    m = max(1, min(args.threads, (len(splits) + 7) // 8))
    wb8 = [clb.SplitWorker(ctx, size, contig_len, device_file=dptr) for _ in range(m)]
    wall_ = clb.SplitWorker(ctx, size, contig_len, device_file=dptr)
    resident = ctx.shard(dptr, file_offset=0, file_size=size, on_device=True, nbytes=size)
    resident.set_contigs(contig_len)
    info = {}

    def per_split(nthreads):
        counts = [None] * len(splits)
        it = iter(range(len(splits)))
        lock = threading.Lock()
        errs = []

        def task(w):
            try:
                while True:
                    with lock:
                        i = next(it, None)
                    if i is None:
                        return
                    counts[i] = int(w.split(read, "bench.bam", *splits[i], decode=decode)["vpos"].size)
            except BaseException as e:  # noqa: B902
                errs.append(e)

        t = time.perf_counter()
        if nthreads == 1:
            task(pool[0])
        else:
            ts = [threading.Thread(target=task, args=(w,)) for w in pool[:nthreads]]
            for x in ts:
                x.start()
            for x in ts:
                x.join()
        wall = time.perf_counter() - t
        if errs:
            raise errs[0]
        return wall, counts

    parts = {}  # path -> {ms_call, ms_fetch, ms_slice} of its last pass, summed over the groups

    def batched(name, ws, k):
        groups = [range(i, min(i + k, len(splits))) for i in range(0, len(splits), k)]
        counts = [None] * len(splits)
        it = iter(groups)
        lock = threading.Lock()
        errs = []
        acc = {"ms_call": 0.0, "ms_fetch": 0.0, "ms_slice": 0.0}

        def task(w):
            try:
                while True:
                    with lock:
                        g = next(it, None)
                    if g is None:
                        return
                    cols = w.split_batch(read, "bench.bam", [splits[i] for i in g], decode=decode)
                    for i, c in zip(g, cols):
                        counts[i] = int(c["vpos"].size)
                    with lock:
                        for key in acc:
                            acc[key] += w.last_batch[key]
                        info.update(w.last_batch)
            except BaseException as e:  # noqa: B902
                errs.append(e)

        t = time.perf_counter()
        if len(ws) == 1:
            task(ws[0])
        else:
            ts = [threading.Thread(target=task, args=(w,)) for w in ws]
            for x in ts:
                x.start()
            for x in ts:
                x.join()
        wall = time.perf_counter() - t
        if errs:
            raise errs[0]
        parts[name] = {key: round(v, 3) for key, v in acc.items()}
        return wall, counts

    def step():
        t = time.perf_counter()
        r = resident.run(0, size)
        status, _, n, _ = resident.split_starts(splits)
        wall = time.perf_counter() - t
        assert not status.any() and int(n.sum()) == r["count"]
        return wall, [int(x) for x in n]

    paths = {
        "per_split_t1": lambda: per_split(1),
        f"per_split_t{args.threads}": lambda: per_split(args.threads),
        "batch8": lambda: batched("batch8", wb8[:1], 8),
        f"batch8_t{m}": lambda: batched(f"batch8_t{m}", wb8, 8),
        "batch_all": lambda: batched("batch_all", [wall_], len(splits)),
        "step": step,
    }
    walls = {k: [] for k in paths}
    counts = {}
    for s in range(args.warmup + args.steps):
        for name, fn in paths.items():  # (alternating: every path sees the same neighbours on the machine)
            wall, c = fn()
            counts[name] = c
            if s >= args.warmup:
                walls[name].append(wall)
    first = counts["per_split_t1"]
    match = all(c == first for c in counts.values()) and sum(first) == args.records
    flat = int(info["flat_size"])
    out = {"bench": "split_batch", "data": f"synthetic config B (tools/synth_bam.c, seed {seed:#x}), resident in HBM",
           "records": args.records, "comp_bytes": int(comp.size), "flat_bytes": flat, "splits": len(splits),
           "split_bytes": args.split, "decode": decode, "steps": args.steps, "warmup": args.warmup,
           "records_match": bool(match), "n_host_batch_all": int(info["n_host"]), "paths": {}}
    for name, w in walls.items():
        w = sorted(w)
        med = w[len(w) // 2]
        out["paths"][name] = {"ms_median": round(med * 1e3, 3), "ms_min": round(w[0] * 1e3, 3),
                              "ms_max": round(w[-1] * 1e3, 3), "GBps_decompressed": round(flat / med / 1e9, 2),
                              "ms_per_split": round(med * 1e3 / len(splits), 3)}
    base = out["paths"][f"per_split_t{args.threads}"]["GBps_decompressed"]
    for name in parts:
        out["paths"][name]["host_ms"] = parts[name]
        out["paths"][name]["x_per_split_threads"] = round(out["paths"][name]["GBps_decompressed"] / base, 3)
        out["paths"][name]["frac_of_step"] = round(out["paths"][name]["GBps_decompressed"] /
                                                   out["paths"]["step"]["GBps_decompressed"], 3)
    for w in pool + wb8 + [wall_]:
        w.close()
    resident.close()
    ctx.close()
    line = json.dumps(out)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)
    if not match:
        raise SystemExit("bench_split_batch: the paths' per-split record counts differ")


if __name__ == "__main__":
    main()
