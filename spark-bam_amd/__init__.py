"""spark-bam on MI355X: host-side mirror of spark-bam's BGZF + record-boundary API over
the C-ABI in include/sparkbam.h (libsparkbam_hip.so, hand-written gfx950 kernels).

Import name: ``spark_bam_amd`` (the directory name contains a hyphen, so load it with
``__graft_entry__.load_package()`` or importlib).  Names follow the reference:

  bgzf:   Pos, Header.make, Metadata, FindBlockStart, Stream (blocks / inflated bytes)
  check:  eager.Checker / full.Checker (batched over positions; per-position windowed
          WindowedEagerChecker / WindowedFullChecker), FindRecordStart
  load:   load_splits_and_reads / load_bam_count / load_reads / load_bam_intervals
          (CanLoadBam), FileSplits, read_bai (bam.index.Index)
  index:  build_bai / write_bai (the `.bai` samtools index writes, built on the GPU)
  text:   view (the records as SAM text, rendered on the GPU), sam_text_host
  subset: view_bam (filtered records as a BAM with its index, gathered on the GPU), bam_gather_host
  sort:   sort_bam (the records sorted on the GPU, by coordinate or by read name), bam_sort_host,
          bam_name_sort_host
  depth:  depth (per-base coverage accumulated and scanned on the GPU), depth_host
  pileup: pileup (per-base allele counts, call bytes and consensus on the GPU), pileup_host
  counts: flagstat, idxstats (flag and per-reference read counts, one pass on the GPU), tally_host
  stats:  stats (the read-level histograms of samtools stats, counted on the GPU), stats_host
  reads:  fastq (the records as FASTQ / FASTA text, rendered on the GPU), fastq_host
"""
from ._lib import (BLOCK_EMPTY, BLOCK_TRUNCATED, FULL_FLAGS_MASK, FULL_N_SHIFT,  # noqa: F401
                   FULL_SUCCESS, FULL_UNKNOWN, HeaderParseException, HeaderSearchFailedException,
                   NoReadFoundException, SparkBamError, lib)
from .device import Context, Depth, Pileup, PinnedBuffer, Shard, Stats, Tally  # noqa: F401
from .api import (FLAG_NAMES, htsjdk_rewrite, Header, Metadata, Pos, Split, bam_header, check_bam, depth,  # noqa: F401
                  pileup,
                  file_splits, flagstat, full_check, idxstats, load_bam_count, load_reads, load_splits_and_reads,
                  parse_bam_header, sort_bam, view, view_bam)
from .tally import TallyResult, flagstat_text, idxstats_text, tally_host  # noqa: F401
from .stats import SN_ROWS, StatsResult, stats_host, stats_text  # noqa: F401
from .api import stats  # noqa: F401,E402  (after the submodule of the same name: the function is what the package exports)
from .fastq import FastqResult, fastq_host, fastq_mode  # noqa: F401
from .api import fastq  # noqa: F401,E402  (after the submodule of the same name: the function is what the package exports)
from .records import Reads, bam_gather_host, bam_header_set_so, bam_name_sort_host, bam_sort_host, sam_text_host  # noqa: F401
from .coverage import DepthResult, depth_bedgraph, depth_host, depth_text  # noqa: F401
from .pileup import PileupResult, consensus_fasta, pileup_host, pileup_text  # noqa: F401
from .api import pileup  # noqa: F401,E402  (after the submodule of the same name: the function is what the package exports)
from .checkers import GpuWindow, WindowedEagerChecker, WindowedFullChecker  # noqa: F401
from .intervals import (Chunk, Index, get_interval_chunks, load_bam_intervals,  # noqa: F401
                        parse_loci, read_bai)
from .bai import build_bai, write_bai  # noqa: F401

__all__ = [
    "htsjdk_rewrite",
    "Context", "PinnedBuffer", "Shard", "SparkBamError", "HeaderParseException", "HeaderSearchFailedException",
    "NoReadFoundException", "Pos", "Header", "Metadata", "Split", "FLAG_NAMES",
    "file_splits", "load_splits_and_reads", "load_bam_count", "check_bam", "full_check",
    "bam_header", "parse_bam_header", "lib", "load_reads", "Reads", "Chunk", "Index",
    "read_bai", "parse_loci", "get_interval_chunks", "load_bam_intervals",
    "GpuWindow", "WindowedEagerChecker", "WindowedFullChecker",
    "build_bai", "write_bai", "view", "sam_text_host", "view_bam", "bam_gather_host",
    "sort_bam", "bam_sort_host", "bam_name_sort_host", "bam_header_set_so",
    "depth", "Depth", "DepthResult", "depth_host", "depth_text", "depth_bedgraph",
    "pileup", "Pileup", "PileupResult", "pileup_host", "pileup_text", "consensus_fasta",
    "flagstat", "idxstats", "Tally", "TallyResult", "tally_host", "flagstat_text", "idxstats_text",
    "fastq", "fastq_host", "fastq_mode", "FastqResult",
    "stats", "Stats", "StatsResult", "stats_host", "stats_text", "SN_ROWS",
]
