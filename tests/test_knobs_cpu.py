"""The run-time knobs (SBH_* environment variables): the set the sources read is the set that
INTEGRATION.md's "Run-time knobs" table lists; the HIP library reads its environment only through
the helpers of csrc/sbh_host.h (env_str, env_flag, env_uint); and the switches whose A/B is settled
and folded stay gone from everything a deployment or a test could set them from."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HELPERS = os.path.join("spark-bam_amd", "csrc", "sbh_host.h")
# folded switches (this file is the one place under tests/ that may name them)
REMOVED = ["SBH_SIEVE", "SBH_PIPE_STREAMS", "SBH_CS_SAME_PRIORITY", "SBH_LOAD_ON_SHARD_STREAM",
           "SBH_PREFETCH_STAGE", "SBH_XQ"]


def text(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8", errors="replace") as f:
        return f.read()


def files(*patterns):
    out = []
    for p in patterns:
        out += [os.path.relpath(f, ROOT) for f in glob.glob(os.path.join(ROOT, p), recursive=True) if os.path.isfile(f)]
    return sorted(out)


def names_read():
    found = set()
    for f in files("spark-bam_amd/csrc/*.hip", "spark-bam_amd/csrc/*.h"):
        found.update(re.findall(r'\benv_(?:str|flag|uint)\(\s*"(SBH_[A-Z0-9_]+)"', text(f)))
    for f in files("cli/*.cpp"):
        found.update(re.findall(r'\bgetenv\(\s*"(SBH_[A-Z0-9_]+)"', text(f)))
    for f in files("spark-bam_amd/*.py"):
        found.update(re.findall(r'os\.environ(?:\.get\(|\[)\s*"(SBH_[A-Z0-9_]+)"', text(f)))
    return found


def names_documented():
    doc = text("INTEGRATION.md")
    section = doc[doc.index("## Run-time knobs"):]
    nxt = section.find("\n## ", 1)
    section = section if nxt < 0 else section[:nxt]
    found = set()
    for line in section.splitlines():
        cells = line.split("|")
        if len(cells) >= 4 and "SBH_" in cells[1]:  # a table row: the names are in its first cell
            found.update(re.findall(r"`(SBH_[A-Z0-9_]+)`", cells[1]))
    return found


def test_table_lists_exactly_the_knobs_the_sources_read():
    read, documented = names_read(), names_documented()
    assert len(read) >= 10 and {"SBH_TOK_BUDGET", "SBH_SCHED", "SBH_LIB_PATH", "SBH_RESIDENT_MAX"} <= read, read
    assert read == documented, "read, not listed: %s; listed, not read: %s" % (
        sorted(read - documented), sorted(documented - read))


def test_library_reads_the_environment_only_through_the_helpers():
    for f in files("spark-bam_amd/csrc/*"):
        src = text(f)
        n = len(re.findall(r"\bgetenv\b", src))
        if f == HELPERS:
            # one call, inside env_str, which the other two helpers go through
            body = src[src.index("inline const char *env_str("):src.index("inline bool env_flag(")]
            assert n == 1 and len(re.findall(r"\bgetenv\b", body)) == 1, n
        else:
            assert n == 0, "%s calls getenv itself" % f


def test_folded_switches_are_named_nowhere():
    me = os.path.relpath(os.path.abspath(__file__), ROOT)
    hits = []
    for f in files(*[d + "/**/*" for d in ("spark-bam_amd", "cli", "jni", "tools", "tests")]):
        parts = f.split(os.sep)
        if f == me or "__pycache__" in parts or "golden" in parts or "build" in parts:
            continue
        if f.endswith((".so", ".o", ".a", ".pyc")) or os.path.getsize(os.path.join(ROOT, f)) > 1 << 20:
            continue  # (build products: no source file is that large)
        src = text(f)
        hits += [(f, name) for name in REMOVED if re.search(r"\b%s\b" % name, src)]
    assert not hits, hits
