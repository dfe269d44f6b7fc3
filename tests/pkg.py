"""Test helper: import the product package (spark-bam_amd/) as spark_bam_amd; set a run-time knob
where no monkeypatch fixture is at hand."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from __graft_entry__ import load_package  # noqa: E402

sb = load_package()


@contextlib.contextmanager
def knob(name, value):
    """The environment variable `name` set to `value` inside the block and put back after it (the
    library reads its knobs again at every call)."""
    old = os.environ.get(name)
    os.environ[name] = str(value)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = old
