"""Every Scala/Java file:line citation in the repo points inside the cited reference file.

The reference's files are known by their recorded line counts (tests/golden/reference_lines.tsv,
written by tools/check_citations.py --index), so the check needs no reference checkout."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_citations_in_range():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_citations
    idx = check_citations.ref_index()
    assert "Z3SFC.scala" in idx and "XZ2SFC.scala" in idx and len(idx) > 1000
    bad = check_citations.check(ROOT)
    assert not bad, "\n".join("%s:%d: %s (%s)" % b for b in bad)
