"""The host-side sizing functions of the re-ranking answer exactly what they answered before rerank.hip was split and its
four workspace layouts were put on one cursor, one clamp_k and one CandBuffers block: tests/golden/rerank_layout.json was
recorded from a build of the parent commit's sources (tests/golden/make_goldens_rerank_layout.py says how, and which
branch of which layout each shape takes).  Workspace offsets may move; totals, limits and chunk counts may not.  No device."""
import json
import os

import pytest

from mpreid import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
FUNCTIONS = ("mpreid_rerank_workspace_bytes_ex", "mpreid_rerank_fits", "mpreid_rr_sparse_workspace_bytes", "mpreid_rr_vcap",
             "mpreid_rr_jaccard_hist_bytes", "mpreid_rr_csc_chunks")


@pytest.fixture(scope="module")
def rows():
    """(function, arguments, recorded answer); a table line holds the answers along ONE argument (`axis`)"""
    with open(os.path.join(HERE, "golden", "rerank_layout.json")) as fh:
        lines = json.load(fh)["lines"]
    return [(fn, args[:axis] + [v] + args[axis + 1:], want)
            for fn, args, axis, values, answers in lines for v, want in zip(values, answers)]


def test_table_covers_every_function_and_branch(rows):
    by_fn = {fn: [a for f, a, _ in rows if f == fn] for fn in FUNCTIONS}
    assert sum(len(v) for v in by_fn.values()) == len(rows)
    for fn in ("mpreid_rerank_workspace_bytes_ex", "mpreid_rerank_fits"):
        a = by_fn[fn]   # (nq, ng, d, k1, k2, has_local, algo)
        assert {r[6] for r in a} >= set(range(5)) and {r[5] for r in a} == {0, 1}
        assert {2047, 2048} <= {r[0] + r[1] for r in a}                                  # the sparse threshold
        assert any(r[0] + r[1] < r[3] + 1 and r[0] + r[1] < r[4] for r in a)            # N below k1 + 1 and below k2
        assert any(r[4] == 1 for r in a)
        assert {64, 65, 256, 257} <= {max(r[3] + 1, r[4]) for r in a}                    # KR at both limits
        assert {24576, 24577} <= {r[1] for r in a}                                       # one Jaccard chunk / the wave form
    assert {1, 255, 256, 257} <= {r[2] for r in by_fn["mpreid_rr_sparse_workspace_bytes"]}
    assert {24576, 24577} <= {r[0] - r[1] for r in by_fn["mpreid_rr_csc_chunks"]}
    assert by_fn["mpreid_rr_vcap"] and by_fn["mpreid_rr_jaccard_hist_bytes"]


def test_sizing_functions_answer_as_before_the_split(rows):
    assert not os.environ.get("MPREID_TUNE"), "MPREID_TUNE changes three of the layouts"
    L = _lib.load()
    bad = [(fn, args, want, got) for fn, args, want in rows for got in [int(getattr(L, fn)(*args))] if got != want]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(rows), bad[:5])
