#!/usr/bin/env python3
"""Generate tests/golden/rerank_layout.json: what the host-side sizing functions of the re-ranking answer, recorded from a
build of the sources as they were BEFORE rerank.hip was split and its layouts were put on one cursor / one clamp_k / one
CandBuffers block.  tests/test_rerank_layout_cpu.py compares the current library with it, exactly.  No device needed.

Build the commit to record from (a checkout of it, e.g. from `git worktree add DIR <commit>`) beside the product library and
point MPREID_LIB at it:

    MPREID_CSRC=DIR/mp-reid_amd/csrc MPREID_BUILD_TAG=parent python mp-reid_amd/mpreid/build.py
    MPREID_LIB=tools/ablation_lib/libmpreid_hip_parent.so python tests/golden/make_goldens_rerank_layout.py

(The table in the tree was recorded from commit 5d8e3c4, the parent of the split.)  MPREID_TUNE must be unset: three of
the layouts read tuning keys.

The shapes are chosen so that every branch of every layout is taken:
  N                10 and 30 (below k1 + 1, k1 / 2 + 1 and k2: the clamps), 300, 2047 / 2048 (the sparse threshold), 5000,
                   19281 (Market-1501), 25576 / 25577 (ng = 24576 / 24577: the Jaccard stage's one chunk / several chunks and
                   wave form, and WIDE's accumulator rows), 100 000, 700 000 (beyond WIDE's LDS masks)
  (k1, k2)         k2 = 1; KR = max(k1 + 1, k2) at 64 / 65 (sparse eligibility) and 256 / 257 (the dense limit) through k1 and
                   through k2; k1 = 190 / 200 (the dense LDS limit at large N); KR above 4096 (WIDE sorts outside LDS)
  d                100 (not a multiple of 64: the fp16 operands are padded); 768 at k = 50 / 15
  has_local, algo  0 / 1, all five
  row blocks       1, 255, 256, 257 rows, half and all of n, for the sharded phase-1 workspace
"""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "mp-reid_amd"))

SHAPES = [(4, 6), (10, 20), (100, 200), (500, 1547), (500, 1548), (1000, 4000), (3368, 15913), (1000, 24576), (1000, 24577),
          (20000, 80000), (100000, 600000)]
KS = [(50, 15), (20, 6), (50, 1), (63, 1), (64, 1), (10, 64), (10, 65), (255, 15), (256, 15), (20, 256), (20, 257), (190, 15),
      (200, 15), (5000, 15), (20, 5000)]

ALL_K_SHAPES = [(10, 20), (3368, 15913), (20000, 80000)]


def cases():
    """(function, argument list, index of the argument that runs, its values): one table line each"""
    for (nq, ng), (k1, k2), d, has_local in itertools.product(SHAPES, KS, (100, 768), (0, 1)):
        if d == 768 and (k1, k2) != KS[0]:
            continue   # d only scales the feature buffers: one k setting at the second width
        if (nq, ng) not in ALL_K_SHAPES and (k1, k2) not in KS[:3]:
            continue   # every k setting at three sizes, the first three (k2 = 1 among them) at every size
        yield "mpreid_rerank_workspace_bytes_ex", [nq, ng, d, k1, k2, has_local, 0], 6, list(range(5))
        if d == 100:   # (d is no argument of the limits)
            yield "mpreid_rerank_fits", [nq, ng, d, k1, k2, has_local, 0], 6, list(range(5))
    for args in ((0, 10, 64, 20, 6, 0, 1), (10, 0, 64, 20, 6, 0, 1), (10, 20, 0, 20, 6, 0, 1), (10, 20, 64, -1, 6, 0, 1),
                 (10, 20, 64, 20, 0, 0, 1)):   # refused arguments; and an algorithm that does not exist
        for fn in ("mpreid_rerank_workspace_bytes_ex", "mpreid_rerank_fits"):
            yield fn, list(args), 6, [1]
    for fn in ("mpreid_rerank_workspace_bytes_ex", "mpreid_rerank_fits"):
        yield fn, [10, 20, 64, 20, 6, 0, 5], 6, [5]
    for n, d, kr in itertools.product((2048, 19281, 100000), (100, 768), (16, 64)):
        yield "mpreid_rr_sparse_workspace_bytes", [n, d, 1, kr], 2, [1, 255, 256, 257, n // 2, n]
    yield "mpreid_rr_sparse_workspace_bytes", [0, 64, 1, 16], 2, [1]
    yield "mpreid_rr_sparse_workspace_bytes", [2048, 64, 0, 16], 2, [0]
    for n in (10, 30, 300, 2048, 19281):
        yield "mpreid_rr_vcap", [n, 0], 1, [0, 1, 20, 50, 255, 300]
    yield "mpreid_rr_jaccard_hist_bytes", [1], 0, [1, 1023, 1024, 1025, 2048, 19281, 100000]
    for nq, ns in ((0, (10, 24576, 24577)), (1, (2,)), (100, (300,)), (3368, (19281,)), (1000, (25576, 25577)), (20000, (100000,)),
                   (100000, (700000,)), (5, (5,))):   # (5, 5): no indexed row, refused
        yield "mpreid_rr_csc_chunks", [ns[0], nq], 0, list(ns)


def main():
    assert not os.environ.get("MPREID_TUNE"), "MPREID_TUNE changes three of the layouts"
    from mpreid import _lib
    L = _lib.load()
    lines = []
    for fn, args, axis, values in cases():
        answers = [int(getattr(L, fn)(*(args[:axis] + [v] + args[axis + 1:]))) for v in values]
        lines.append([fn, args, axis, values, answers])
    out = os.path.join(HERE, "rerank_layout.json")
    with open(out, "w") as fh:
        fh.write('{"lines": [\n' + ",\n".join(json.dumps(r, separators=(",", ":")) for r in lines) + "\n]}\n")
    print("%s: %d lines, %d answers from %s" % (out, len(lines), sum(len(r[4]) for r in lines), _lib.LIB_PATH))


if __name__ == "__main__":
    main()
