#!/usr/bin/env python3
"""Generate tests/golden/eval_func_samecam.npz: the REFERENCE's eval_func with its same-camera filter switched back on.

Run in the build container only (needs /root/reference), like make_goldens.py:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_goldens_samecam.py

The reference's utils/metrics.py promises the Market-1501 protocol in eval_func's docstring (:29-31) and carries the line
that implements it commented out (:54, followed by `remove = False`).  This script reads that file's source, restores
the line IN MEMORY by string markers (un-comment `# remove = (`, drop `remove = False`), executes the result and runs
eval_func on a seeded, tie-free input.  Nothing of the reference is copied into this repository: the fixture holds the
input (d, q_pid, g_pid, q_cam, g_cam) and the reference's output (cmc, mAP).
"""
import contextlib
import io
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.dont_write_bytecode = True


def load_eval_funcs():
    """(eval_func with line 54 restored, eval_func as shipped) from the reference's source text"""
    src = open(os.path.join(REF, "utils", "metrics.py")).read()
    start = src.index("def eval_func(")
    end = src.index("\nclass ", start)
    body = src[start:end]
    on, off = "# remove = (", "remove = False"
    assert body.count(on) == 1 and body.count(off) == 1, "the reference's eval_func is not the one this script knows"
    lines = []
    for line in body.split("\n"):
        if line.strip() == off:
            continue
        lines.append(line.replace(on, on[2:]))
    out = []
    for text in ("\n".join(lines), body):
        mod = types.ModuleType("ref_eval_func")
        mod.np = np
        exec(compile(text, "<reference eval_func>", "exec"), mod.__dict__)
        out.append(mod.eval_func)
    return out


def make_input():
    nq, ng, ids, cams = 48, 384, 16, 4
    rng = np.random.default_rng(11)
    d = np.stack([rng.permutation(ng) for _ in range(nq)]).astype(np.float32) / np.float32(ng)   # tie-free rows
    q_pid = rng.integers(0, ids, nq).astype(np.int64)
    g_pid = rng.integers(0, ids, ng).astype(np.int64)
    q_cam = rng.integers(0, cams, nq).astype(np.int64)
    g_cam = rng.integers(0, cams, ng).astype(np.int64)
    q_pid[0] = 10_000                       # query 0: no match at all
    q_pid[1] = 5_000                        # query 1: an identity of its own whose 5 gallery items sit on ITS camera
    own = rng.choice(ng, 5, replace=False)
    g_pid[own] = 5_000
    g_cam[own] = q_cam[1]
    return d, q_pid, g_pid, q_cam, g_cam


def main():
    filtered, shipped = load_eval_funcs()
    d, q_pid, g_pid, q_cam, g_cam = make_input()
    nq, ng = d.shape
    # preconditions
    assert all(np.unique(row).size == ng for row in d), "rows must be tie-free (np.argsort is unstable)"
    order = np.argsort(d, axis=1)
    match = g_pid[order] == q_pid[:, None]
    junk = match & (g_cam[order] == q_cam[:, None])
    has = match.any(axis=1)
    first_is_junk = int(sum(junk[q, match[q].argmax()] for q in range(nq) if has[q]))
    assert first_is_junk >= 1, "no query whose nearest pid match is junk"
    valid_unf = int(has.sum())
    valid_fil = int((match & ~junk).any(axis=1).sum())
    assert valid_fil == valid_unf - 1, (valid_fil, valid_unf)
    with contextlib.redirect_stdout(io.StringIO()):
        cmc, mAP = filtered(d, q_pid, g_pid, q_cam, g_cam)
        cmc_u, mAP_u = shipped(d, q_pid, g_pid, q_cam, g_cam)
    assert cmc.dtype == np.float32 and not np.array_equal(cmc, cmc_u)
    path = os.path.join(HERE, "eval_func_samecam.npz")
    np.savez_compressed(path, d=d, q_pid=q_pid, g_pid=g_pid, q_cam=q_cam, g_cam=g_cam, cmc=cmc, mAP=np.float64(mAP))
    print(f"eval_func_samecam.npz: {os.path.getsize(path) / 1024:.0f} KiB; valid queries {valid_fil} of {valid_unf}, "
          f"first match junk for {first_is_junk} queries, |dmAP| vs unfiltered {abs(mAP - mAP_u):.3e}")


if __name__ == "__main__":
    main()
