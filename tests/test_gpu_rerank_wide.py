"""GPU parity of the WIDE re-ranking algorithm (any k1 / k2), all through the C ABI via mpreid.ops / utils.reranking.

Bar: BIT-EXACT against the oracle (outputs, neighbour table, nnz of V / V_qe), BIT-EXACT against DENSE and SPARSE where
they apply, BIT-EXACT against the reference when both are fed the same distance matrix (tests/golden/rerank_wide.npz),
and the bounds of tests/test_gpu_rerank.py (RR_FRAC / RR_MAX) against the reference as called."""
import threading

import numpy as np
import pytest
import torch

from oracle import oracle as orc
from test_oracle_rerank_wide import wide_case, check_against_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from mpreid import ops as o
    return o


def _check_vs_oracle(ops, f, nq, k1, k2, lam, local=None, only_local=False, want_all=None):
    q, g = torch.from_numpy(f[:nq]), torch.from_numpy(f[nq:])
    got, st, rank, vc, vq = ops.re_ranking(q, g, k1, k2, lam, local_distmat=local, only_local=only_local, debug=True,
                                           algo=ops.RERANK_WIDE)
    assert st["algo"] == ops.RERANK_WIDE
    want, orank, ovc, ovq = want_all if want_all is not None else orc.re_ranking(
        f[:nq], f[nq:], k1, k2, lam, local_distmat=local, only_local=only_local, debug=True)
    assert rank.shape == orank.shape and np.array_equal(rank, orank), "initial_rank differs"
    assert np.array_equal(vc, ovc), "nnz(V) differs"
    assert np.array_equal(vq, ovq), "nnz(V_qe) differs"
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want, equal_nan=True), np.abs(got - want).max()
    assert st["v_nnz"] == int(ovc.sum()) and st["vqe_nnz"] == int(ovq.sum())
    return got


# ---- 1. WIDE == oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,d,k1,k2", [(1500, 300, 64, 300, 40), (1200, 200, 64, 299, 15), (1200, 200, 64, 50, 257),
                                           (2000, 300, 256, 126, 10), (700, 100, 1280, 30, 40), (64, 10, 32, 100, 80),
                                           (900, 1, 128, 400, 1)])
def test_wide_seeded_bit_exact(ops, n, nq, d, k1, k2):
    from mpreid import synth
    f, _ = synth.clustered_features(n, d, 2.5, seed=n + k1, per_id=30)
    _check_vs_oracle(ops, f, nq, k1, k2, 0.3)


@pytest.mark.parametrize("lam", [0.3, 0.0, 1.0])
def test_wide_lambda_values(ops, lam):
    from mpreid import synth
    f, _ = synth.clustered_features(1200, 64, 2.5, seed=1499, per_id=30)
    _check_vs_oracle(ops, f, 200, 299, 15, lam)


def test_wide_local_distmat(ops):
    from mpreid import synth
    n, nq = 1000, 150
    f, _ = synth.clustered_features(n, 64, 2.5, seed=61, per_id=25)
    rng = np.random.default_rng(5)
    local = (rng.random((n, n), dtype=np.float32) * 0.5 + 0.25).astype(np.float32)   # not symmetric
    _check_vs_oracle(ops, f, nq, 280, 30, 0.3, local=local)
    _check_vs_oracle(ops, f, nq, 280, 30, 0.3, local=local, only_local=True)


# ---- 2. WIDE == DENSE == SPARSE; exact ties --------------------------------------------------------------------------
@pytest.mark.parametrize("n,nq,d,k1,k2,sigma", [(3000, 600, 768, 50, 15, 3.0), (2500, 1, 128, 20, 6, 2.0)])
def test_wide_equals_dense_equals_sparse(ops, n, nq, d, k1, k2, sigma):
    from mpreid import synth
    f, _ = synth.clustered_features(n, d, sigma, seed=n + k1, per_id=20)
    ft = torch.from_numpy(f).cuda()
    outs = {}
    for algo in (ops.RERANK_WIDE, ops.RERANK_DENSE, ops.RERANK_SPARSE):
        out, st, rank, vc, vq = ops.re_ranking(ft[:nq], ft[nq:], k1, k2, 0.3, debug=True, algo=algo)
        assert st["algo"] == algo
        outs[algo] = (out.cpu().numpy(), rank, vc, vq, st["v_nnz"], st["vqe_nnz"])
    w = outs[ops.RERANK_WIDE]
    for algo in (ops.RERANK_DENSE, ops.RERANK_SPARSE):
        o = outs[algo]
        assert np.array_equal(w[0], o[0]) and np.array_equal(w[1], o[1]) and np.array_equal(w[2], o[2])
        assert np.array_equal(w[3], o[3]) and w[4:] == o[4:]
    assert np.array_equal(w[0], orc.re_ranking(f[:nq], f[nq:], k1, k2, 0.3))


def test_wide_with_exact_ties(ops):
    """the inputs of test_gpu_rerank.py::test_rerank_with_exact_ties: duplicated rows (tied distances: the (value, index)
    tie-break) and all rows identical (0 / 0 = NaN everywhere, the neighbour table is pure index order)"""
    from mpreid import synth
    f, _ = synth.clustered_features(600, 64, 2.0, seed=77, per_id=10)
    f[100:160] = f[40:100]       # 60 exact duplicates
    f[300:310] = f[0]            # 10 copies of one row
    _check_vs_oracle(ops, f, 120, 20, 6, 0.3)
    _check_vs_oracle(ops, f, 120, 50, 15, 0.3)
    _check_vs_oracle(ops, f, 120, 300, 15, 0.3)
    same = np.tile(f[:1], (80, 1))
    _check_vs_oracle(ops, same, 16, 10, 3, 0.3)


# ---- 3. against the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", range(4))
def test_wide_vs_reference_golden(ops, golden, row):
    g = golden("rerank_wide.npz")
    tag, feat, pid, nq, k1, k2, lam = wide_case(g, g["cases"][row])
    got = _check_vs_oracle(ops, feat, nq, k1, k2, lam)
    ft = torch.from_numpy(feat).cuda()
    d_dev = ops.euclidean_distance(ft, ft)   # the device's exact distance matrix IS the oracle's
    got2, st = ops.re_ranking(ft[:nq], ft[nq:], k1, k2, lam, local_distmat=d_dev, only_local=True, algo=ops.RERANK_WIDE)
    assert st["algo"] == ops.RERANK_WIDE
    check_against_reference(g, tag, pid, nq, got, got2.cpu().numpy())


# ---- 4. the drop-in layer takes any k --------------------------------------------------------------------------------
def test_dropin_takes_any_k(ops):
    from mpreid import synth
    from utils.reranking import re_ranking, re_ranking_device
    f, _ = synth.clustered_features(1200, 64, 2.5, seed=3)   # the inputs of test_rerank_limits_fail_loudly_and_name_the_limit
    q, g = torch.from_numpy(f[:200]), torch.from_numpy(f[200:])
    for k1, k2 in ((299, 15), (50, 257)):
        want = orc.re_ranking(f[:200], f[200:], k1, k2, 0.3)
        out = re_ranking(q, g, k1, k2, 0.3)
        assert isinstance(out, np.ndarray) and out.dtype == np.float32 and np.array_equal(out, want)
        assert np.array_equal(re_ranking(f[:200], f[200:], k1, k2, 0.3), want)          # numpy inputs
        assert np.array_equal(re_ranking(q.cuda(), g.cuda(), k1, k2, 0.3), want)        # device tensors
        _, st = re_ranking_device(q, g, k1, k2, 0.3)
        assert st["algo"] == ops.RERANK_WIDE
    # what ran before takes the path it took
    _, st = re_ranking_device(q, g, 50, 15, 0.3)
    assert st["algo"] in (ops.RERANK_DENSE, ops.RERANK_SPARSE)
    out, st = re_ranking_device(q, g, 255, 15, 0.3)
    assert st["algo"] == ops.RERANK_DENSE and np.array_equal(out.cpu().numpy(), orc.re_ranking(f[:200], f[200:], 255, 15, 0.3))
    # an explicitly passed algorithm is honoured as given, refusal included
    with pytest.raises(RuntimeError, match=r"exceeds this build's limit of 256"):
        re_ranking_device(q, g, 299, 15, 0.3, algo=ops.RERANK_AUTO)


def test_dropin_k1_255_at_20000(ops):
    """N = 20 000, k1 = 255: the LDS refusal of DENSE; the drop-in call returns, and a 1/8 row sub-sample computed on its
    own equals the oracle bit for bit (the pattern of test_rerank_market_shape_d1280)"""
    from mpreid import synth
    from utils.reranking import re_ranking, re_ranking_device
    N, nq = 20000, 100
    f, _ = synth.clustered_features(N, 32, 2.5, seed=4)
    ft = torch.from_numpy(f).cuda()
    assert not ops.rerank_fits(nq, N - nq, 32, 255, 15) and ops.rerank_fits(nq, N - nq, 32, 255, 15, algo=ops.RERANK_WIDE)
    out, st = re_ranking_device(ft[:nq], ft[nq:], 255, 15, 0.3)
    assert st["algo"] == ops.RERANK_WIDE and out.shape == (nq, N - nq) and bool(torch.isfinite(out).all())
    ops.release_workspaces("rerank")
    sub = np.arange(0, N, 8)
    fs = f[sub]
    nqs = int((sub < nq).sum())
    got, st = re_ranking_device(ft[sub[:nqs]], ft[sub[nqs:]], 255, 15, 0.3, algo=ops.RERANK_WIDE)
    assert np.array_equal(got.cpu().numpy(), orc.re_ranking(fs[:nqs], fs[nqs:], 255, 15, 0.3))


# ---- 5. the predicate ------------------------------------------------------------------------------------------------
def test_rerank_fits_predicate(ops):
    from mpreid import synth
    # (nq, ng, d, k1, k2, AUTO accepts?) -- the calls of test_rerank_limits_fail_loudly_and_name_the_limit
    calls = [(200, 1000, 64, 299, 15, False), (200, 1000, 64, 50, 257, False), (200, 1000, 64, 255, 15, True),
             (100, 19900, 32, 255, 15, False), (100, 19900, 32, 50, 15, True)]
    for nq, ng, d, k1, k2, ok in calls:
        assert ops.rerank_fits(nq, ng, d, k1, k2) is ok, (nq, ng, k1, k2)
        assert ops.rerank_fits(nq, ng, d, k1, k2, algo=ops.RERANK_WIDE), (nq, ng, k1, k2)
    assert not ops.rerank_fits(200, 1000, 64, 299, 15, algo=ops.RERANK_DENSE)
    assert not ops.rerank_fits(200, 1000, 64, 50, 15, algo=ops.RERANK_SPARSE)       # N < 2048
    assert ops.rerank_fits(600, 2400, 64, 50, 15, algo=ops.RERANK_SPARSE)
    assert not ops.rerank_fits(600, 2400, 64, 50, 15, has_local=True, algo=ops.RERANK_SPARSE)
    assert not ops.rerank_fits(200, 1000, 64, 50, 0, algo=ops.RERANK_WIDE)          # invalid k2
    # ops keeps its contract: the default algorithm still refuses, with the pinned text
    f, _ = synth.clustered_features(1200, 64, 2.5, seed=3)
    q, g = torch.from_numpy(f[:200]).cuda(), torch.from_numpy(f[200:]).cuda()
    with pytest.raises(RuntimeError, match=r"max\(k1 \+ 1, k2\) = 300 exceeds this build's limit of 256.*k1 = 50, k2 = 15"):
        ops.re_ranking(q, g, 299, 15, 0.3)


# ---- 6. workspace ----------------------------------------------------------------------------------------------------
def test_wide_reads_no_workspace_byte_it_did_not_write(ops):
    from mpreid import synth
    f, _ = synth.clustered_features(1300, 64, 2.5, seed=8, per_id=30)
    ft = torch.from_numpy(f).cuda()
    q, g = ft[:250], ft[250:]
    ops.release_workspaces("wide_poison")
    ref, _ = ops.re_ranking(q, g, 280, 20, 0.3, algo=ops.RERANK_WIDE, ws_tag="wide_poison")
    ref = ref.clone()
    for pat in (0xFF, 0x7B, 0x00):   # NaN halves / floats, large finite values, zeros
        bufs = [b for k, b in ops._ws_cache.items() if k[1] == "wide_poison"]
        assert len(bufs) == 1
        bufs[0].fill_(pat)
        got, _ = ops.re_ranking(q, g, 280, 20, 0.3, algo=ops.RERANK_WIDE, ws_tag="wide_poison")
        assert torch.equal(ref, got), hex(pat)
    ops.release_workspaces("wide_poison")


def test_wide_two_streams_two_workspaces(ops):
    from mpreid import synth
    cases = [(1400, 250, 64, 290, 20), (1100, 150, 128, 60, 270)]
    feats = [torch.from_numpy(synth.clustered_features(n, d, 2.5, seed=177 + n, per_id=30)[0]).cuda() for n, _, d, _, _ in cases]
    want = [ops.re_ranking(ft[:c[1]], ft[c[1]:], c[3], c[4], 0.3, algo=ops.RERANK_WIDE)[0].clone() for ft, c in zip(feats, cases)]
    torch.cuda.synchronize()
    errors = []

    def run(i):
        try:
            st = torch.cuda.Stream()
            n, nq, d, k1, k2 = cases[i]
            with torch.cuda.stream(st):
                for rep in range(3):
                    out, _ = ops.re_ranking(feats[i][:nq], feats[i][nq:], k1, k2, 0.3, algo=ops.RERANK_WIDE, ws_tag=f"wide{i}")
                    st.synchronize()
                    if not torch.equal(out, want[i]):
                        errors.append((i, rep))
        except Exception as e:   # noqa: BLE001
            errors.append((i, repr(e)))
    ths = [threading.Thread(target=run, args=(i,)) for i in range(len(cases))]
    [t.start() for t in ths]
    [t.join() for t in ths]
    ops.release_workspaces("wide0")
    ops.release_workspaces("wide1")
    assert not errors, errors


# ---- the forms a tuning key selects (read once per process: child process) -------------------------------------------
_FORM_WORKER = """
import os, sys
import numpy as np, torch
sys.path[:0] = [{root!r}, os.path.join({root!r}, "mp-reid_amd")]
from mpreid import ops, synth
res = {{}}
for n, nq, d, k1, k2 in {cases!r}:
    f, _ = synth.clustered_features(n, d, 2.5, seed=77 + n, per_id=30)
    ft = torch.from_numpy(f).cuda()
    out, st = ops.re_ranking(ft[:nq], ft[nq:], k1, k2, 0.3, algo=ops.RERANK_WIDE)
    assert st["algo"] == ops.RERANK_WIDE
    res[f"{{n}}_{{k1}}"] = out.cpu().numpy()
np.savez(sys.argv[1], **res)
"""


def test_wide_scratch_sort_and_chunked_jaccard_forms(tmp_path):
    """neighbour sorts larger than wide_sort_lds entries run in workspace scratch, galleries larger than
    wide_jaccard_rows rows are accumulated chunk by chunk: both forms forced at sizes the oracle can check"""
    import os
    import subprocess
    import sys
    from mpreid import synth
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    cases = [(1300, 200, 64, 300, 20), (1100, 100, 64, 40, 10)]
    script = tmp_path / "w.py"
    script.write_text(_FORM_WORKER.format(root=root, cases=cases))
    out = tmp_path / "out.npz"
    r = subprocess.run([sys.executable, str(script), str(out)],
                       env=dict(os.environ, MPREID_TUNE="wide_sort_lds=32,wide_jaccard_rows=256"), capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(out)
    for n, nq, d, k1, k2 in cases:
        f, _ = synth.clustered_features(n, d, 2.5, seed=77 + n, per_id=30)
        assert np.array_equal(got[f"{n}_{k1}"], orc.re_ranking(f[:nq], f[nq:], k1, k2, 0.3)), (n, k1)
