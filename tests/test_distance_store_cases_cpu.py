"""The premise of tests/test_gpu_distance_stores.py, re-asserted on the host for every case of its matrix: on the integer
features of tests/distance_store_cases.py all three distance modes compute in exact arithmetic, so the expectation
float32(|q|^2 + |g|^2 - 2 q.g) is a matter of equality, not of tolerance.  Whoever edits the shapes or the family and
breaks that learns it here, without a GPU."""
import numpy as np
import pytest

import distance_store_cases as S

EXACT_F32 = 1 << 24      # every integer of smaller magnitude is a float32 (and a sum of such below it is exact)


def _operand_sets():
    return sorted({(c.operands, c.nq, c.ng, c.d) for c in S.CASES})


def test_matrix_covers_the_store_paths():
    """the geometries the kernels branch on, for every operand kind and both K depths"""
    for operands in S.OPERANDS:
        for d in S.D_VALUES:
            cs = [c for c in S.CASES if c.operands == operands and c.d == d]
            vec = [c for c in cs if c.ldo % 4 == 0 and c.col_offset % 4 == 0]
            assert {c.ng % 4 for c in vec} == {0, 1, 2, 3}                       # full and partial 4-packs of 1, 2, 3
            assert any(c.ldo % 4 == 0 and c.col_offset % 4 for c in cs)          # aligned ldo, misaligned pointer
            assert any(c.ldo % 4 and c.col_offset == 0 and c.ldo == c.ng for c in cs)
            assert any(c.ldo % 4 and c.ldo > c.ng for c in cs)
            for c in cs:
                assert c.col_offset + c.ng <= c.ldo
                assert c.nq == (S.NQ if operands == "two" else c.ng)
                # 256-tiles: an interior one, a ragged last one; 128-column tiles: one wholly past n_valid
                assert 2 * 256 < c.ng < 3 * 256 - 128 and 256 < c.nq < 3 * 256
    assert {c.d for c in S.CASES} == {40, 200} and len(S.CASES) == len(S.OPERANDS) * len(S.GEOMETRIES) * 2
    assert len({S.case_id(c) for c in S.CASES}) == len(S.CASES)


def test_family_is_what_it_says():
    x = S.int_features(603, 200, seed=1)
    assert x.dtype == np.int64 and np.abs(x).max() <= 66 and not x[7].any()
    assert len({r.tobytes() for r in x}) == 603                                  # no two rows alike
    row = np.arange(603)
    body = x[:, 1:]
    assert all((body[row % 5 == e] % (1 << e) == 0).all() for e in range(5))


@pytest.mark.parametrize("operands,nq,ng,d", _operand_sets())
def test_every_mode_is_exact_on_the_integer_family(operands, nq, ng, d):
    q, g, want = S.operands_of(operands, nq, ng, d)
    assert (g is q) == (operands != "two") and want.shape == (nq, ng)
    for x in (q, g):
        # operands: fp16 values, so the FAST cast and the fp32 upload lose nothing
        assert np.array_equal(x.astype(np.float16).astype(np.int64), x)
        assert np.isfinite(x.astype(np.float16)).all()
    qn, gn = (q * q).sum(1), (g * g).sum(1)
    absdot = np.abs(q).astype(np.float64) @ np.abs(g).astype(np.float64).T        # bounds every partial sum of q.g, any order
    assert qn.max() < EXACT_F32 and gn.max() < EXACT_F32
    assert absdot.max() < EXACT_F32
    assert (qn[:, None] + gn[None, :]).max() < EXACT_F32                          # the epilogue's an + bn
    assert want.min() >= 0 and want.max() < EXACT_F32                             # fmaf(-2, dot, an + bn): one rounding, of an integer
    assert np.array_equal(want.astype(np.float32).astype(np.int64), want)
    assert np.array_equal(want, qn[:, None] + gn[None, :] - 2 * (q @ g.T))            # (integer product: no float anywhere)
    if operands != "two":
        assert np.array_equal(want, want.T) and not np.diag(want).any()
    # the 3-term split: x * 2^(10 - ex) = hi exactly, lo == 0, nothing near fp16's subnormals or its overflow; rows of one
    # tile carry different exponents, so rscale[m] * cscale[n] matters
    for x in (q, g):
        v, hi, lo, sc = S.split3_pack(x)
        assert np.array_equal(hi.astype(np.float32), v) and not lo.any()
        assert np.abs(v).max() < 2.0 ** 10
        assert np.abs(v[v != 0]).min() >= 2.0 ** -14
        assert len(set(sc[:128].tolist())) >= 3 and (sc[1:] != sc[:-1]).mean() > 0.5
        assert not v[7].any()


def test_cosine_features_are_what_the_bounds_assume():
    q, g = S.cosine_features()
    assert q.shape == (S.COS_NQ, S.COS_D) and g.shape == (S.COS_NG, S.COS_D) and q.dtype == g.dtype == np.float32
    c = S.cosine_f64(q, g)
    zero = np.zeros(c.shape, bool)
    zero[:, S.COS_ZERO_G] = True
    assert np.array_equal(np.isnan(c), zero)
    assert abs(c[S.COS_PLANT_Q, S.COS_PLANT_POS] - 1.0) < 1e-7 and abs(c[S.COS_PLANT_Q, S.COS_PLANT_NEG] + 1.0) < 1e-7
    off = ~zero
    off[S.COS_PLANT_Q, [S.COS_PLANT_POS, S.COS_PLANT_NEG]] = False
    assert np.abs(c[off]).max() < 0.5
    assert np.abs(g).max() < 16 and np.abs(q).max() < 16                          # far inside fp16's range
