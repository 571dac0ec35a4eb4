"""Host-side premises of test_gpu_attention_direct.py and test_gpu_attention_direct_forms.py (no GPU): the data is what the tests
say it is, and a kernel that drops or moves the spiked key is far outside their bounds."""
import hashlib
import json
import os

import pytest
import torch

import attention_direct_cases as adc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind", adc.KINDS)
@pytest.mark.parametrize("width,heads", adc.SHAPES)
def test_data_premises_in_float64(width, heads, kind):
    batch = 3
    qkv = adc.make_qkv(width, heads, batch, kind)
    assert qkv.dtype == torch.float32 and tuple(qkv.shape) == (batch * adc.L, 3 * width)
    fig = adc.check_premises(qkv, batch, heads, kind)
    print("ATTDIRECT premises width=%d kind=%s %s" % (width, kind, fig))
    if kind.startswith("spike"):
        # the mutants are at least four orders of magnitude above every asserted bound
        bounds = json.load(open(os.path.join(ROOT, "profiles", "attention_direct_parent.json")))["max_err"]
        assert min(fig["mutant_drop"], fig["mutant_move"]) >= 1e4 * 2.0 * max(bounds.values()), (fig, bounds)


def test_recorded_parent_errors_are_the_asserted_ones():
    """PARENT_MAX_ERR of the GPU test is the record in profiles/attention_direct_parent.json, digit for digit"""
    import ast
    src = open(os.path.join(ROOT, "tests", "test_gpu_attention_direct.py")).read()
    tree = ast.parse(src)
    val = [n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], "id", "") == "PARENT_MAX_ERR"]
    asserted = ast.literal_eval(val[0])
    rec = json.load(open(os.path.join(ROOT, "profiles", "attention_direct_parent.json")))["max_err"]
    assert asserted == rec and sorted(rec) == sorted(adc.KINDS) and all(0.0 < v < 1e-4 for v in rec.values()), (asserted, rec)


def test_reference_is_the_plain_formula():
    """attention_f64 against a loop over one slab written out by hand"""
    qkv = adc.make_qkv(128, 2, 1, "spike128")
    want = adc.attention_f64(qkv, 1, 2)
    x = qkv.double().view(adc.L, 3, 2, 64)
    for h in range(2):
        q, k, v = x[:, 0, h], x[:, 1, h], x[:, 2, h]
        p = torch.exp(q @ k.t() / 8.0)
        o = (p / p.sum(1, keepdim=True)) @ v
        assert torch.allclose(o, want[0, :, h], rtol=1e-12, atol=1e-12)


# ---- the data of the L = 129 cases does not move: PARENT_MAX_ERR of test_gpu_attention_direct.py was measured on it ---------------
# sha256 of make_qkv(128, 2, 3, kind) as the module stood when it knew one token count only
L129_DIGESTS = {
    "plain": "bf32b4f121781bb9b89baf99d46b0b93981e0b70294052c07f3ac995a397c361",
    "spike128": "a6eb86ad513319b4d753c049be8f7a77ee31d2bd4d521f23afc346a28bc2dcb6",
    "spike127": "63c2bb396081030e68289eb24c2a42ebf3bb5f73012d9f87a8eab1bc12efa87e",
    "spike112": "6c62c1d892f311a177aadebb5ec1ca7aaf97b5d04e13a119cad70c4f785d0701",
    "spike0": "6195067b7dcf66f1620b6f0a4efba0c41c4cc6e7eb4c37f52d80ee12987628ce",
    "magnitude": "4df57970bdb6be2222269092da866c5cd92a44e6d8dae602d217f917dc8fe21e",
}


@pytest.mark.parametrize("kind", adc.KINDS)
def test_the_129_token_data_is_pinned(kind):
    want = L129_DIGESTS[kind]
    assert hashlib.sha256(adc.make_qkv(128, 2, 3, kind).numpy().tobytes()).hexdigest() == want
    assert hashlib.sha256(adc.make_qkv(128, 2, 3, kind, 129).numpy().tobytes()).hexdigest() == want   # the same recipe at any L
    assert set(adc.kinds(129)) == set(adc.KINDS) - {"spike112"} and adc.spike_a(129) == adc.SPIKE_A


def test_spike_keys_are_named_relative_to_the_token_count():
    assert adc.spike_keys(3) == [] and adc.kinds(2) == ["plain", "magnitude"]
    assert adc.spike_keys(17) == [("last", 16), ("0", 0)] and adc.spike_keys(32) == [("last", 31), ("0", 0)]
    assert adc.spike_keys(33) == [("last", 32), ("last-1", 31), ("0", 0)]                      # tile = 32 = last
    assert adc.spike_keys(129) == [("last", 128), ("last-1", 127), ("0", 0)]                   # tile = 128 = last
    assert adc.spike_keys(130) == [("last", 129), ("last-1", 128), ("0", 0)] and adc.spike_keys(160)[2] == ("tile", 144)
    assert adc.spike_keys(257) == [("last", 256), ("last-1", 255), ("0", 0), ("64", 64)]       # tile = block = 256 = last
    assert adc.spike_keys(258) == [("last", 257), ("last-1", 256), ("0", 0), ("64", 64)]       # tile = block = 256 = last-1
    assert adc.spike_keys(442) == [("last", 441), ("last-1", 440), ("tile", 432), ("0", 0), ("block", 384), ("64", 64)]
    assert adc.spike_keys(1025) == [("last", 1024), ("last-1", 1023), ("0", 0), ("64", 64)]
    assert adc.q_tiles_of(129, "plain") == [0, 1, 2, 8, 9, 12] and adc.q_tiles_of(129, "spike0") == [0, 1]
    assert adc.q_tiles_of(2, "plain") == [0, 1, 4] and adc.q_tiles_of(33, "spike32") == [0, 1, 2, 3, 6]
    assert adc.q_tiles_of(257, "spike256") == [0, 1, 2, 8, 9, 16, 17, 20] and adc.q_tiles_of(17, "plain") == [0, 1, 2, 5]
    assert [adc.written_rows(129, n) for n in (0, 1, 2, 8, 9, 12)] == [129, 16, 32, 128, 129, 129]


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["fp32", "fp16"])
@pytest.mark.parametrize("tokens,width,heads,kind", adc.premise_cases())
def test_forms_data_premises_in_float64(tokens, width, heads, kind, dtype):
    """every (token count, shape, kind) of test_gpu_attention_direct_forms.py, in both operand types: the thresholds of
    attention_direct_cases.check_premises, and mutants at least 25 times every bound that module asserts"""
    batch = 3
    qkv = adc.make_qkv(width, heads, batch, kind, tokens, dtype)
    assert qkv.dtype == dtype and tuple(qkv.shape) == (batch * tokens, 3 * width)
    if dtype == torch.float16:
        assert torch.equal(qkv, adc.make_qkv(width, heads, batch, kind, tokens).half())
    fig = adc.check_premises(qkv, batch, heads, kind)
    print("ATTFORMS premises L=%d width=%d kind=%s %s %s" % (tokens, width, kind, dtype, fig))
    if kind.startswith("spike"):
        assert min(fig["mutant_drop"], fig["mutant_move"]) >= 25.0 * max(adc.BOUND_F16, adc.BOUND_SPLIT, adc.BOUND_F32), fig
        if tokens > 256 and kind == "spike%d" % (tokens - 1):
            assert fig["rescale_rows"] >= 0.5


def test_bounds_of_the_forms_module():
    assert adc.BOUND_F16 == 4 * 2.0 ** -11 and adc.BOUND_SPLIT == 2e-5 and adc.BOUND_F32 == 2e-5
    import text_cases
    assert adc.BOUND_SPLIT == text_cases.BOUND_SPLIT
    assert adc.MUTANT_FLOOR >= 25.0 * adc.BOUND_F16
