"""Host-side premises of test_gpu_attention_direct.py (no GPU): the data is what the tests say it is, and a kernel that drops or
moves the spiked key is far outside their bounds."""
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
