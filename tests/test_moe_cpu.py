"""Host-side checks of the MoE image encoder: the float64 restatement against the reference's golden vectors, the routing
margin of every stored case, a wrong variant against the golden, and the host logic of mpreid.ops / mpreid.synth / the
drop-in model (moe_layers resolution, error cases, unused later gates, the untouched dense path).  No GPU needed."""
import numpy as np
import pytest
import torch

import moe_cases as mc
from mpreid import ops, synth


@pytest.mark.parametrize("name", list(mc.CASES))
def test_float64_restatement_agrees_with_the_golden(name):
    """relative L2 <= 2e-5 on the features; the top-k selection of the float64 logits equals that of the reference's logits on
    every token (compared as sets per token: the order inside the k is not part of the decision)"""
    g = mc.golden_case(name)
    rel = mc.rel_l2(g["f64"]["feat"], g["ref"])
    print("float64 restatement vs the reference, %s: %.3e" % (name, rel))
    assert rel <= mc.BOUND_SPLIT
    K = g["cfg"]["top_k"]
    ref_sel = mc.topk_lower_first(torch.from_numpy(g["ref_logits"]).double(), K)
    assert g["f64"]["logits"].shape == g["ref_logits"].shape
    assert torch.equal(ref_sel.sort(-1).values, g["f64"]["sel"].sort(-1).values)


@pytest.mark.parametrize("name", list(mc.CASES))
def test_routing_margin_of_the_fixture(name):
    """on every token the K-th / (K+1)-th float64 logit gap is at least 1000 x the reference's own fp32 logit error; no token is
    excluded"""
    g = mc.golden_case(name)
    gap, err = mc.margin_figures(g["f64"]["logits"], g["ref_logits"], g["cfg"]["top_k"])
    print("%s: gap %.3e, fp32 logit error %.3e, ratio %.0f" % (name, gap, err, gap / err))
    assert err > 0 and gap >= mc.MARGIN_RATIO * err
    stored = np.load(mc.GOLDEN)[name + "_margin"]
    assert np.allclose(stored, [gap, err], rtol=1e-9)


def test_wrong_variants_miss_the_goldens():
    """re-gating in every MoE block misses `reduced`'s golden by more than MUTANT_FLOOR; so does every other wrong variant on at
    least one reduced case (the figures written beside MUTANT_FLOOR in moe_cases.py are the ones printed here)"""
    figs = {}
    for variant in mc.WRONG_VARIANTS:
        for name in ("reduced", "reduced_all", "reduced_wide"):
            g = mc.golden_case(name)
            figs[variant, name] = mc.rel_l2(mc.tower_f64(g["cfg"], g["sd"], g["imgs"], variant=variant)["feat"], g["ref"])
    for k, v in figs.items():
        print("%-13s %-13s %.3e" % (k + (v,)))
    assert figs["regate", "reduced"] > mc.MUTANT_FLOOR
    for variant in mc.WRONG_VARIANTS:
        assert max(v for (vr, _), v in figs.items() if vr == variant) > mc.MUTANT_FLOOR, variant
    # a variant that changes nothing for a case (re-gating with one MoE block, bias placement with w == 1) gives the golden again
    assert figs["regate", "reduced_wide"] <= mc.BOUND_SPLIT and figs["bias_outside", "reduced_all"] <= mc.BOUND_SPLIT


def test_moe_layers_resolve_as_in_the_reference():
    base = dict(layers=12, num_experts=4, top_k=2)
    assert ops.resolve_moe(dict(base, moe_layers=-1)) == (4, 2, 12)
    assert ops.resolve_moe(dict(base, moe_layers=20)) == (4, 2, 12)
    assert ops.resolve_moe(dict(base, moe_layers=3)) == (4, 2, 3)
    assert ops.resolve_moe(dict(base, moe_layers=0)) == (0, 0, 0)            # use_moe with no MoE block: the dense tower
    assert ops.resolve_moe(dict(layers=12)) == (0, 0, 0)
    assert ops.resolve_moe(dict(layers=12, num_experts=4, top_k=0, moe_layers=-1)) == (0, 0, 0)   # use_moe is False
    assert ops.resolve_moe(dict(layers=12, num_experts=0, top_k=2, moe_layers=-1)) == (0, 0, 0)
    with pytest.raises(ValueError, match="top_k 5 > num_experts 4"):
        ops.resolve_moe(dict(base, top_k=5, moe_layers=2))
    with pytest.raises(NotImplementedError):
        ops.resolve_moe(dict(base, num_experts=65, moe_layers=2))
    with pytest.raises(NotImplementedError):
        ops.resolve_moe(dict(layers=12, num_experts=16, top_k=9, moe_layers=2))


def test_request_errors_are_raised_on_the_host():
    """top_k > num_experts, missing expert keys, a missing gate and a precision other than split: clear errors before any device
    is asked for; the unused gates of later blocks may be present or absent"""
    cfg = dict(mc.CASES["reduced"][0])
    sd = synth.vit_moe_state_dict(cfg, seed=3)
    assert ops.check_moe_request(cfg, sd, "split") == (4, 2, 2)
    assert ops.check_moe_request(cfg, {"image_encoder." + k: v for k, v in sd.items()}, "split") == (4, 2, 2)
    assert "transformer.resblocks.1.gate.weight" in sd and "transformer.resblocks.2.gate.weight" not in sd
    without_late_gate = {k: v for k, v in sd.items() if k != "transformer.resblocks.1.gate.weight"}
    assert ops.check_moe_request(cfg, without_late_gate, "split") == (4, 2, 2)
    for prec in ("fp16", "fp32"):
        with pytest.raises(NotImplementedError, match="split"):
            ops.VitEncoder(cfg, sd, (64, 32), precision=prec)
    with pytest.raises(ValueError, match="top_k"):
        ops.VitEncoder(dict(cfg, top_k=5), sd, (64, 32))
    lacking = {k: v for k, v in sd.items() if k != "transformer.resblocks.1.experts.3.c_proj.bias"}
    with pytest.raises(ValueError, match=r"resblocks\.1\.experts\.3\.c_proj\.bias"):
        ops.VitEncoder(cfg, lacking, (64, 32))
    with pytest.raises(ValueError, match=r"resblocks\.0\.gate\.weight"):
        ops.VitEncoder(cfg, {k: v for k, v in sd.items() if k != "transformer.resblocks.0.gate.weight"}, (64, 32))
    with pytest.raises(ValueError):   # a dense checkpoint is not an MoE checkpoint
        ops.VitEncoder(cfg, synth.vit_state_dict(cfg, seed=3), (64, 32))


def test_synth_moe_state_dict_layout():
    cfg = dict(mc.CASES["reduced"][0])
    sd = synth.vit_moe_state_dict(cfg, seed=3, std=0.05, ln_jitter=0.1)
    dense = synth.vit_state_dict(cfg, seed=3, std=0.05, ln_jitter=0.1)
    w = cfg["width"]
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}."
        if i < 2:
            assert b + "mlp.c_fc.weight" not in sd and sd[b + "gate.weight"].shape == (4, w)
            assert sd[b + "experts.3.c_fc.weight"].shape == (4 * w, w) and sd[b + "experts.0.c_proj.bias"].shape == (w,)
        else:
            assert b + "gate.weight" not in sd and np.array_equal(sd[b + "mlp.c_proj.weight"], dense[b + "mlp.c_proj.weight"])
    assert all(np.array_equal(sd[k], dense[k]) for k in sd if k in dense)       # the dense keys keep their bytes
    assert float(np.std(sd["transformer.resblocks.0.gate.weight"])) > 0.2       # a gate that separates the experts
    allb = synth.vit_moe_state_dict(dict(cfg, moe_layers=-1), seed=3)
    assert "transformer.resblocks.2.gate.weight" in allb and not any(".mlp." in k for k in allb)
    assert all(v.dtype == np.float32 for v in sd.values())


def test_dropin_config_and_model_host_logic():
    """MODEL.MOE defaults are the reference's keys; RN50 with MoE raises; make_model with MoE creates the reference's key names"""
    from config import cfg, cfg_base
    for c in (cfg, cfg_base):
        assert dict(c.MODEL.MOE) == {"ENABLED": False, "NUM_EXPERTS": 0, "TOP_K": 0, "MOE_LAYERS": 0, "DROPOUT": 0.0}
    from model.make_model import make_model
    c = cfg_base.clone()
    c.defrost()
    c.merge_from_list(["MODEL.NAME", "RN50", "MODEL.MOE.ENABLED", True, "MODEL.MOE.NUM_EXPERTS", 2, "MODEL.MOE.TOP_K", 1,
                       "MODEL.MOE.MOE_LAYERS", 1])
    with pytest.raises(NotImplementedError, match="RN50"):
        make_model(c, num_class=3, camera_num=2, view_num=1)


def test_the_dense_request_is_untouched():
    """What the host can see of the dense path: with num_experts = 0, without the MoE keys, or with moe_layers = 0, the request
    resolves to no MoE block, for any precision and with no expert key in the state dict, so VitEncoder takes the branch it took
    before.  That the packed weights and the features are then the same needs a device: tests/test_gpu_moe.py
    (test_single_expert_equals_the_dense_tower) compares a cfg with the MoE keys at 0 against one without them bit for bit."""
    cfg = dict(mc.CASES["reduced"][0], num_experts=0, top_k=0, moe_layers=0)
    sd = synth.vit_state_dict(cfg, seed=3)
    assert ops.check_moe_request(cfg, sd, "fp16") == (0, 0, 0)
    assert ops.check_moe_request({k: v for k, v in cfg.items() if k not in ("num_experts", "top_k", "moe_layers")}, sd, "fp32") == (0, 0, 0)
    assert ops.check_moe_request(dict(cfg, num_experts=4, top_k=2, moe_layers=0), sd, "fp16") == (0, 0, 0)
