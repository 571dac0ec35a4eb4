"""Host-side checks of the text tower: the float64 restatement against the reference's golden vectors, the premises of the
attention data (wrong masks are far from the right one), the workspace query, and the host logic of the Uni-Prompt model's
text branch.  No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import text_cases as tc
from mpreid import _lib, ops, synth


@pytest.mark.parametrize("name", ["reduced", "full"])
def test_float64_restatement_agrees_with_the_reference(name):
    """tower_f64 is a sound reference for a 2e-5 bound: within 2e-6 (relative L2) of the reference's own fp32 encode_text"""
    cfg, sd, prompts, eot, ref, f64 = tc.golden_case(name)
    assert list(eot) == list(tc.GOLDEN_CASES[name][2]) and ref.shape == (len(eot), cfg["out_dim"])
    assert np.array_equal(prompts, tc.make_prompts(cfg, len(eot), tc.GOLDEN_CASES[name][1] + 1000))   # regenerated, not trusted
    fig = tc.rel_l2(f64, ref)
    print(name, "rel L2 of the float64 restatement against the golden:", fig)
    assert fig <= 2e-6


@pytest.mark.parametrize("tokens", tc.ATT_TOKENS)
def test_attention_data_tells_wrong_masks_apart(tokens):
    """every wrong mask changes the float64 result by >= MUTANT_FLOOR (slab-relative) wherever it differs from the causal one
    at this length: an error of that kind cannot hide under the 2e-5 bound of the GPU test"""
    width, heads = tc.ATT_SHAPES[0]
    qkv, want, scale = tc.attention_case(width, heads, tokens)
    sc = (lambda q, k, v: q @ k.transpose(2, 3) / 8.0)(*tc.split_heads(qkv, tc.ATT_BATCH, heads))
    if tokens >= 16:
        assert 1.7 <= float(sc.std()) <= 2.3
    right = tc.causal_mask(tokens)
    assert bool(right[0, 0]) and not bool(right[0, 1]) and bool(right[1, 0]) and int(right.sum()) == tokens * (tokens + 1) // 2
    tried = 0
    for name, fn in tc.WRONG_MASKS.items():
        wrong = fn(tokens)
        if bool((wrong == right).all()):
            continue
        tried += 1
        fig = tc.error_figure(tc.attention_f64(qkv, tc.ATT_BATCH, heads, wrong), want, scale)
        print(tokens, name, fig)
        assert fig >= tc.MUTANT_FLOOR, (tokens, name, fig)
    assert tried >= 3, tried


def test_workspace_query_needs_no_device_and_grows_with_the_batch():
    L = _lib.load()
    cfg = _lib.TextCfg(**synth.CLIP_TEXT)
    one, many = L.mpreid_text_workspace_bytes(ctypes.byref(cfg), 1), L.mpreid_text_workspace_bytes(ctypes.byref(cfg), 512)
    # the residual stream, q | k | v and the pair operands of 77 * batch rows at least
    assert one >= 77 * 512 * (4 + 12 + 4 + 16) and many > one and many >= 512 * 77 * 512 * (4 + 12 + 4 + 16)
    assert L.mpreid_text_workspace_bytes(ctypes.byref(cfg), 513) > many
    assert L.mpreid_text_workspace_bytes(None, 4) == 0 and L.mpreid_text_workspace_bytes(ctypes.byref(cfg), 0) == 0


def test_text_forward_checks_its_arguments_before_any_launch():
    """no device here: every refusal below happens before the first HIP call"""
    L = _lib.load()
    dummy = ctypes.c_void_p(0x1000)
    layers = (_lib.VitLayer * 2)()
    w = _lib.TextWeights(pos_emb=0x1000, ln_final_g=0x1000, ln_final_b=0x1000, proj=0x1000,
                         layers=ctypes.cast(layers, ctypes.POINTER(_lib.VitLayer)))

    def run(cfg, prompts=dummy, eot=dummy, batch=2, out=dummy, ws=None, ws_bytes=0, weights=w):
        return L.mpreid_text_forward(ctypes.byref(cfg), None if weights is None else ctypes.byref(weights), prompts, eot, batch, out,
                                     ws, ws_bytes, None)
    good = _lib.TextCfg(21, 128, 2, 2, 64)
    assert run(good) == _lib.ERR_WORKSPACE and "workspace too small" in L.mpreid_last_error().decode()
    assert run(good, ws=dummy, ws_bytes=1024) == _lib.ERR_WORKSPACE
    for what, cfg in {"tokens over the limit": _lib.TextCfg(_lib.TEXT_MAX_TOKENS + 1, 128, 2, 2, 64), "one token": _lib.TextCfg(1, 128, 2, 2, 64),
                      "head dim 32": _lib.TextCfg(21, 128, 2, 4, 64), "width 64": _lib.TextCfg(21, 64, 2, 1, 64),
                      "width 1152": _lib.TextCfg(21, 1152, 2, 18, 64)}.items():
        assert run(cfg) == _lib.ERR_UNSUPPORTED, what
        assert L.mpreid_last_error().decode(), what
    assert run(good, prompts=None) == _lib.ERR_ARG and run(good, eot=None) == _lib.ERR_ARG and run(good, out=None) == _lib.ERR_ARG
    assert run(good, batch=0) == _lib.ERR_ARG and run(good, weights=None) == _lib.ERR_ARG
    assert run(good, prompts=ctypes.c_void_p(0x1004)) == _lib.ERR_ARG
    # the unit entry point of the kernel
    att = L.mpreid_text_attention
    assert att(None, 1, 17, 128, 2, dummy, None) == _lib.ERR_ARG and att(dummy, 0, 17, 128, 2, dummy, None) == _lib.ERR_ARG
    assert att(ctypes.c_void_p(0x1008), 1, 17, 128, 2, dummy, None) == _lib.ERR_ARG
    assert att(dummy, 1, _lib.TEXT_MAX_TOKENS + 1, 128, 2, dummy, None) == _lib.ERR_UNSUPPORTED
    assert att(dummy, 1, 1, 128, 2, dummy, None) == _lib.ERR_UNSUPPORTED and att(dummy, 1, 17, 128, 4, dummy, None) == _lib.ERR_UNSUPPORTED
    assert _lib.TEXT_MAX_TOKENS == 128


def test_eot_validation():
    assert ops.check_eot([0, 5, 20], 3, 21).dtype == np.int32
    assert ops.check_eot(torch.tensor([20, 0]), 2, 21).tolist() == [20, 0]
    for bad in ([0, 21], [-1, 3], [0.0, 1.0], [True, False], [1], [[0, 1]]):
        with pytest.raises(ValueError):
            ops.check_eot(bad, 2, 21)


def test_text_state_dict_layout_and_scales():
    cfg = tc.REDUCED
    sd = synth.text_state_dict(cfg, seed=31, vocab=50)
    w = cfg["width"]
    assert sd["positional_embedding"].shape == (cfg["tokens"], w) and sd["text_projection"].shape == (w, cfg["out_dim"])
    assert sd["token_embedding.weight"].shape == (50, w) and "token_embedding.weight" not in synth.text_state_dict(cfg, seed=31)
    assert all(v.dtype == np.float32 for v in sd.values())
    std = {k: float(sd[k].std()) for k in ("transformer.resblocks.0.attn.in_proj_weight", "transformer.resblocks.1.mlp.c_fc.weight",
                                           "transformer.resblocks.1.mlp.c_proj.weight", "positional_embedding")}
    want = (w ** -0.5, (2 * w) ** -0.5, w ** -0.5 * (2 * cfg["layers"]) ** -0.5, 0.01)
    for got, exp in zip(std.values(), want):
        assert 0.9 * exp <= got <= 1.1 * exp, (std, want)
    again = synth.text_state_dict(cfg, seed=31, vocab=50)
    assert all(np.array_equal(sd[k], again[k]) for k in sd)


# ---- host logic of the Uni-Prompt model's text branch ------------------------------------------------------------
def _learner(num_class=7, seed=3, stage="1a"):
    from model import make_model_uniprompt as mu
    t = tc.prompt_learner_tensors(num_class, seed)
    pl = mu.PromptLearner()
    pl.set_tensors(t)
    pl.set_training_stage(stage)
    return pl, t


def test_prompt_assembly_matches_the_restatement():
    label = torch.tensor([3, 0, 6, 6, 1])
    pl, t = _learner()
    assert pl.training_stage == "1a"
    got = pl(label)
    assert got.shape == (5, 77, 512) and torch.equal(got, tc.assemble_prompts(t, label, "1a"))
    assert float(got[:, 9:17].abs().max()) == 0.0 and torch.equal(got[:, 1:9], t["ctx_generic"][label])
    assert torch.equal(pl(label, view=torch.tensor([0, 6, 11, 12, 13])), got)      # stage 1a ignores the view
    pl.set_training_stage("1b")
    view = torch.tensor([0, 6, 11, 12, 13])
    got = pl(label, view=view)
    assert torch.equal(got, tc.assemble_prompts(t, label, "1b", view))
    # view 0: rgb / cctv, 6 and 11: ir / cctv, 12: rgb / uav, 13: ir / uav
    for row, (modal, plat) in enumerate([(0, 0), (1, 0), (1, 0), (0, 1), (1, 1)]):
        assert torch.equal(got[row, 9:13], t["ctx_modality"][modal]) and torch.equal(got[row, 13:17], t["ctx_platform"][plat])
    got = pl(label)
    assert torch.equal(got, tc.assemble_prompts(t, label, "1b", None))
    assert torch.equal(got[2, 9:13], t["ctx_modality"].mean(dim=0)) and torch.equal(got[0, 17:], t["token_suffix"][0])
    with pytest.raises(ValueError):
        pl(torch.tensor([7]))


def _text_checkpoint(num_class, seed=5):
    from model import make_model_uniprompt as mu
    sd = synth.text_state_dict(mu.TEXT_CFG, seed=seed)
    ck = {"module.text_encoder." + k: torch.from_numpy(v) for k, v in sd.items()}
    ck.update({"module.prompt_learner." + k: v for k, v in tc.prompt_learner_tensors(num_class, seed + 1).items()})
    ck["module.prompt_learner.visual_enhanced_net.linear1.weight"] = torch.zeros(32, 512)
    ck["module.image_fusion_net.fc1.weight"] = torch.zeros(256, 1024)
    return ck


def test_text_checkpoint_complete_incomplete_and_wrongly_shaped():
    from model import make_model_uniprompt as mu
    ck = _text_checkpoint(7)
    text, prompt, used = mu.split_text_checkpoint(ck, 7)
    assert set(text) == set(mu.text_shapes()) and set(prompt) == set(mu.PROMPT_KEYS)
    assert len(used) == len(text) + len(prompt) and not any("visual_enhanced_net" in k or "image_fusion_net" in k for k in used)
    with pytest.raises(ValueError):
        mu.split_text_checkpoint(ck, 8)                     # ctx_generic of another label space
    for drop in ("module.text_encoder.ln_final.bias", "module.prompt_learner.token_suffix",
                 "module.text_encoder.transformer.resblocks.11.mlp.c_proj.weight"):
        assert mu.split_text_checkpoint({k: v for k, v in ck.items() if k != drop}, 7) is None, drop
    for key, shape in (("module.text_encoder.positional_embedding", (76, 512)), ("module.prompt_learner.ctx_platform", (2, 4, 256)),
                       ("module.prompt_learner.ctx_generic", (7, 4, 512)), ("module.text_encoder.text_projection", (512, 256))):
        assert mu.split_text_checkpoint(dict(ck, **{key: torch.zeros(shape)}), 7) is None, key
    # the checkpoint of tests/test_gpu_pipeline.py::test_uniprompt_model_branches: one text tensor and an unknown prompt key
    assert mu.split_text_checkpoint({"module.prompt_learner.cls_ctx": torch.zeros(7, 4, 512),
                                     "module.text_encoder.ln_final.weight": torch.ones(512)}, 7) is None


def test_model_host_side_of_the_text_branch(tmp_path, capsys):
    """construction keeps the state dict and builds nothing of the text tower; PROMPT_EOT_INDEX and tokenized_prompts give the
    read-out row; load_param takes a complete text checkpoint and skips an incomplete one with the old message and count"""
    from config import cfg_base
    from model import make_model_uniprompt as mu
    cfg = cfg_base.clone()
    cfg.defrost()
    assert cfg.MODEL.PROMPT_EOT_INDEX == 19
    m = mu.make_model(cfg, num_class=7, camera_num=6, view_num=1)
    keys = set(m.state_dict())
    assert not any(k.startswith(("text_encoder.", "prompt_learner.")) for k in keys)
    assert m._text_encoder is None and m.prompt_learner.ctx_generic is None and m.prompt_learner.training_stage == "1a"
    assert m._eot_rows(3).tolist() == [19, 19, 19]
    tok = torch.zeros(1, 77, dtype=torch.long)
    tok[0, 0], tok[0, 23] = 49406, 49407
    m.prompt_learner.tokenized_prompts = tok
    assert m._eot_rows(4).tolist() == [23] * 4
    m.prompt_learner.tokenized_prompts = None
    cfg.merge_from_list(["MODEL.PROMPT_EOT_INDEX", 25])
    assert mu.make_model(cfg, 7, 6, 1)._eot_rows(2).tolist() == [25, 25]
    cfg.merge_from_list(["MODEL.PROMPT_EOT_INDEX", 77])
    with pytest.raises(ValueError):
        mu.make_model(cfg, 7, 6, 1)
    for kw in ("get_text", "get_raw_text", "get_image_update", "get_more_image"):
        with pytest.raises(NotImplementedError):
            m(x=None, **{kw: True})
    # a complete checkpoint
    ck = {"module." + k: v.clone() for k, v in m.state_dict().items()}
    ck.update(_text_checkpoint(7))
    path = tmp_path / "full.pth"
    torch.save(ck, path)
    capsys.readouterr()
    m.load_param(str(path))
    out = capsys.readouterr().out
    assert "(2 text-tower / fusion tensors are not used at evaluation and were skipped)" in out and "text tower:" in out
    assert m._text_source is not None and set(m._text_source[1]) == set(mu.PROMPT_KEYS) and set(m.state_dict()) == keys
    # an incomplete one: every key under the prefixes is skipped, the earlier text tensors stay
    del ck["module.text_encoder.ln_final.bias"]
    n_text = sum(1 for k in ck if k.replace("module.", "").startswith(("text_encoder.", "prompt_learner.", "image_fusion_net.")))
    torch.save(ck, path)
    kept = m._text_source
    m.load_param(str(path))
    out = capsys.readouterr().out
    assert "({} text-tower / fusion tensors are not used at evaluation and were skipped)".format(n_text) in out
    assert "text tower:" not in out and m._text_source is kept
    # another label space
    torch.save(dict(_text_checkpoint(9), **{"module." + k: v for k, v in m.state_dict().items()}), path)
    with pytest.raises(ValueError):
        m.load_param(str(path))


def test_text_encoder_refuses_other_precisions_before_touching_a_device():
    for call in (lambda: ops.TextEncoder(dict(tc.REDUCED, precision="fp16"), {}), lambda: ops.TextEncoder(dict(tc.REDUCED, precision="fp32"), {})):
        with pytest.raises(RuntimeError, match=r"code -3"):
            call()
