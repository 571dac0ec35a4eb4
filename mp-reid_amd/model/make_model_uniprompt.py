"""Drop-in for the reference's ``model/make_model_uniprompt.py`` — evaluation branches only.

The Uni-Prompt ``build_transformer`` computes its evaluation feature exactly like the base model (reference
model/make_model_uniprompt.py:209-238: image encoder with the SIE embedding, CLS of the last block and of its
projection, eval BatchNorm, concat per ``TEST.NECK_FEAT``), so the HIP encoder of ``model/make_model.py`` serves it.
Kept from the reference signature (:159): ``forward(x=None, label=None, get_image=False, get_text=False,
cam_label=None, view_label=None, ..., get_image_vp=False)``:

  default                      -> Tensor[B, 1280]           (:203-238, what do_inference / the TTA evaluation call)
  get_image=True               -> projected CLS [B, 512]    (:172-177)
  get_image_vp                 -> projected CLS + visual_prompt (:178-186)
  label=..., get_text=True     -> text features of the identity prompts, Tensor[b, 512] (:160-170; get_raw_text is
                                  the same branch there and returns the same thing here)

The text branch: ``prompt_learner`` assembles ``token_prefix | ctx_generic[label] | modality ctx | platform ctx |
token_suffix`` (PromptLearner.forward, :334-377; torch indexing on the device) and the CLIP text transformer
(mpreid.ops.TextEncoder: causal attention, ln_final on the end-of-text row, text_projection -- :49-68) encodes it.  The
end-of-text row is ``prompt_learner.tokenized_prompts.argmax(-1)`` when a caller sets that tensor (the reference's
source; it is in no checkpoint) and ``MODEL.PROMPT_EOT_INDEX`` otherwise (config/node.py).  The text-tower tensors are
NOT registered parameters (``state_dict()`` keeps the evaluation model's keys, construction costs what it did): they
live in a holder that is built at the first ``get_text`` call -- from the checkpoint when ``load_param`` found a
complete set (``text_encoder.*`` and ``prompt_learner.{ctx_generic, ctx_modality, ctx_platform, token_prefix,
token_suffix}``), else from the seeded initialisation (``MODEL.INIT_SEED``), as the image tower does with an empty
``TEST.WEIGHT``.  ``get_text`` / ``get_raw_text`` without ``label``, the MLP feature fusion (``get_image_update``) and the
multi-token variant (``get_more_image``) raise NotImplementedError; so does training mode before
``enable_stage2_training()``.

Stage 2 (reference train_uniprompt.py:137-154, processor/processor_uniprompt_stage2.py:14-175): ``enable_stage2_training()``
marks every parameter as trained except ``text_encoder`` / ``expert`` / ``prompt_learner`` names (none of which is a registered
parameter here), moves the module to the device and builds a training encoder without a neck whose fp32 masters ARE the
module's ``image_encoder.*`` parameters (mpreid.ops.VitEncoder.enable_training(masters)): an optimizer over
``named_parameters()`` updates what the encoder reads, after a re-pack of the split-precision operands.  In training mode
``forward(x=, label=, cam_label=, view_label=)`` then returns the reference's training outputs under autograd (see
``_forward_training``); ``stage2_trainer(cfg, optimizer, text_features)`` gives the fused step without autograd
(mpreid.ops.Stage2Trainer) over the same parameters.  ``.eval()`` drops the folded evaluation encoders, so the next
evaluation call rebuilds them from the updated parameters and running statistics.  The dense ViT-B-16 tower in the split
precision only: MODEL.MOE.ENABLED and RN50 keep NotImplementedError (the MoE tower's backward and an RN50 backward do not
exist).

Prompt learning (reference processor/processor_uniprompt_stage1.py:44-100): ``enable_stage1a_training()`` /
``enable_stage1b_training()`` (:138-157) mark ``ctx_generic``, or ``ctx_modality`` and ``ctx_platform``, as leaves that
require grad.  While grad mode is on and the assembled prompts require grad, ``get_text`` runs
``TextEncoder.forward_grad``: the same features, as a node of torch's autograd graph whose backward is the library's
prompt gradient (mpreid_text_backward; the tower's weights stay frozen), and autograd carries it through the prompt
assembly to the context tensors.  The stage-1 loop itself is ``processor/processor_uniprompt_stage1.py::do_train_stage1``
with ``loss/supcontrast.py``, ``solver/make_optimizer_prompt.py`` and ``solver/scheduler_factory.py``; with their Adam / AdamW
optimizer a step is one fused ``mpreid.ops.PromptTrainer.step`` (loss, context gradients and the update in HIP kernels, no
autograd graph), and it writes the context tensors in place, so the next ``get_text`` call sees the new values.
``text_state_dict()`` gives the tower and prompt tensors under the reference's checkpoint keys.  The model stays in
``.eval()`` throughout (neither branch has a mode-dependent layer).  Otherwise -- no stage enabled, or under
``torch.no_grad()`` -- the call is the evaluation call, bit for bit.  ``load_param`` skips the checkpoint keys of modules this build
does not have (``prompt_learner.visual_enhanced_net.*``, ``image_fusion_net.*``, unknown keys under those prefixes), and
an INCOMPLETE set of text-tower tensors as a whole.

``tta_view`` (not in the reference) selects a test-time-augmentation view computed inside the patch gather; the
reference materialises the view tensors instead (processor/processor_uniprompt_stage2.py:605-633) — passing such a
tensor as ``x`` works as well and gives the same bits.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from mpreid import ops as _ops
from mpreid import synth as _synth

from . import make_model as _base

_SKIPPED_PREFIXES = ("prompt_learner.", "text_encoder.", "image_fusion_net.")
TEXT_CFG = dict(_synth.CLIP_TEXT)
#: reference PromptLearner.__init__ (:279-296): 8 generic + 4 modality + 4 platform context tokens of width 512
N_GENERIC_CTX, N_MODAL_CTX, N_PLAT_CTX, CTX_DIM = 8, 4, 4, 512
PROMPT_KEYS = ("ctx_generic", "ctx_modality", "ctx_platform", "token_prefix", "token_suffix")


def prompt_shapes(num_class, tokens=TEXT_CFG["tokens"]):
    n_ctx = N_GENERIC_CTX + N_MODAL_CTX + N_PLAT_CTX
    return {"ctx_generic": (num_class, N_GENERIC_CTX, CTX_DIM), "ctx_modality": (2, N_MODAL_CTX, CTX_DIM),
            "ctx_platform": (2, N_PLAT_CTX, CTX_DIM), "token_prefix": (1, 1, CTX_DIM),
            "token_suffix": (1, tokens - 1 - n_ctx, CTX_DIM)}


def text_shapes(cfg=TEXT_CFG):
    """name -> shape of every text_encoder.* tensor the tower needs (CLIP's own key names)"""
    w = cfg["width"]
    s = {"positional_embedding": (cfg["tokens"], w), "ln_final.weight": (w,), "ln_final.bias": (w,),
         "text_projection": (w, cfg["out_dim"])}
    for i in range(cfg["layers"]):
        b = f"transformer.resblocks.{i}."
        s.update({b + "attn.in_proj_weight": (3 * w, w), b + "attn.in_proj_bias": (3 * w,), b + "attn.out_proj.weight": (w, w),
                  b + "attn.out_proj.bias": (w,), b + "ln_1.weight": (w,), b + "ln_1.bias": (w,), b + "ln_2.weight": (w,),
                  b + "ln_2.bias": (w,), b + "mlp.c_fc.weight": (4 * w, w), b + "mlp.c_fc.bias": (4 * w,),
                  b + "mlp.c_proj.weight": (w, 4 * w), b + "mlp.c_proj.bias": (w,)})
    return s


class PromptLearner:
    """The prompt tensors and PromptLearner.forward (:334-377).  A plain holder, not a module: its tensors stay out of
    the model's state_dict.  ``tokenized_prompts`` is None unless a caller sets it (see the module docstring)."""

    def __init__(self):
        self.training_stage = '1a'
        self.tokenized_prompts = None
        for k in PROMPT_KEYS:
            setattr(self, k, None)

    def set_training_stage(self, stage):
        self.training_stage = stage

    def parameters(self):
        """the three context tensors (what the reference's nn.Module registers as parameters), for torch.optim.*"""
        return iter([self.ctx_generic, self.ctx_modality, self.ctx_platform])

    def set_tensors(self, tensors, device=None):
        for k in PROMPT_KEYS:
            setattr(self, k, tensors[k].detach().to(device=device, dtype=torch.float32).contiguous())

    @staticmethod
    def platform_index(view):
        """0-5 cctv_rgb, 6-11 cctv_ir, 12 uav_rgb, 13 uav_ir: platform 1 iff view >= 12"""
        return (view >= 12).long()

    @staticmethod
    def modality_index(view):
        """modality 1 iff 6 <= view < 12 or view == 13"""
        return (((view >= 6) & (view < 12)) | (view == 13)).long()

    def forward(self, label, view=None, validate=True):
        """validate=False skips the range check of `label` (it reads the labels back from the device): for a caller that has
        checked them already (mpreid.ops.PromptTrainer, whose step must not wait for the device)"""
        dev = self.ctx_generic.device
        label = torch.as_tensor(label).to(dev).long()
        b = label.shape[0]
        if validate and b and (int(label.min()) < 0 or int(label.max()) >= self.ctx_generic.shape[0]):
            raise ValueError(f"label outside 0 .. {self.ctx_generic.shape[0] - 1}")
        generic_ctx = self.ctx_generic[label]
        if self.training_stage == '1a':
            # (the context tensors' own shapes: [.., 4, 512] in the model, narrower in a reduced tower)
            modal_ctx = torch.zeros(b, *self.ctx_modality.shape[1:], device=dev, dtype=generic_ctx.dtype)
            plat_ctx = torch.zeros(b, *self.ctx_platform.shape[1:], device=dev, dtype=generic_ctx.dtype)
        elif view is not None:
            view = torch.as_tensor(view).to(dev).long()
            if view.shape != label.shape:
                raise ValueError(f"view: expected shape {tuple(label.shape)}, got {tuple(view.shape)}")
            plat_ctx = self.ctx_platform[self.platform_index(view)]
            modal_ctx = self.ctx_modality[self.modality_index(view)]
        else:
            modal_ctx = self.ctx_modality.mean(dim=0, keepdim=True).expand(b, -1, -1)
            plat_ctx = self.ctx_platform.mean(dim=0, keepdim=True).expand(b, -1, -1)
        return torch.cat([self.token_prefix.expand(b, -1, -1), generic_ctx, modal_ctx, plat_ctx,
                          self.token_suffix.expand(b, -1, -1)], dim=1)

    __call__ = forward


def seeded_text_tensors(num_class, seed):
    """(text state dict, prompt tensors) of a model without a text checkpoint: synth.text_state_dict and N(0, 0.02) prompt
    tensors (the reference's init of the ctx_* parameters, :287-296; prefix / suffix stand in for token embeddings)"""
    g = torch.Generator().manual_seed(seed + 3)
    prompt = {k: torch.randn(*s, generator=g) * 0.02 for k, s in prompt_shapes(num_class).items()}
    return _synth.text_state_dict(TEXT_CFG, seed=seed + 2), prompt


def split_text_checkpoint(param_dict, num_class):
    """The text-tower part of a Uni-Prompt checkpoint -> (text state dict, prompt tensors, keys used), or None when the
    set is incomplete or a shape does not fit the tower (the caller then skips those keys).  A complete set whose
    ctx_generic is not [num_class, 8, 512] is a checkpoint of another label space: ValueError."""
    text, prompt, used = {}, {}, []
    for name, v in param_dict.items():
        key = name.replace('module.', '')
        if key.startswith("text_encoder."):
            text[key[len("text_encoder."):]] = v
            used.append(name)
        elif key.startswith("prompt_learner.") and key[len("prompt_learner."):] in PROMPT_KEYS:
            prompt[key[len("prompt_learner."):]] = v
            used.append(name)
    want_t, want_p = text_shapes(), prompt_shapes(num_class)
    if any(k not in text or tuple(text[k].shape) != s for k, s in want_t.items()):
        return None
    if any(k not in prompt for k in want_p):
        return None
    if any(tuple(prompt[k].shape) != s for k, s in want_p.items() if k != "ctx_generic"):
        return None
    cg = tuple(prompt["ctx_generic"].shape)
    if cg[1:] != want_p["ctx_generic"][1:]:
        return None
    if cg[0] != num_class:
        raise ValueError(f"prompt_learner.ctx_generic holds {cg[0]} identities, the model was built for {num_class}")
    return {k: text[k] for k in want_t}, prompt, used


LOAD_BALANCE_LOSS_COEFF = 0.01   # processor/processor_uniprompt_stage2.py:76 of the reference


def load_balancing_loss_func(gate_logits, top_k):
    """model/clip/model.py:342-377 restated: gate_logits [rows, E] of ONE layer -> E * sum_e f_e P_e, f_e the share of rows
    whose top-k holds e (not differentiated), P_e the mean softmax probability of e.  The row order does not matter."""
    num_experts = gate_logits.shape[-1]
    gate_logits = gate_logits.reshape(-1, num_experts)
    routing_weights = F.softmax(gate_logits, dim=-1)
    _, selected = torch.topk(routing_weights, top_k, dim=-1)
    tokens_per_expert = F.one_hot(selected, num_experts).float().mean(dim=0)
    return (tokens_per_expert * routing_weights.mean(dim=0)).sum() * num_experts


class build_transformer(_base.build_transformer):
    def __init__(self, num_classes, camera_num, view_num, cfg):
        eot = int(getattr(cfg.MODEL, "PROMPT_EOT_INDEX", 19))
        if not 0 <= eot < TEXT_CFG["tokens"]:
            raise ValueError(f"MODEL.PROMPT_EOT_INDEX {eot} outside 0 .. {TEXT_CFG['tokens'] - 1}")
        super().__init__(num_classes, camera_num, view_num, cfg)
        self.prompt_eot_index = eot
        self.prompt_dim = 512   # hard-coded in the reference (:89), whatever the backbone
        self._init_seed = int(getattr(cfg.MODEL, "INIT_SEED", 7))
        g = torch.Generator().manual_seed(self._init_seed + 1)
        self.visual_prompt = nn.Parameter(torch.randn(1, 1, self.prompt_dim, generator=g) * 0.02, requires_grad=False)
        self._proj_encoder = None
        # the text tower: nothing is generated, copied or packed before the first get_text call
        self.prompt_learner = PromptLearner()
        self._text_source = None    # (text state dict, prompt tensors) of the last checkpoint that carried a complete set
        self._text_encoder = None
        self._text_sd = None        # the state dict self._text_encoder was built from (text_state_dict)
        self._train_encoder = None  # enable_stage2_training() / enable_stage2_moe_training()
        self._moe_training = False  # enable_stage2_moe_training(): the explicit opt-in to train an MoE tower
        self.router_aux_loss = None  # the last training forward's load-balancing loss [1], differentiable (MoE towers)

    def _invalidate(self):
        super()._invalidate()
        self._proj_encoder = None

    def train(self, mode=True):
        super().train(mode)
        if not mode:      # an optimizer may have changed the parameters: the next evaluation call folds them afresh
            self._invalidate()
        return self

    # -- stage 2 ----------------------------------------------------------------------------------
    def _is_moe(self):
        return bool(self.vit_cfg.get("num_experts", 0) or self.vit_cfg.get("moe_layers", 0))

    def _check_stage2_tower(self, moe_ok=False):
        if self.model_name == 'RN50':
            raise NotImplementedError("stage-2 training with MODEL.NAME 'RN50': the RN50 tower has no backward pass (missing: the "
                                      "gradient kernels of the ModifiedResNet); train the ViT-B-16 tower")
        if self._is_moe() and not (moe_ok or self._moe_training):
            raise NotImplementedError("stage-2 training with MODEL.MOE.ENABLED: the MoE tower has no backward pass behind this "
                                      "call (missing: the expert matrices' own gradients -- the experts stay frozen, the gate "
                                      "and the dense parts are trained); opt in with enable_stage2_moe_training()")

    def enable_stage2_moe_training(self, device="cuda", set_requires_grad=True):
        """enable_stage2_training() for an MoE tower, as an explicit opt-in: the reference's 2a marking does real work here --
        every `expert` name is frozen (the gradient flows THROUGH the experts), block 0's gate and the dense parts are trained;
        the gates of later blocks are never read (model/clip/model.py:310-322), so they get no gradient and nothing moves them.
        set_requires_grad=False keeps the caller's marking, which must have frozen the experts already (an expert that requires
        grad is the encoder's NotImplementedError: their own gradients are not implemented).
        Afterwards a training-mode forward returns the 4-tuple (scores, feats, f_proj, router_logits), router_logits
        [L * B, E] in the reference's flat order.  ValueError on a dense tower.  Returns self."""
        if not self._is_moe():
            raise ValueError("enable_stage2_moe_training: the tower has no MoE block (MODEL.MOE.ENABLED is off); "
                             "call enable_stage2_training()")
        self._check_stage2_tower(moe_ok=True)
        self._moe_training = True
        try:
            return self.enable_stage2_training(device, set_requires_grad)
        except Exception:
            self._moe_training = False
            raise

    def enable_stage2_training(self, device="cuda", set_requires_grad=True):
        """Stage 2a of the reference (train_uniprompt.py:137-154): every parameter requires grad except those whose name
        contains text_encoder, expert or prompt_learner; the module moves to the device; the training encoder is built on the
        module's own image_encoder.* parameters (no copies); the folded evaluation encoders are dropped.  Returns self.
        An MoE tower: through enable_stage2_moe_training() only."""
        self._check_stage2_tower()
        print("Enabling Stage 2 Training: image tower, BNNeck, classifiers, SIE table.")
        self.to(device)
        if set_requires_grad:     # (False: the caller has marked the trained parameters itself, e.g. make_optimizer_2bstage)
            for name, p in self.named_parameters():
                p.requires_grad = not ('text_encoder' in name or 'expert' in name or 'prompt_learner' in name)
        self._invalidate()
        enc = self._build_encoder(False, ws_tag="enc_train")
        enc.enable_training({k: p for k, p in self.named_parameters() if k.startswith("image_encoder.")})
        self._train_encoder = enc
        return self

    def _sie_index(self, cam_label, view_label):
        """the row of cv_embed per image (reference :209-216), or None without SIE labels"""
        if cam_label is not None and view_label is not None:
            return cam_label * self.view_num + view_label
        return cam_label if cam_label is not None else view_label

    def stage2_trainer(self, cfg, optimizer, text_features):
        """The fused stage-2 step of this model (mpreid.ops.Stage2Trainer) over the module's own parameters, with `optimizer` a
        mpreid.ops.TensorOptimizer over them (solver/make_optimizer_prompt.py) and the text features of all identities held
        constant.  step(img, target, cv_index) takes cv_index = _sie_index(cam_label, view_label) when SIE is on."""
        if self._train_encoder is None:
            raise RuntimeError("stage2_trainer: call enable_stage2_training() first")
        sie = bool(cfg.MODEL.SIE_CAMERA or cfg.MODEL.SIE_VIEW)
        self._train_encoder.sync_weights_batched()
        return _ops.Stage2Trainer(self._train_encoder, self.stage2_head(cfg), optimizer, text_features,
                                  cv_table=self.cv_embed if sie else None, sie_coe=self.sie_coe, pixel_mean=self.pixel_mean,
                                  pixel_std=self.pixel_std, aux_coef=LOAD_BALANCE_LOSS_COEFF if self._is_moe() else None)

    def _forward_training(self, x, cam_label, view_label):
        """The reference's training outputs (:203-231) under autograd: ([cls_score, cls_score_proj], [f_last, f, f_proj], f_proj).
        The tower is VitEncoder.forward_grad (its backward is the library's gradient sweep, into the module's parameters and
        the SIE table), the two bottlenecks are F.batch_norm in training mode on the module's own buffers, the classifiers
        F.linear.  The split-precision operands are re-packed from the parameters first (one wait for the device), so any
        optimizer may have updated them.  A 3-tuple, which the reference's loop accepts: its fourth output is the all-token
        projection, which the loop takes for router logits and never reads on a dense tower."""
        self._check_stage2_tower()
        enc = self._train_encoder
        if enc is None:
            raise NotImplementedError("training-mode forward: call enable_stage2_training() first (stage 2 of the dense ViT-B-16 "
                                      "tower); there is no other training forward")
        enc.sync_weights_batched()
        if isinstance(x, (list, tuple, _ops.PackedRawImages)):
            x = _ops.resize_bilinear_u8(x, self.img_hw)
        cv = self._sie(cam_label, view_label)
        router_logits = None
        if self._is_moe():
            # Under autograd the logits are DATA (the sweep takes no gradient with respect to them); the load-balancing term
            # reaches the gate through the fifth output: router_aux_loss [1] is load_balancing_loss_func of these logits as a
            # differentiable node, and the gradient that arrives at it is the term's coefficient.
            f_last, f, f_proj, logits, self.router_aux_loss = enc.forward_grad(x, cv, 0, self.pixel_mean, self.pixel_std)
            n_tok = logits.shape[0] // f.shape[0]
            router_logits = logits.view(f.shape[0], n_tok, -1).transpose(0, 1).reshape(logits.shape)   # rows l * B + b
        else:
            f_last, f, f_proj = enc.forward_grad(x, cv, 0, self.pixel_mean, self.pixel_std)
        feats = []
        for bn, t in ((self.bottleneck, f), (self.bottleneck_proj, f_proj)):
            feats.append(F.batch_norm(t, bn.running_mean, bn.running_var, bn.weight, bn.bias, True, 0.1, 1e-5))
            bn.num_batches_tracked.add_(1)
        scores = [F.linear(feats[0], self.classifier.weight), F.linear(feats[1], self.classifier_proj.weight)]
        if router_logits is not None:
            return scores, [f_last, f, f_proj], f_proj, router_logits
        return scores, [f_last, f, f_proj], f_proj

    def text_tower(self):
        """the device text encoder (mpreid.ops.TextEncoder), built on first use together with the prompt tensors"""
        if self._text_encoder is None:
            if self._text_source is None:
                print('text tower: no checkpoint tensors, seeded initialisation (MODEL.INIT_SEED {})'.format(self._init_seed))
                sd, prompt = seeded_text_tensors(self.num_classes, self._init_seed)
            else:
                sd, prompt = self._text_source
            enc = _ops.TextEncoder(TEXT_CFG, sd, ws_tag="text")
            self.prompt_learner.set_tensors(prompt, enc.device)
            self._text_encoder = enc
            self._text_sd = sd
        return self._text_encoder

    def _enable_stage(self, stage, trained):
        self.text_tower()
        pl = self.prompt_learner
        pl.set_training_stage(stage)
        for p in pl.parameters():
            p.requires_grad_(False)
            p.grad = None
        for name in trained:
            getattr(pl, name).requires_grad_(True)

    def enable_stage1a_training(self):
        """Stage 1a (reference :138-146): only the generic context vectors are trained"""
        print("Enabling Stage 1a Training: Generic Context only.")
        self._enable_stage('1a', ("ctx_generic",))

    def enable_stage1b_training(self):
        """Stage 1b (reference :148-157): only the modality and platform context vectors are trained"""
        print("Enabling Stage 1b Training: Domain-Specific Context only.")
        self._enable_stage('1b', ("ctx_modality", "ctx_platform"))

    def text_state_dict(self):
        """the text tower and the prompt tensors (as they stand, tuned or not) under the reference's checkpoint key names,
        on the host: torch.save(model.text_state_dict(), path), then load_param(path)"""
        self.text_tower()

        def host(v):
            return (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v.detach()).float().cpu().clone()
        out = {"text_encoder." + k: host(self._text_sd[k]) for k in text_shapes()}
        for k in PROMPT_KEYS:
            out["prompt_learner." + k] = getattr(self.prompt_learner, k).detach().cpu().clone()
        return out

    def _eot_rows(self, b):
        tok = self.prompt_learner.tokenized_prompts
        if tok is None:
            return np.full(b, self.prompt_eot_index, dtype=np.int64)
        rows = torch.as_tensor(tok).reshape(-1, TEXT_CFG["tokens"]).argmax(dim=-1).cpu().numpy()
        if rows.shape[0] not in (1, b):
            raise ValueError(f"prompt_learner.tokenized_prompts: {rows.shape[0]} rows for {b} prompts")
        return np.broadcast_to(rows, (b,)).astype(np.int64)

    def _text_features(self, label, view):
        enc = self.text_tower()
        prompts = self.prompt_learner(label, view=view)
        if torch.is_grad_enabled() and prompts.requires_grad:   # prompt learning: see the module docstring
            return enc.forward_grad(prompts, self._eot_rows(prompts.shape[0]))
        return enc.forward(prompts, self._eot_rows(prompts.shape[0]))

    def _raw_features(self, x, view):
        """cat(x12[:,0], xproj[:,0]) before any BatchNorm, whatever TEST.NECK_FEAT says"""
        if self.neck_feat != 'after':
            return self._encode(x, None, view)
        if self._proj_encoder is None:
            self._proj_encoder = self._build_encoder(False, ws_tag="enc_proj")
        keep, self._encoder = self._encoder, self._proj_encoder
        try:
            return self._encode(x, None, view)
        finally:
            self._encoder = keep

    def forward(self, x=None, label=None, get_image=False, get_text=False, cam_label=None, view_label=None,
                image_feature=None, get_raw_text=False, view=None, get_image_update=False, text_feature=None,
                get_more_image=False, exp_setting=None, get_image_vp=False, tta_view=0):
        if get_image_update or get_more_image:
            raise NotImplementedError("feature fusion / multi-token outputs belong to Uni-Prompt training and TTPT, outside "
                                      "the accelerated evaluation path (SURVEY.md §8f)")
        if get_text or get_raw_text:
            if label is None:
                raise NotImplementedError("get_text / get_raw_text encode the identity prompts of `label` (reference "
                                          ":168-170): pass label=...; there is no text output without it")
            # (the reference also runs the image encoder when x is given, :161-166, and does not use the result)
            return self._text_features(label, view)
        if get_image or get_image_vp:
            proj = self._raw_features(x, tta_view)[:, self.in_planes:]
            return proj + self.visual_prompt[0].to(proj.device) if get_image_vp else proj
        if self.training:
            return self._forward_training(x, cam_label, view_label)
        return self._encode(x, self._sie(cam_label, view_label), tta_view)

    def load_param(self, trained_path):
        param_dict = torch.load(trained_path, map_location="cpu")
        own = self.state_dict()
        text = split_text_checkpoint(param_dict, self.num_classes)
        used = set(text[2]) if text is not None else set()
        skipped = 0
        for name in param_dict:
            key = name.replace('module.', '')
            if name in used:
                continue
            if key.startswith(_SKIPPED_PREFIXES):
                skipped += 1
                continue
            own[key].copy_(param_dict[name])
        self._invalidate()
        if text is not None:
            self._text_source = ({k: v.detach().float() for k, v in text[0].items()},
                                 {k: v.detach().float() for k, v in text[1].items()})
            self._text_encoder = None
        print('Loading pretrained model from {}'.format(trained_path))
        if text is not None:
            print('  (text tower: {} tensors loaded)'.format(len(used)))
        if skipped:
            print('  ({} text-tower / fusion tensors are not used at evaluation and were skipped)'.format(skipped))

    def load_param_finetune(self, model_path):
        self.load_param(model_path)


def make_model(cfg, num_class, camera_num, view_num):
    return build_transformer(num_class, camera_num, view_num, cfg)
