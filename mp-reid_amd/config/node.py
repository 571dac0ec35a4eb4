import ast
import copy

import yaml


class CfgNode(dict):
    def __init__(self, d=None):
        super().__init__()
        object.__setattr__(self, "_frozen", False)
        for k, v in (d or {}).items():
            self[k] = CfgNode(v) if isinstance(v, dict) else v

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)

    def __setattr__(self, k, v):
        if object.__getattribute__(self, "_frozen"):
            raise AttributeError("config is frozen")
        self[k] = v

    def freeze(self):
        object.__setattr__(self, "_frozen", True)
        for v in self.values():
            if isinstance(v, CfgNode):
                v.freeze()

    def defrost(self):
        object.__setattr__(self, "_frozen", False)
        for v in self.values():
            if isinstance(v, CfgNode):
                v.defrost()

    def clone(self):
        return copy.deepcopy(self)

    def _merge(self, other):
        for k, v in other.items():
            if v is None:      # a section whose keys are all commented out (reference YAMLs have these)
                continue
            if isinstance(v, dict):
                if k not in self or not isinstance(self[k], CfgNode):
                    self[k] = CfgNode()
                self[k]._merge(v)
            else:
                self[k] = v

    def merge_from_file(self, path):
        with open(path) as f:
            self._merge(yaml.safe_load(f) or {})

    def merge_from_list(self, opts):
        opts = list(opts or [])
        assert len(opts) % 2 == 0, "opts must be KEY VALUE pairs"
        for key, val in zip(opts[0::2], opts[1::2]):
            node = self
            parts = key.split(".")
            for p in parts[:-1]:
                node = node.setdefault(p, CfgNode()) if p not in node else node[p]
            if isinstance(val, str):
                try:
                    val = ast.literal_eval(val)
                except (ValueError, SyntaxError):
                    pass
            node[parts[-1]] = val


def _stage1_defaults():
    """SOLVER.STAGE1 / STAGE1A / STAGE1B of the reference (config/defaults.py:123-210: the three sections carry the same keys
    and values).  The stage-1 loop reads IMS_PER_BATCH, MAX_EPOCHS, CHECKPOINT_PERIOD and LOG_PERIOD from STAGE1, the optimizer
    and the schedule OPTIMIZER_NAME, BASE_LR, WEIGHT_DECAY, MOMENTUM, MAX_EPOCHS, LR_MIN, WARMUP_LR_INIT and WARMUP_EPOCHS from the
    section of their stage; the other keys are accepted and unused, as in the reference."""
    return {"IMS_PER_BATCH": 64, "OPTIMIZER_NAME": "Adam", "MAX_EPOCHS": 100, "BASE_LR": 3e-4, "MOMENTUM": 0.9,
            "WEIGHT_DECAY": 0.0005, "WEIGHT_DECAY_BIAS": 0.0005, "WARMUP_FACTOR": 0.01, "WARMUP_EPOCHS": 5,
            "WARMUP_LR_INIT": 0.01, "LR_MIN": 0.000016, "WARMUP_ITERS": 500, "WARMUP_METHOD": "linear", "COSINE_MARGIN": 0.5,
            "COSINE_SCALE": 30, "CHECKPOINT_PERIOD": 10, "LOG_PERIOD": 100, "EVAL_PERIOD": 10}


def _stage2_defaults():
    """SOLVER.STAGE2 of the reference (config/defaults.py:218-265), its keys and values.  The stage-2 optimizers read
    OPTIMIZER_NAME, BASE_LR, LARGE_FC_LR, BIAS_LR_FACTOR, MOMENTUM, WEIGHT_DECAY, WEIGHT_DECAY_BIAS and CENTER_LR, the schedule
    STEPS, GAMMA, WARMUP_FACTOR, WARMUP_ITERS and WARMUP_METHOD, the loop IMS_PER_BATCH (and, through its caller, MAX_EPOCHS,
    LOG_PERIOD, CHECKPOINT_PERIOD, EVAL_PERIOD); the other keys are accepted and unused, as in the reference."""
    return {"IMS_PER_BATCH": 64, "OPTIMIZER_NAME": "Adam", "MAX_EPOCHS": 100, "BASE_LR": 3e-4, "LARGE_FC_LR": False,
            "BIAS_LR_FACTOR": 1, "MOMENTUM": 0.9, "CENTER_LR": 0.5, "CENTER_LOSS_WEIGHT": 0.0005, "WEIGHT_DECAY": 0.0005,
            "WEIGHT_DECAY_BIAS": 0.0005, "GAMMA": 0.1, "STEPS": [40, 70], "WARMUP_FACTOR": 0.01, "WARMUP_EPOCHS": 5,
            "WARMUP_LR_INIT": 0.01, "LR_MIN": 0.000016, "WARMUP_ITERS": 500, "WARMUP_METHOD": "linear", "COSINE_MARGIN": 0.5,
            "COSINE_SCALE": 30, "CHECKPOINT_PERIOD": 10, "LOG_PERIOD": 100, "EVAL_PERIOD": 10}


def make_defaults():
    return CfgNode({
        "SOLVER": {"STAGE1": _stage1_defaults(), "STAGE1A": _stage1_defaults(), "STAGE1B": _stage1_defaults(),
                   "STAGE2": _stage2_defaults(), "SEED": 1234,
                   "MARGIN": 0.3},   # the triplet loss's margin (loss/make_loss.py)
        "MODEL": {"NAME": "ViT-B-16", "DEVICE": "cuda", "DEVICE_ID": "0", "STRIDE_SIZE": [16, 16],
                  # what loss/make_loss.py reads (reference config/defaults.py:39-49)
                  "ID_LOSS_WEIGHT": 1.0, "TRIPLET_LOSS_WEIGHT": 1.0, "I2T_LOSS_WEIGHT": 1.0, "METRIC_LOSS_TYPE": "triplet",
                  "NO_MARGIN": False, "IF_LABELSMOOTH": "on",
                  "SIE_CAMERA": False, "SIE_VIEW": False, "SIE_COE": 3.0, "NECK": "bnneck", "COS_LAYER": False,
                  "DIST_TRAIN": False, "INIT_SEED": 7, "ENCODER_PRECISION": "split",
                  # not a reference key: the row of the Uni-Prompt prompt that get_text reads out.  The reference takes it
                  # from tokenized_prompts.argmax(-1), a tensor that is in no checkpoint.  19 = the end-of-text position of
                  # its template "X X ... X person." (16 X): start token, 16 context tokens, `person`, `.`, end token.
                  # DERIVED from the template, NOT checked against the BPE tokenizer (which this build does not ship);
                  # model.prompt_learner.tokenized_prompts, when a caller sets it, takes precedence
                  "PROMPT_EOT_INDEX": 19,
                  # the reference's keys (config/defaults.py:65-73): the first MOE_LAYERS blocks (-1: all) of the ViT image
                  # tower carry NUM_EXPERTS expert MLPs behind a softmax gate, TOP_K of them per token.  DROPOUT is accepted
                  # and unused at eval
                  "MOE": {"ENABLED": False, "NUM_EXPERTS": 0, "TOP_K": 0, "MOE_LAYERS": 0, "DROPOUT": 0.0}},
        "INPUT": {"SIZE_TRAIN": [256, 128], "SIZE_TEST": [256, 128], "PIXEL_MEAN": [0.5, 0.5, 0.5],
                  "PIXEL_STD": [0.5, 0.5, 0.5],
                  # train_transforms (reference config/defaults.py:83-91): the probability of the horizontal flip, the zero
                  # padding in front of the random crop, the probability of random erasing
                  "PROB": 0.5, "PADDING": 10, "RE_PROB": 0.5},
        "DATASETS": {"NAMES": "synthetic", "ROOT_DIR": "", "EXP_SETTING": "", "SYNTH_QUERY": 3368,
                     "SYNTH_GALLERY": 15913, "SYNTH_IDS": 751, "SYNTH_SEED": 1234,
                     # SYNTH_RAW: the loader hands over DECODED uint8 images of ragged sizes (what PIL gives before
                     # val_transforms) and Resize + ToTensor + Normalize run on the GPU
                     "SYNTH_RAW": False,
                     # SYNTH_TRAIN > 0: that many synthetic TRAINING images of SYNTH_IDS identities; make_dataloader then
                     # returns the two training loaders (0: None, None -- evaluation only)
                     "SYNTH_TRAIN": 0,
                     # PROTOCOL 'vehicleid' (not a reference key; the reference branches on NAMES == 'VehicleID', test.py:46):
                     # TEST.TRIALS trials over ONE encoded pool, in each of them one random image per identity is the
                     # gallery and all the others are queries (datasets/make_dataloader.py:vehicleid_trial_splits, drawn
                     # from TRIAL_SEED).  '' = the single query-then-gallery evaluation
                     "PROTOCOL": "", "TRIAL_SEED": 0},
        "DATALOADER": {"NUM_WORKERS": 0, "SAMPLER": "softmax", "NUM_INSTANCE": 16},
        "TEST": {"IMS_PER_BATCH": 64, "RE_RANKING": False, "WEIGHT": "", "NECK_FEAT": "before", "FEAT_NORM": "yes",
                 "DIST_MAT": "dist_mat.npy", "EVAL": False,
                 "DISTANCE_MODE": "exact", "RERANK_ALGO": "exact",   # not reference keys: see processor.do_inference
                 # not a reference key: True evaluates under the Market-1501 protocol -- for each query the gallery images
                 # of the same identity from the same camera are removed (utils/metrics.py; the reference's eval_func
                 # keeps that line commented out, utils/metrics.py:54)
                 "REMOVE_SAME_CAM": False,
                 # not reference keys: RANK_LIST_K > 0 keeps, for every query, its first K gallery images in ranked order
                 # (utils/metrics.py:rank_lists; K <= 1024) and test.py writes them to RANK_LIST_FILE
                 # ('' = <OUTPUT_DIR>/rank_lists.npz; no OUTPUT_DIR either: nothing is written)
                 "RANK_LIST_K": 0, "RANK_LIST_FILE": "",
                 # not reference keys: QE_K > 0 turns on query expansion in feature space before ranking (AQE on the
                 # queries, DBA on the gallery rows; utils/metrics.py:expand_features) -- every feature row becomes the mean
                 # of its first QE_K neighbours (itself included; K <= 1024) weighted by cosine ** QE_ALPHA, QE_TIMES rounds
                 "QE_K": 0, "QE_ALPHA": 3.0, "QE_TIMES": 1,
                 # not reference keys: EXTRA_METRICS True also reports mINP (how deep a query's hardest true match sits) and,
                 # over ALL query x gallery pairs, TPR at the false-positive rates ROC_FPRS; PAIR_HIST_BINS > 0 (<= 4095) adds
                 # the positive- / negative-pair distance histograms over PAIR_HIST_RANGE, written to
                 # <OUTPUT_DIR>/pair_hist.npz (utils/metrics.py: eval_metrics, tpr_at_fpr, pair_counts)
                 "EXTRA_METRICS": False, "ROC_FPRS": [1e-4, 1e-3, 1e-2], "PAIR_HIST_BINS": 0, "PAIR_HIST_RANGE": [0.0, 4.0],
                 "TRIALS": 10,   # DATASETS.PROTOCOL 'vehicleid': number of trials (the reference's loop runs 10, test.py:47)
                 # Uni-Prompt evaluation (reference config/defaults.py:331-344)
                 "TTA_ENABLED": False, "TTPT": {"ENABLED": False, "LR": 0.001, "STEPS": 5, "TEMPERATURE": 0.07}},
        "OUTPUT_DIR": "",
    })
