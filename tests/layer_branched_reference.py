"""The reference's layer-wise confidence-branch model (tasks/gqa_branched_layer.py:47-59 GQAProjector, :104-110 all_feats, :280-320 GQAModel_branched) restated
with torch on top of the oracle's encoder, whose trace holds every cross-modality layer's language output.  The trainer statements (:396-413) and the scorer
(:480-485) are those of tasks/gqa_branched.py: tests.branched_reference.trainer_statements / scores, one copy.  Shared by tools/gen_g16_branched_layer.py,
tests/test_layer_branched_host.py and tests/test_gpu_layer_branched.py; runs on the CPU in the dtype of the weights it is given.  Not a test module."""
import math

import numpy as np
import torch

from rgqa_amd import synth
from tests.branched_reference import trainer_statements, scores      # noqa: F401  (re-exported: the statements of this model's trainer)

CONF_FC_KEYS = ("conf_fc.0.weight", "conf_fc.0.bias", "conf_fc.2.weight", "conf_fc.2.bias", "conf_fc.3.weight", "conf_fc.3.bias")
GROUPS = ("encoder.layer.", "r_layers.", "x_layers.0.", "x_layers.1.")      # condition (b) of the fixture: one stored tensor of each must feel the branch
F32_GATE = dict(rtol=2e-3, atol=1e-6, atol_rel=2e-4)                       # the f32 gradient gate of tests/test_gpu_branched.py


def branch_keys(X):
    """state_dict keys of the branch in the engine's table order: the projectors, then conf_fc"""
    ks = []
    for i in range(X):
        ks += ["projs.%d.proj.0.weight" % i, "projs.%d.proj.0.bias" % i]
    return tuple(ks) + CONF_FC_KEYS


def branch_shapes(H, X, P):
    s = {}
    for i in range(X):
        s["projs.%d.proj.0.weight" % i], s["projs.%d.proj.0.bias" % i] = (P, H), (P,)
    n = X * P
    s.update(zip(CONF_FC_KEYS, [(2 * n, n), (2 * n,), (2 * n,), (2 * n,), (1, 2 * n), (1,)]))
    return s


def is_branch(key):
    return key.startswith(("projs.", "conf_fc."))


def param_shapes(cfgd, P):
    """every state_dict key of the model -> shape (the oracle's GQAModel keys + the branch)"""
    from oracle import lxmert_ref as R
    shapes = dict(R.param_shapes(R.RefConfig(**cfgd)))
    shapes.update(branch_shapes(cfgd["hidden"], cfgd["x_layers"], P))
    return shapes


def weights(cfgd, P, dtype, fill=None):
    """{key: leaf tensor with requires_grad} filled by `fill` (default: synth.layer_branched_fill, the fixture's filler)"""
    filled = (fill or synth.layer_branched_fill)(param_shapes(cfgd, P))
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(True) for k, v in filled.items()}


def head(W, taps, eps=1e-12):
    """the branch alone: taps = the [CLS] row [B, H] of every cross-modality layer's language output -> (conf [B, 1], projcat [B, X P])"""
    projcat = torch.cat([torch.tanh(t @ W["projs.%d.proj.0.weight" % i].t() + W["projs.%d.proj.0.bias" % i]) for i, t in enumerate(taps)], 1)      # :47-59, :313-317
    h = projcat @ W["conf_fc.0.weight"].t() + W["conf_fc.0.bias"]                                                                                     # :285-291
    h = h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    h = torch.nn.functional.layer_norm(h, (h.shape[1],), W["conf_fc.2.weight"], W["conf_fc.2.bias"], eps)
    return h @ W["conf_fc.3.weight"].t() + W["conf_fc.3.bias"], projcat


def forward(W, cfgd, batch, eps=1e-12):
    """-> (logit [B, NA], conf [B, 1], projcat [B, X P], pooled [B, H]) in the dtype of W; batch: dict of torch tensors (feats, boxes, input_ids, input_mask,
    segment_ids)"""
    from oracle import lxmert_ref as R
    cfg = R.RefConfig(**cfgd)
    dtype = W["logit_fc.0.weight"].dtype
    tr = {}
    logit, pooled = R.gqa_forward({k: v for k, v in W.items() if not is_branch(k)}, cfg, batch["feats"].to(dtype), batch["boxes"].to(dtype), batch["input_ids"],
                                  batch["input_mask"], batch["segment_ids"], trace=tr)
    conf, projcat = head(W, [tr["x%d_lang" % i][:, 0] for i in range(cfgd["x_layers"])], eps)
    return logit, conf, projcat, pooled


def fixture_index(form, key, numel):
    """which elements of a gradient tests/golden/g16_branched_layer.npz stores, as g15 samples them: None = the whole tensor, else indices into the flattened one.
    (g15's counts - whole up to 4096 elements, 1024 of the larger ones - would put this file, with one more layer and the noconf set, at 2 MiB: whole up to 1024
    elements, 512 of the larger ones.)"""
    if form == "mce":
        return synth.sample_idx(key, numel)
    if key.startswith("logit_fc.") or is_branch(key) or numel <= 1024:
        return None
    return synth.sample_idx(key, numel, 512)


def gate(ref):
    """element-wise tolerance of the f32 GPU gradient gate for a reference array"""
    ref = np.asarray(ref, dtype=np.float64)
    return F32_GATE["atol"] + F32_GATE["atol_rel"] * np.abs(ref).max() + F32_GATE["rtol"] * np.abs(ref)


def branch_reach(g, factor=50.0):
    """condition (b) from a fixture's arrays: {group: largest (|full - noconf| / gate) over the stored tensors of the group} and whether each reaches `factor`"""
    out = {}
    for grp in GROUPS:
        best = 0.0
        for k in g.files if hasattr(g, "files") else g:
            if k.startswith("bce.grad.") and grp in k and ("noconf.grad." + k[len("bce.grad."):]) in g:
                full, nc = np.asarray(g[k], np.float64), np.asarray(g["noconf.grad." + k[len("bce.grad."):]], np.float64)
                best = max(best, float((np.abs(full - nc) / gate(full)).max()))
        out[grp] = best
    return out, all(v >= factor for v in out.values())
