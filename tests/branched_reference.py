"""The reference's confidence-branch model and trainer statements (tasks/gqa_model_branched.py:28-33, :47-51; tasks/gqa_branched.py:126-143, :147, :206-214)
restated with torch, and the inputs the branched tests draw.  Shared by tools/gen_g15_branched.py, tests/test_branched_host.py and
tests/test_gpu_branched.py; runs on the CPU in the dtype it is asked for.  Not a test module."""
import math

import numpy as np
import torch

CONF_KEYS = ("conf_fc.0.weight", "conf_fc.0.bias", "conf_fc.2.weight", "conf_fc.2.bias", "conf_fc.3.weight", "conf_fc.3.bias")


def fixture_index(form, key, numel):
    """which elements of a gradient tests/golden/g15_branched.npz stores (tools/gen_g15_branched.py): None = the whole tensor, else indices into the flattened one"""
    from rgqa_amd import synth
    if form == "mce":
        return synth.sample_idx(key, numel)
    if key.startswith(("logit_fc.", "conf_fc.")) or numel <= 4096:
        return None
    return synth.sample_idx(key, numel, 1024)


def conf_head(pooled, w, eps=1e-12):
    """conf_fc on the pooled vector: Linear(H, 2H) -> exact-erf GeLU -> LayerNorm(2H) -> Linear(2H, 1).  w: {state_dict key: tensor} in pooled's dtype.
    Returns conf [B, 1]."""
    h = pooled @ w["conf_fc.0.weight"].t() + w["conf_fc.0.bias"]
    h = h * 0.5 * (1.0 + torch.erf(h / math.sqrt(2.0)))
    h = torch.nn.functional.layer_norm(h, (h.shape[1],), w["conf_fc.2.weight"], w["conf_fc.2.bias"], eps)
    return h @ w["conf_fc.3.weight"].t() + w["conf_fc.3.bias"]


def trainer_statements(logit, conf, target, mce_loss=False):
    """gqa_branched.py:126-142 and :147.  target carries the UQ column last; conf [B, 1] or [B].  Returns (loss, loss_ce, loss_conf, sigmoid(conf) [B], label)."""
    id_inds = target[:, -1] == 0                                                                        # :126
    target = target[:, :-1]                                                                             # :127
    if mce_loss:
        _, tgt = target.max(1)                                                                          # :133
        loss_ce = torch.nn.CrossEntropyLoss(ignore_index=-1)(logit[id_inds], tgt[id_inds]) * logit.size(1)      # :134
    else:
        loss_ce = torch.nn.BCEWithLogitsLoss()(logit[id_inds], target[id_inds])                         # :136
        loss_ce = loss_ce * logit.size(1)                                                               # :137
    conf = torch.sigmoid(conf).reshape(-1)                                                              # :138 (squeeze: B > 1)
    conf_target = id_inds.to(conf.dtype)                                                                # :139
    loss_conf = torch.nn.functional.binary_cross_entropy(conf, conf_target)                            # :140
    loss = loss_ce + loss_conf                                                                          # :142
    _, label = logit.max(1)                                                                             # :147
    return loss, loss_ce, loss_conf, conf, label


def evaluate(z, c, target_uq, mce_loss, dtype):
    """the statements and their backward to the logits / conf logits in `dtype` on the CPU: dict(loss, loss_ce, loss_conf, conf, dlogits, dconf, score1) as
    f64, label int64.  An empty answerable subset leaves a NaN loss_ce whose backward is NaN-free zeros on the logits, as torch computes it."""
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    cc = c.detach().to(dtype).reshape(-1).clone().requires_grad_(True)
    loss, ce, cf, conf, label = trainer_statements(zz, cc, target_uq.to(dtype), mce_loss)
    loss.backward()
    d = lambda t: t.detach().double()
    dz = d(zz.grad)
    return dict(loss=d(loss), loss_ce=d(ce), loss_conf=d(cf), conf=d(conf), dlogits=torch.nan_to_num(dz, nan=0.0) if not bool((target_uq[:, -1] == 0).any()) else dz,
                dconf=d(cc.grad), score1=d(torch.sigmoid(zz).max(1)[0]), label=label)      # score1: :209


def closed_form(z, c, target_uq, mce_loss):
    """dlogits and dconf in closed form, f64: what rgqa_amd/csrc/branched_loss.hip computes (its header)"""
    z, c, t = z.double(), c.double().reshape(-1), target_uq.double()
    idm = t[:, -1] == 0
    n_id, B, NA = int(idm.sum()), z.shape[0], z.shape[1]
    t = t[:, :-1]
    if mce_loss:
        onehot = torch.zeros_like(z)
        onehot[torch.arange(B), t.max(1)[1]] = 1.0
        dz = (NA / max(n_id, 1)) * (torch.softmax(z, 1) - onehot)
    else:
        dz = (torch.sigmoid(z) - t) / max(n_id, 1)
    dz = dz * idm[:, None].double()
    return dz, (torch.sigmoid(c) - idm.double()) / B


def scores(logit, conf, mix):
    """gqa_branched.py:209-214 -> (score, label)"""
    score1, label = torch.sigmoid(logit).max(1)
    score2 = torch.sigmoid(conf).squeeze()
    return (score1 * score2 if mix else score2), label


def draw(B, NA, seed, uq="third"):
    """logits 3 randn - 6, conf logits uniform in [-8, 8]; unanswerable rows (UQ column 1, all-zero answers): every third row starting at row 1 ("third"),
    or all ("all"); two soft target entries (0.9, 0.3) per answerable row.  Returns (logits [B, NA], conf_logit [B], target_with_uq [B, NA + 1]) f32 on the CPU."""
    rng = np.random.RandomState(seed)
    z = (3.0 * rng.standard_normal((B, NA)) - 6.0).astype(np.float32)
    c = rng.uniform(-8.0, 8.0, B).astype(np.float32)
    t = np.zeros((B, NA + 1), np.float32)
    for b in range(B):
        if {"third": b % 3 == 1, "all": True}[uq]:
            t[b, NA] = 1.0
        else:
            k = rng.choice(NA, 2, replace=False)
            t[b, k[0]], t[b, k[1]] = 0.9, 0.3
    return torch.from_numpy(z), torch.from_numpy(c), torch.from_numpy(t)
