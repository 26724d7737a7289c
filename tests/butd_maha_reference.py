"""joint_repr of the BUTD model on the host, for the tests of the Mahalanobis method on BUTD (tests/test_butd_maha_oracle.py,
tests/test_gpu_butd_maha.py) and the fixture generator (tools/gen_g14_butd_maha.py): lines 66-76 of oracle/butd_ref.py butd_forward restated from
its own wn_linear / gru_last - what the reference's GQABUTD_maha returns beside the logits (butd/butd.py:463-467).  Pinned to the reference class by
tests/golden/g14_butd_maha.npz.  Not a test module."""
import functools
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import butd_ref as BR
from rgqa_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSAMP = 4096
CLASSIFIER = ("ans_classifier.0.", "ans_classifier.3.")


def joint_repr(P, c, feat, pos, toks):
    """(joint_repr [B, H], q_repr, img_repr) in the dtype of P / feat"""
    w = F.embedding(toks, P["w_emb.emb.weight"], padding_idx=c.ntoken)
    q = BR.gru_last(w, P)
    img = torch.cat([feat, pos], dim=2)
    ip = torch.relu(BR.wn_linear(img, P, "att.image_proj.mlp.0"))
    qp = torch.relu(BR.wn_linear(q, P, "att.question_proj.mlp.0")).unsqueeze(1)
    att = torch.softmax(BR.wn_linear(ip * qp, P, "att.linear"), dim=1)
    img_enc = (img * att).sum(dim=1)
    q_repr = torch.relu(BR.wn_linear(q, P, "q_project.mlp.0"))
    img_repr = torch.relu(BR.wn_linear(img_enc, P, "img_project.mlp.0"))
    return q_repr * img_repr, q_repr, img_repr


def logits_from(P, joint):
    return BR.wn_linear(torch.relu(BR.wn_linear(joint, P, "ans_classifier.0")), P, "ans_classifier.3")


@functools.lru_cache(None)
def g14():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "g14_butd_maha.npz")))


@functools.lru_cache(None)
def case():
    """(config, unit-gain weights {key: f32 array}, feat, pos, toks): the G7 batch with synth.butd_maha_fill's weights"""
    from tests.test_input_grads_oracle import butd_g7_inputs
    c, filled, feat, pos, toks = butd_g7_inputs()
    return c, synth.butd_maha_fill(filled), feat, pos, toks


def params(dtype, requires_grad=False):
    filled = case()[1]
    return {k: torch.from_numpy(np.asarray(v)).to(dtype).requires_grad_(requires_grad) for k, v in filled.items()}


def joint_on(feat, pos, dtype):
    """joint_repr of the fixture's model on given inputs, no gradient"""
    c, _, _, _, toks = case()
    with torch.no_grad():
        return joint_repr(params(dtype), c, feat.to(dtype), pos.to(dtype), toks)[0]


@functools.lru_cache(None)
def fixture_dp():
    """d loss / d joint_repr of gqa_maha.py:239-244 for the fixture's own joint_repr and prediction: formed in f64, rounded to f32 ([B, H] tensor)"""
    g = g14()
    P = synth.butd_maha_precision()
    B = g["pooled"].shape[0]
    dp = (g["pooled"].astype(np.float64) - g["mean"][g["sample_pred"]].astype(np.float64)) @ P / B
    return torch.from_numpy(dp.astype(np.float32))


def autograd(dtype, dp=None, dl=None):
    """the restatement's autograd of sum(joint * dp) (+ sum(logits * dl)) on the fixture's batch:
    (joint, logits, dfeats, dboxes, {key: parameter gradient or None})"""
    c, _, feat, pos, toks = case()
    P = params(dtype, True)
    f, p = feat.to(dtype).clone().requires_grad_(True), pos.to(dtype).clone().requires_grad_(True)
    joint, _, _ = joint_repr(P, c, f, p, toks)
    lg = logits_from(P, joint)
    loss = 0
    if dp is not None:
        loss = loss + (joint * dp.to(dtype)).sum()
    if dl is not None:
        loss = loss + (lg * dl.to(dtype)).sum()
    loss.backward()
    return joint.detach(), lg.detach(), f.grad, p.grad, {k: v.grad for k, v in P.items()}


@functools.lru_cache(None)
def ref_f64():
    """f64 autograd for the fixture's dp: the reference of the engine tests"""
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    return autograd(torch.float64, dp=fixture_dp())


def check_against_g14(dfeats, dboxes, tol, tag=""):
    """tests/test_input_grads_oracle.py check_against_g12's rule on the g14 fixture: dboxes in full, dfeats at the sampled entries and by its 2-norm"""
    g = g14()
    rb = g["dboxes"].reshape(dboxes.shape)
    rf = g["dfeats_samp"]
    got = dfeats.reshape(-1)[synth.sample_idx("g14.butd.dfeats", dfeats.size, NSAMP)]
    assert np.abs(rb).max() > 0 and np.abs(rf).max() > 0
    eb = np.abs(dboxes - rb).max() / np.abs(rb).max()
    ef = np.abs(got - rf).max() / np.abs(rf).max()
    print("g14 %s: dfeats err / max|ref| %.3e, dboxes err / max|ref| %.3e (bound %.1e)" % (tag, ef, eb, tol))
    assert ef <= tol and eb <= tol, (ef, eb)
    n = float(np.sqrt((dfeats.astype(np.float64) ** 2).sum()))
    full_max = max(float(np.abs(dfeats).max()), float(np.abs(rf).max()))
    assert abs(n - float(g["dfeats_norm"])) <= tol * full_max * np.sqrt(dfeats.size), (n, float(g["dfeats_norm"]))
    return ef, eb
