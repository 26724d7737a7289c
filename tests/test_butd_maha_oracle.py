"""The Mahalanobis method on BUTD, host side (no GPU): tests/golden/g14_butd_maha.npz - what the reference's own GQABUTD_maha produced on the G7
batch (tools/gen_g14_butd_maha.py) - pins the restated joint_repr of tests/butd_maha_reference.py, forward and autograd, and the drop-in class
exists under both import paths.

Bounds: forward atol 2e-5 * max(1, max|ref|), what tests/test_input_grads_oracle.py holds the BUTD oracle's logits to; gradients TOL = 2e-4 of
max|ref| under check_against_g12's rule (samples, 2-norm, boxes in full), that file's bound for the same oracle's input gradients."""
import os
import sys

import numpy as np
import torch

from rgqa_amd import synth
from tests import butd_maha_reference as BM
from tests.test_input_grads_oracle import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_pins_the_restated_joint_repr():
    g = BM.g14()
    c, _, feat, pos, toks = BM.case()
    x = BM.joint_on(feat, pos, torch.float32).numpy()
    ref = g["pooled"]
    err, bound = float(np.abs(x - ref).max()), 2e-5 * max(1.0, float(np.abs(ref).max()))
    print("g14: restated joint_repr f32 vs the reference's: max err %.3e (bound %.1e; max|ref| %.3f, exact zeros %.1f %% / %.1f %%)" % (
        err, bound, np.abs(ref).max(), 100 * (ref == 0).mean(), 100 * (x == 0).mean()))
    assert err <= bound
    assert g["mean"].shape == (synth.BUTD_MAHA_NC, synth.BUTD_MAHA_H) and ref.shape == (5, synth.BUTD_MAHA_H)
    # the stored f64 scores are the f64 evaluation on the stored vectors with the regenerated precision matrix
    P = synth.butd_maha_precision()
    for key, sk, lab in (("pooled", "score_f64", "sample_pred"), ("pooled2", "score2_f64", "label2")):
        d = g[key].astype(np.float64)[:, None, :] - g["mean"].astype(np.float64)[None, :, :]
        s = -0.5 * np.einsum("bch,hk,bck->bc", d, P, d)
        np.testing.assert_allclose(s, g[sk], rtol=1e-9)
        assert np.array_equal(s.argmax(1), g[lab])
    assert len(set(g["sample_pred"].tolist())) >= 2


def test_fixture_pins_the_restated_autograd():
    """dp = (pooled - mean[sample_pred]) P / B formed in f64 and rounded to f32 (as tests/test_gpu_maha.py
    test_input_gradients_through_the_pooled_output forms it) through the f32 restatement's autograd, against the reference's feats.grad / boxes.grad"""
    _, _, df, db, pg = BM.autograd(torch.float32, dp=BM.fixture_dp())
    BM.check_against_g14(df.numpy(), db.numpy(), TOL, "restatement f32")
    # joint_repr does not pass through the classifier
    assert all((v is None) == k.startswith(BM.CLASSIFIER) for k, v in pg.items())


def test_gqabutd_maha_is_importable_from_both_trees():
    from rgqa_amd.butd.butd import GQABUTD, GQABUTD_maha
    assert issubclass(GQABUTD_maha, GQABUTD) and GQABUTD_maha is not GQABUTD
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import importlib
        mod = importlib.import_module("butd.butd")
        assert mod.GQABUTD_maha is GQABUTD_maha and mod.GQABUTD is GQABUTD
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
