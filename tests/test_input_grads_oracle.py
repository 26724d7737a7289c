"""Input gradients of the ODIN scorer (tasks/gqa_odin.py:97-112) for BUTD and UNITER: the oracles' autograd (oracle/butd_ref.py,
oracle/uniter_ref.py: functional torch) against tests/golden/g12_input_grads.npz, which the reference's own GQABUTD and UNITER modules
produced (tools/gen_g12_input_grads.py).  No GPU.

Both sides get the SAME dlogits, built from the fixture's column, target and logits: at temperature 1e5 the reference's column and target
are decided by the last bit of an f32 sigmoid value (whole rows tie), so neither may be re-chosen by the side under test.

Bound: atol = 2e-4 * max|ref| - 4x the largest difference between an oracle in f32 and the same oracle in f64 on these cases (BUTD 4.8e-5,
UNITER 5.8e-7 small / 2.4e-6 full, all relative to max|ref|)."""
import os

import numpy as np
import pytest
import torch

from oracle import lxmert_ref as R
from oracle import uniter_ref as U
from rgqa_amd import synth
from rgqa_amd.synth import BUTD_WORDS, BUTD_SENTS, U_SMALL, U_FULL, uniter_batch, sample_idx

TOL = 2e-4
NSAMP = 4096
UNITER_CASES = {("small", 5): (3, 6, 91), ("small", 8): (3, 6, 92), ("full", 20): (4, 36, 93)}


def g12(golden_dir):
    return np.load(os.path.join(golden_dir, "g12_input_grads.npz"))


def odin_dlogits_from(logits, col, y):
    """d/dlogits of mean_b BCEWithLogits(logits[b, col[b]], y[b]) (gqa_odin.py:107-110) for GIVEN columns and targets: f32 [B, NA]"""
    z = torch.as_tensor(logits, dtype=torch.float64)
    col = torch.as_tensor(col, dtype=torch.int64)
    y = torch.as_tensor(y, dtype=torch.float64)
    B = z.shape[0]
    d = torch.zeros_like(z)
    r = torch.arange(B)
    d[r, col] = (torch.sigmoid(z[r, col]) - y) / B
    return d.float()


def butd_g7_inputs():
    from oracle import butd_ref as BR
    from tests.test_oracle_golden import butd_fill
    c = BR.ButdConfig(ntoken=len(BUTD_WORDS), num_answers=23)
    filled = butd_fill(c)
    b = synth.synth_batch(len(BUTD_SENTS), 8, O=36, F=2048, NA=23, vocab=64, seed=606, uq_frac=0.2)
    word2idx = {w: i for i, w in enumerate(BUTD_WORDS)}
    toks = torch.tensor(BR.tokenize(BUTD_SENTS, word2idx), dtype=torch.int64)
    return c, filled, torch.from_numpy(b["feats"]), torch.from_numpy(b["boxes"]), toks


def butd_oracle_input_grads(c, filled, feat, pos, toks, dlogits, dtype=torch.float32):
    """(logits, dfeats, dboxes) of the BUTD oracle's autograd in `dtype` for the given dlogits"""
    from oracle import butd_ref as BR
    P = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in filled.items()}
    f, p = feat.to(dtype).clone().requires_grad_(True), pos.to(dtype).clone().requires_grad_(True)
    lg = BR.butd_forward(P, c, f, p, toks)
    lg.backward(dlogits.to(dtype))
    return lg.detach(), f.grad, p.grad


def uniter_case(tag, T):
    cfgd = U_SMALL if tag == "small" else U_FULL
    B, O, seed = UNITER_CASES[(tag, T)]
    return cfgd, uniter_batch(cfgd, T, B, O, seed)


def uniter_oracle_input_grads(cfgd, b, dlogits):
    cfg = R.RefConfig(**cfgd)
    P = {k: torch.from_numpy(v) for k, v in synth.fill_state_dict(U.param_shapes(cfg)).items()}
    t = {k: torch.from_numpy(v) for k, v in b.items() if k != "lengths"}
    f, p = t["feats"].clone().requires_grad_(True), t["pos7"].clone().requires_grad_(True)
    lg, _ = U.gqa_forward(P, cfg, f, p, t["input_ids"], t["input_mask"], t["segment_ids"])
    lg.backward(dlogits)
    return lg.detach(), f.grad, p.grad


def check_against_g12(g, case, dfeats, dboxes, tol, tag=""):
    """dfeats / dboxes (numpy) against the fixture: full arrays, or the samples and the 2-norm.  Returns the printed errors / max|ref|."""
    rb = g[case + ".dboxes"].reshape(dboxes.shape)
    assert np.abs(rb).max() > 0
    eb = np.abs(dboxes - rb).max() / np.abs(rb).max()
    if case + ".dfeats" in g.files:
        rf = g[case + ".dfeats"].reshape(dfeats.shape)
        got = dfeats
    else:
        rf = g[case + ".dfeats_samp"]
        got = dfeats.reshape(-1)[sample_idx("g12.%s.dfeats" % case, dfeats.size, NSAMP)]
    assert np.abs(rf).max() > 0
    ef = np.abs(got - rf).max() / np.abs(rf).max()
    print("%s %s: dfeats err / max|ref| %.3e, dboxes err / max|ref| %.3e (bound %.1e)" % (case, tag, ef, eb, tol))
    assert ef <= tol and eb <= tol, (case, ef, eb)
    if case + ".dfeats_norm" in g.files:
        # every entry within tol * max|ref| => the 2-norms differ by at most tol * max|ref| * sqrt(numel); max|ref| >= the sampled maximum
        n = float(np.sqrt((dfeats.astype(np.float64) ** 2).sum()))
        ref_n = float(g[case + ".dfeats_norm"])
        full_max = max(float(np.abs(dfeats).max()), float(np.abs(rf).max()))
        assert abs(n - ref_n) <= tol * full_max * np.sqrt(dfeats.size), (case, n, ref_n)
    return ef, eb


def test_butd_oracle_input_gradients_vs_reference(golden_dir):
    g = g12(golden_dir)
    c, filled, feat, pos, toks = butd_g7_inputs()
    dl = odin_dlogits_from(g["butd_g7.logits"], g["butd_g7.col"], g["butd_g7.y"])
    lg, df, db = butd_oracle_input_grads(c, filled, feat, pos, toks, dl)
    np.testing.assert_allclose(lg.numpy(), g["butd_g7.logits"], rtol=0, atol=2e-5)
    check_against_g12(g, "butd_g7", df.numpy(), db.numpy(), TOL, "oracle f32")


@pytest.mark.parametrize("tag,T", [("small", 5), ("small", 8), ("full", 20)])
def test_uniter_oracle_input_gradients_vs_reference(golden_dir, tag, T):
    g = g12(golden_dir)
    case = "uniter_%s_T%d" % (tag, T)
    cfgd, b = uniter_case(tag, T)
    dl = odin_dlogits_from(g[case + ".logits"], g[case + ".col"], g[case + ".y"])
    lg, df, dp = uniter_oracle_input_grads(cfgd, b, dl)
    np.testing.assert_allclose(lg.numpy(), g[case + ".logits"], rtol=0, atol=5e-6 if tag == "small" else 5e-5)
    check_against_g12(g, case, df.numpy(), dp.numpy(), TOL, "oracle f32")


def test_fixture_columns_are_the_ties_the_issue_describes(golden_dir):
    """The columns the reference's statements chose at temperature 1e5: ties resolved to the first index - every G7 row picks column 4"""
    g = g12(golden_dir)
    assert g["butd_g7.col"].tolist() == [4] * 5
    for case in ("butd_g7", "uniter_small_T5", "uniter_small_T8", "uniter_full_T20"):
        z = torch.from_numpy(g[case + ".logits"])
        preds = torch.sigmoid(z / 1e5)
        assert torch.equal(torch.max(preds, 1)[1], torch.from_numpy(g[case + ".col"]))
        assert torch.equal((preds >= 0.5).float().gather(1, torch.from_numpy(g[case + ".col"]).unsqueeze(1)).squeeze(1), torch.from_numpy(g[case + ".y"]))
