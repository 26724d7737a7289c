"""The Mahalanobis test method on BUTD (tasks/gqa_maha.py with GQABUTD_maha, butd/butd.py:355-469): rgqa_engine_backward_pooled on the BUTD
engine - the backward from joint_repr = q_repr * img_repr - in all four precisions against the f64 restatement of
tests/butd_maha_reference.py (pinned to the reference's own class by tests/golden/g14_butd_maha.npz, tests/test_butd_maha_oracle.py), and
`maha_scores` / `maha_sample_estimator` through the drop-in `GQABUTD_maha`.  Everything at the G7 shape (B = 5, 36 regions, 40 tokens, 23
answers; hidden 1024 and feature width 2048 are fixed by the class) with the unit-gain weights of synth.butd_maha_fill, but for the last test.

Bounds are those the same engine's input and parameter gradients are held to through the logits entry (tests/test_gpu_odin.py BUTD_GTOL,
tests/test_gpu_butd.py gtol): the pooled entry is a sub-chain of that one.  Measured values: docs/MEASUREMENTS.md "Mahalanobis on BUTD"."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from rgqa_amd import synth                                                       # noqa: E402
from rgqa_amd.synth import BUTD_WORDS, BUTD_SENTS, sample_idx                    # noqa: E402
from tests import butd_maha_reference as BM                                      # noqa: E402
from tests.test_gpu_odin import BUTD_GTOL, butd_engine, rel_errors, sign_agreement   # noqa: E402
from tests.test_gpu_maha import MARGIN, accumulate_numpy, by_hand, score_f64, synthetic   # noqa: E402

B, O, F, PD, H, NC = 5, 36, 2048, 4, synth.BUTD_MAHA_H, synth.BUTD_MAHA_NC
GTOL_PARAM = 3e-3            # tests/test_gpu_butd.py test_butd_vs_reference_golden, f32
NOISE = synth.BUTD_MAHA_NOISE


def engine(prec):
    _, filled, _, _, _ = BM.case()
    return butd_engine(prec, filled, len(BUTD_WORDS), NC, B, 40, O)


def fwd_args():
    _, _, feat, pos, toks = BM.case()
    kg = toks.cuda()
    return feat.cuda(), pos.cuda(), kg, kg, None


def pooled_input_grads(e, dp):
    """backward_pooled without input-gradient buffers, then twice with them: (dfeats, dboxes, arena) after the bit-identity checks"""
    args = fwd_args()
    e.forward(*args)
    e.backward_pooled(dp)
    g0 = e.grads.clone()
    runs = []
    for _ in range(2):
        df = torch.full((B * O, F), 7.0, device="cuda")
        db = torch.full((B * O, PD), 7.0, device="cuda")
        e.set_input_grads(df, db)
        e.forward(*args)
        e.backward_pooled(dp)
        e.set_input_grads(None, None)
        runs.append((df, db, e.grads.clone()))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][2], g0) and torch.equal(runs[1][2], g0), "parameter gradients changed by asking for input gradients"
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "second run differs from the first"
    return runs[0][0], runs[0][1], g0


def check_param_grads(tag, e, arena, ref, classifier_zero, gtol=GTOL_PARAM):
    """every parameter against the f64 autograd: 2-norm within gtol * ref_norm, sampled entries within 3 * gtol * max|ref| (the rule of
    tests/test_gpu_butd.py test_butd_vs_reference_golden); classifier_zero: the classifier's tensors are exact zeros instead"""
    wn = ws = 0.0
    smallest = float("inf")
    for sp in e.specs:
        got = e.view(arena, sp).cpu().numpy()
        if classifier_zero and sp.name.startswith(BM.CLASSIFIER):
            assert float(np.abs(got).max()) == 0.0, sp.name
            continue
        r = ref[sp.name].numpy().reshape(got.shape)
        ref_norm = float(np.sqrt((r ** 2).sum()))
        dn = abs(float(np.sqrt((got.astype(np.float64) ** 2).sum())) - ref_norm)
        idx = sample_idx(sp.name, got.size)
        rs = r.reshape(-1)[idx]
        ds = float(np.abs(got.reshape(-1)[idx] - rs).max())
        if ref_norm > 1e-6:           # (att.linear.bias: the softmax over the regions ignores it, its gradient is zero up to rounding on both sides)
            wn, ws = max(wn, dn / ref_norm), max(ws, ds / max(float(np.abs(rs).max()), 1e-6))
        # that test's rule to the letter, its absolute floors (1e-7; 1e-6 under the sampled maximum) included: they carry the tensors whose gradient is zero
        assert dn <= gtol * ref_norm + 1e-7, (sp.name, dn, ref_norm)
        assert ds <= 3 * gtol * max(float(np.abs(rs).max()), 1e-6) + 1e-7, (sp.name, ds, float(np.abs(rs).max()))
        smallest = min(smallest, ref_norm) if ref_norm > 1e-6 else smallest
    print("%s: smallest reference gradient norm above 1e-6: %.3e" % (tag, smallest))
    print("%s: worst gradient-norm rel err %.3e (bound %.1e), worst sampled-entry err / max %.3e (bound %.1e)" % (tag, wn, gtol, ws, 3 * gtol))
    emb = [sp for sp in e.specs if sp.name == "w_emb.emb.weight"][0]
    assert float(e.view(arena, emb)[len(BUTD_WORDS)].abs().max()) == 0.0       # the padding row gets no gradient


def classifier_tail(e):
    """the arena range of ans_classifier.0 / .3: the tail of the arena from ans_classifier.0.bias on"""
    return min(sp.offset for sp in e.specs if sp.name.startswith(BM.CLASSIFIER))


# ------------------------------------------------------------------------------------------------ 1. the engine entry
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "bf16x3_fwd"])
def test_backward_pooled_input_gradients_vs_f64(prec):
    """dfeats / dboxes of the pooled entry within 3 * BUTD_GTOL[prec] * max|ref| of the f64 restatement; the sign of every element inside the mask
    of tests/test_gpu_odin.py is gated for f32 / bf16x3 and printed for bf16 / bf16x3_fwd, as the BUTD ODIN tests do.  (bf16 and bf16x3_fwd take the
    persistent GRU backward at this batch.)"""
    joint, _, rf, rb, _ = BM.ref_f64()
    rf, rb = rf.numpy().reshape(-1, F), rb.numpy().reshape(-1, PD)
    e = engine(prec)
    dp = BM.fixture_dp().cuda()
    _, pooled = e.forward(*fwd_args())
    perr = float((pooled.cpu().double() - joint).abs().max())
    print("butd maha %s: engine joint_repr vs the f64 restatement: max err %.3e (max|joint| %.3f)" % (prec, perr, float(joint.abs().max())))
    df, db, _ = pooled_input_grads(e, dp)
    df, db = df.cpu().numpy(), db.cpu().numpy()
    tol = 3 * BUTD_GTOL[prec]
    ef, eb = rel_errors("butd maha pooled entry %s" % prec, df, db, rf, rb, tol)
    gate = prec in ("f32", "bf16x3")
    sign_agreement("butd maha %s dfeats" % prec, df, rf, gate=gate)
    sign_agreement("butd maha %s dboxes" % prec, db, rb, gate=gate)
    assert ef <= tol and eb <= tol, (prec, ef, eb)
    if prec == "f32":       # and against the reference's own autograd (samples, norm, boxes in full)
        BM.check_against_g14(df.reshape(B, O, F), db.reshape(B, O, PD), tol, "engine f32")


def test_backward_pooled_parameter_gradients_f32():
    _, _, _, _, pg = BM.ref_f64()
    e = engine("f32")
    e.grads.fill_(3.0)                     # accumulate = 0 overwrites whatever the arena held, the classifier's range with zeros
    e.forward(*fwd_args())
    e.backward_pooled(BM.fixture_dp().cuda())
    arena = e.grads.clone()
    assert float(arena[classifier_tail(e):].abs().max()) == 0.0
    check_param_grads("butd maha pooled entry f32", e, arena, pg, classifier_zero=True)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_both_entries_after_one_forward(prec):
    """backward(dl, accumulate = 0) then backward_pooled(dp, accumulate = 1), what the autograd boundary issues when a loss reads both outputs:
    the gradient of sum(logits * dl) + sum(joint * dp); the classifier's range is that of backward(dl) alone, bit for bit.  bf16: the grouped
    (collecting) launches of the first call followed by the per-layer path of the second, finite and the classifier untouched."""
    dp = BM.fixture_dp()
    dl = torch.from_numpy(synth.uniform("g14.butd.dlogits", (B, NC), -1e-3, 1e-3))
    e = engine(prec)
    args = fwd_args()
    e.forward(*args)
    e.backward(dl.cuda())
    only_logits = e.grads.clone()
    e.forward(*args)
    e.backward(dl.cuda())
    e.backward_pooled(dp.cuda(), accumulate=True)
    both = e.grads.clone()
    t = classifier_tail(e)
    assert torch.equal(both[t:], only_logits[t:]) and float(only_logits[t:].abs().max()) > 0
    assert torch.isfinite(both).all() and not torch.equal(both[:t], only_logits[:t])
    if prec == "f32":
        _, _, _, _, pg = BM.autograd(torch.float64, dp=dp, dl=dl)
        check_param_grads("butd maha both entries f32", e, both, pg, classifier_zero=False)


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
def test_strided_dpooled(prec):
    """dpooled as a column slice of a wider tensor: ld = 1024 + 8 (the 16-byte path) and an odd ld from an odd first column (the scalar path) give
    the gradients of the dense call, bit for bit"""
    e = engine(prec)
    dp = BM.fixture_dp().cuda()
    args = fwd_args()
    out = []
    for pad, first in ((0, 0), (8, 0), (7, 3)):
        wide = torch.full((B, H + pad), 9.0, device="cuda")
        view = wide[:, first:first + H]
        view.copy_(dp)
        assert view.stride(0) == H + pad and (pad == 0 or not view.is_contiguous())
        df = torch.full((B * O, F), 7.0, device="cuda"); db = torch.full((B * O, PD), 7.0, device="cuda")
        e.set_input_grads(df, db)
        e.forward(*args)
        e.backward_pooled(view)
        e.set_input_grads(None, None)
        out.append((e.grads.clone(), df, db))
    for o in out[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, out[0]))
    assert float(out[0][0].abs().max()) > 0 and float(out[0][1].abs().max()) > 0


def test_errors():
    from rgqa_amd import _lib, scoring
    e = engine("f32")
    dp = BM.fixture_dp().cuda()
    with pytest.raises(RuntimeError, match="no forward pass recorded"):
        e.backward_pooled(dp)
    e.forward(*fwd_args())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(RuntimeError, match="ld"):
        _lib.check(e.lib.rgqa_engine_backward_pooled(e.h, _lib.ptr(dp), H - 8, 0, st))
    with pytest.raises(RuntimeError, match="null"):
        _lib.check(e.lib.rgqa_engine_backward_pooled(e.h, None, H, 0, st))
    e.backward_pooled(dp)                  # and the engine still works
    torch.cuda.synchronize()
    assert torch.isfinite(e.grads).all()
    # a plain GQABUTD returns no joint_repr
    m, _ = build_dropin("f32", maha=False)
    feat, pos = fwd_args()[:2]
    pack = fixture_pack()
    with pytest.raises(NotImplementedError, match="BUTD"):
        scoring.maha_scores(m, feat, pos, BUTD_SENTS, pack, NOISE)
    with pytest.raises(NotImplementedError, match="GQABUTD_maha"):
        scoring.maha_sample_estimator(m, [])


# ------------------------------------------------------------------------------------------------ 2. the drop-in class
def build_dropin(precision, maha=True):
    """GQABUTD_maha (or GQABUTD) over the G7 dictionary with the fixture's unit-gain weights, dropout=False as the reference's test scripts build it"""
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import butd.butd as DB
        from butd.preprocess import Dictionary
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))
    d = Dictionary()
    for w in BUTD_WORDS:
        d.add_word(w)
    _, filled, _, _, _ = BM.case()
    m = (DB.GQABUTD_maha if maha else DB.GQABUTD)(NC, d, dropout=False, precision=precision)
    assert set(m.state_dict()) == set(filled)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in filled.items()})
    return m.cuda(), filled


@functools.lru_cache(None)
def precision_f64():
    return synth.butd_maha_precision()


def fixture_pack():
    from rgqa_amd import scoring
    return scoring.maha_pack(BM.g14()["mean"], precision_f64())


def test_forward_returns_logits_and_joint_repr():
    """(logits, joint_repr), or (logits, att) with attention=True (butd/butd.py:466-469); the logits are GQABUTD's on the same weights"""
    m, filled = build_dropin("f32")
    plain, _ = build_dropin("f32", maha=False)
    feat, pos = fwd_args()[:2]
    m.train(); plain.train()
    with torch.no_grad():
        lg, x = m(feat, pos, BUTD_SENTS)
        lg2, att = m(feat, pos, BUTD_SENTS, attention=True)
        lp = plain(feat, pos, BUTD_SENTS)
    assert lg.shape == (B, NC) and x.shape == (B, H) and att.shape == (B, O, 1)
    assert torch.equal(lg, lg2) and torch.equal(lg, lp)
    ref = torch.from_numpy(BM.g14()["pooled"])
    err = float((x.cpu() - ref).abs().max())
    print("GQABUTD_maha f32: joint_repr vs the reference's: max err %.3e (max|ref| %.3f)" % (err, float(ref.abs().max())))
    assert err <= 2e-5 * max(1.0, float(ref.abs().max()))          # the bound the host restatement is held to (tests/test_butd_maha_oracle.py)
    with torch.enable_grad():
        lg3, x3 = m(feat, pos, BUTD_SENTS)
    assert lg3.grad_fn is not None and x3.grad_fn is lg3.grad_fn and torch.equal(x3.detach(), x)


def test_maha_scores_end_to_end_f32():
    """mirror of tests/test_gpu_maha.py test_maha_scores_end_to_end, in train() with dropout=False as gqa_maha.py:205-206 scores BUTD"""
    from rgqa_amd import scoring
    from tests.maha_reference import ood_batch
    g = BM.g14()
    mean, P = g["mean"], precision_f64()
    ref_err = float(g["ref_f32_err"])
    m, _ = build_dropin("f32")
    m.train()
    pack = fixture_pack()
    feat, pos = fwd_args()[:2]
    out = scoring.maha_scores(m, feat, pos, BUTD_SENTS, pack, NOISE)
    assert m.training
    hand = by_hand(m, feat, pos, BUTD_SENTS, pack, NOISE)
    for a, h, name in zip(out, hand[:5], scoring.MahaScores._fields):
        assert torch.equal(a, h), name
    assert torch.equal(out.feats_pt, torch.add(feat, (torch.ge(hand[5], 0).float() - 0.5) * 2, alpha=-NOISE))
    assert torch.equal(out.boxes_pt, torch.add(pos, (torch.ge(hand[6], 0).float() - 0.5) * 2, alpha=-NOISE))
    # the classifier got no gradient from the scoring pass, everything else did
    for k, p in m.named_parameters():
        assert p.grad is not None and (float(p.grad.abs().max()) == 0.0 or not k.startswith(BM.CLASSIFIER)), k
    assert float(dict(m.named_parameters())["w_emb.emb.weight"].grad.abs().max()) > 0
    # the f64 restatement's joint_repr on the returned perturbed inputs, scored in f64 at the device's label.  A joint_repr error e moves the score by
    # (P (x - mean))^T e in first order, at most |P (x - mean)|_1 max|e|; max|e| allowed: 8 x the f32 restatement's own error on these inputs
    fp, bp = out.feats_pt.cpu(), out.boxes_pt.cpu()
    xo = BM.joint_on(fp, bp, torch.float64).numpy()
    e32 = float(np.abs(BM.joint_on(fp, bp, torch.float32).numpy().astype(np.float64) - xo).max())
    tol_joint = MARGIN * e32
    lab = out.label.cpu().numpy()
    z = xo - mean[lab].astype(np.float64)
    Pz = z @ P
    s64 = -0.5 * (Pz * z).sum(1)
    allowed = MARGIN * ref_err + np.abs(Pz).sum(1) * tol_joint
    err = np.abs(out.score.cpu().numpy() - s64)
    perr = float(np.abs(out.pooled.cpu().numpy() - xo).max())
    print("maha_scores butd f32: f32 restatement vs f64 on the perturbed inputs %.3e (tol_joint %.3e); device joint_repr err %.3e; second-pass score vs f64: "
          "max err %.3e (allowed %.3e .. %.3e); labels %s (fixture %s)" % (e32, tol_joint, perr, err.max(), allowed.min(), allowed.max(), lab.tolist(), g["label2"].tolist()))
    assert bool((err <= allowed).all()), (err, allowed)
    assert np.array_equal(lab, score_f64(xo, mean, P).argmax(1)) and np.array_equal(lab, g["label2"])
    # the reference's unchanged statements through the same drop-in model
    ref = ood_batch(m, feat, pos, BUTD_SENTS, torch.from_numpy(mean).cuda(), torch.from_numpy(P).float().cuda(), NC, NOISE)
    assert torch.equal(ref["label2"], out.label)
    serr = (ref["score2"] - out.score).abs().cpu().numpy()
    print("maha_scores butd f32: the reference's statements through the drop-in: max score difference %.3e; labels %s first pass %s" % (
        serr.max(), ref["label2"].tolist(), ref["sample_pred"].tolist()))
    assert bool((serr <= allowed).all())
    assert np.array_equal(ref["label2"].cpu().numpy(), g["label2"]) and np.array_equal(ref["sample_pred"].cpu().numpy(), g["sample_pred"])
    # dropout=False: eval() computes the same bits
    m.eval()
    again = scoring.maha_scores(m, feat, pos, BUTD_SENTS, pack, NOISE)
    assert not m.training
    for a, h, name in zip(again, out, scoring.MahaScores._fields):
        assert torch.equal(a, h), name


@pytest.mark.parametrize("prec", ["bf16", "bf16x3", "bf16x3_fwd"])
def test_maha_scores_other_precisions(prec):
    from rgqa_amd import scoring
    g = BM.g14()
    m, _ = build_dropin(prec)
    m.train()
    pack = fixture_pack()
    feat, pos = fwd_args()[:2]
    out = scoring.maha_scores(m, feat, pos, BUTD_SENTS, pack, NOISE)
    assert m.training
    assert torch.isfinite(out.score).all() and torch.isfinite(out.pooled).all() and out.pooled.shape == (B, H)
    hand = by_hand(m, feat, pos, BUTD_SENTS, pack, NOISE)
    for a, h, name in zip(out, hand[:5], scoring.MahaScores._fields):
        assert torch.equal(a, h), (prec, name)
    perr = float((out.pooled.cpu() - torch.from_numpy(g["pooled2"])).abs().max())
    serr = float((out.score.cpu() - torch.from_numpy(g["score2"])).abs().max())
    print("maha_scores butd %s: labels %s (fixture %s); joint_repr vs the fixture's second pass: max diff %.3e; score max diff %.3e (min top-2 gap %.3e)" % (
        prec, out.label.tolist(), g["label2"].tolist(), perr, serr, float(np.diff(np.sort(g["noised_gaussian_score"], 1)[:, -2:], axis=1).min())))


def test_sample_estimator_through_the_dropin():
    from rgqa_amd import scoring
    m, _ = build_dropin("f32")
    m.train()
    target = synth.maha_targets("g14.butd.train", 3 * B)
    assert target.shape[1] == NC and bool(((target != 0).sum(1) > 1).any()) and bool(((target != 0).sum(0) == 0).any())
    batches = []
    for i in range(3):
        b = synth.synth_batch(B, 8, O=O, F=F, NA=NC, vocab=64, seed=606 + i, uq_frac=0.2)
        batches.append((torch.from_numpy(b["feats"]).cuda(), torch.from_numpy(b["boxes"]).cuda(), BUTD_SENTS, torch.from_numpy(target[i * B:(i + 1) * B]).cuda()))
    modes = []
    hook = m.register_forward_pre_hook(lambda mod, inp: modes.append(mod.training))
    try:
        pack = scoring.maha_sample_estimator(m, batches)
    finally:
        hook.remove()
    assert modes == [False] * 3 and m.training                  # it runs in eval() and restores the mode
    assert isinstance(pack, scoring.MahaPack) and pack.mean.shape == (NC, H) and pack.precision.shape == (H, H) and pack.nu.shape[0] == NC
    assert pack.W.shape[0] == H and 0 < pack.W.shape[1] <= 3 * B and torch.isfinite(pack.W).all()      # 15 rows: the covariance has rank < 15
    m.eval()
    with torch.no_grad():
        rows = [m(f, b, s)[1] for f, b, s, _ in batches]
    est = scoring.MahaEstimator(NC, H)
    for x, (_, _, _, t) in zip(rows, batches):
        est.update(x, t)
    n, sums, G = est.parts()
    rn, rs, rG = accumulate_numpy(torch.cat(rows).cpu().numpy(), target)
    es, eg = np.abs(sums - rs).max() / np.abs(rs).max(), np.abs(G - rG).max() / np.abs(rG).max()
    print("maha estimator butd: sums err %.2e, G err %.2e (relative to the largest entry; bound 1e-12)" % (es, eg))
    assert np.array_equal(n, rn) and es <= 1e-12 and eg <= 1e-12
    mean = rs / np.maximum(rn, 1.0)[:, None]
    assert float(np.abs(pack.mean.cpu().numpy() - mean).max()) <= 1e-6
    assert float(pack.mean[torch.from_numpy(rn == 0).cuda()].abs().max()) == 0.0


def test_maha_scores_runs_no_collective_in_train_mode(tmp_path, monkeypatch):
    """as tests/test_gpu_maha.py test_maha_scores_runs_no_collective_in_train_mode, for GQABUTD_maha in train() (how the reference scores BUTD)"""
    import torch.distributed as dist
    from rgqa_amd import scoring
    from rgqa_amd.lxrt import modeling as M
    monkeypatch.setenv("RGQA_DP_REHEARSAL", "1")
    m, _ = build_dropin("bf16x3_fwd")
    m.train()
    pack = fixture_pack()
    feat, pos = fwd_args()[:2]
    calls = []
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        for name in ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter", "barrier"):
            if hasattr(dist, name):
                monkeypatch.setattr(dist, name, (lambda n: lambda *a, **k: calls.append(n))(name))
        assert M._dp_exchanging()
        out = scoring.maha_scores(m, feat, pos, BUTD_SENTS, pack, NOISE)
        torch.cuda.synchronize()
        assert torch.isfinite(out.score).all() and out.pooled.shape == (B, H) and m.training
        assert calls == [] and m.__dict__.get("_dp_ex") is None
        assert M._SCORING_DEPTH == 0
    finally:
        dist.destroy_process_group()


def test_reference_batch_bf16x3_fwd(monkeypatch):
    """the reference's test batch (32, scripts/butd/test/maha.sh) at 36 regions and NC = 1842 in bf16x3_fwd precision with a synthetic pack at H = 1024:
    finite scores, and maha_scores is the by-hand composition bit for bit"""
    from rgqa_amd import scoring
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import maha_bench as MB
        import odin_bench as OB
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    monkeypatch.setenv("RGQA_PRECISION", "bf16x3_fwd")          # (make_model sets it as well: restored with the test)
    torch.manual_seed(0)
    m = MB.make_model("butd", "bf16x3_fwd")
    assert m.training and type(m).__name__ == "GQABUTD_maha"
    feats, boxes, sent = OB.make_batch("butd", 32)
    _, mean, P = synthetic(256, H=H)
    pack = scoring.maha_pack(mean, P)
    out = scoring.maha_scores(m, feats, boxes, sent, pack, NOISE)
    assert out.score.shape == (32,) and out.pooled.shape == (32, H) and torch.isfinite(out.score).all() and bool((out.label >= 0).all()) and bool((out.label < 1842).all())
    hand = by_hand(m, feats, boxes, sent, pack, NOISE)
    for a, h, name in zip(out, hand[:5], scoring.MahaScores._fields):
        assert torch.equal(a, h), name
    assert float((out.feats_pt - feats).abs().max()) > 0
