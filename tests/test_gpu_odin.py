"""ODIN scoring on every backbone (tasks/gqa_odin.py:97-131): dL/dfeats and dL/dboxes of the BUTD engine and of the UNITER front end
through the C ABI (rgqa_engine_set_input_grads), the two device operators (rgqa_odin_dlogits, rgqa_sign_step), the unchanged reference
statements through the drop-in classes, and scoring.odin_scores end to end.

At temperature 1e5 the reference's column (first maximum among tied f32 sigmoid values) and target (preds >= 0.5 at the last bit of 0.5)
flip with logit differences far below any tolerance, so no test here compares a device-chosen column or target with a reference-chosen one,
and every gradient test feeds both sides the SAME dlogits (tests/test_input_grads_oracle.py odin_dlogits_from)."""
import contextlib
import functools
import os
import sys
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from rgqa_amd import synth                                           # noqa: E402
from rgqa_amd.synth import BUTD_WORDS, BUTD_SENTS, U_SMALL            # noqa: E402
from tests.test_input_grads_oracle import (g12, odin_dlogits_from, butd_g7_inputs, butd_oracle_input_grads, uniter_case,     # noqa: E402
                                           uniter_oracle_input_grads, check_against_g12)
from tests.test_gpu_dropin import env                                # noqa: E402,F401  (fixture: the small LXMERT drop-in model)

# 3 * gtol * max|ref|, gtol as tests/test_gpu_butd.py:37,62 and tests/test_gpu_butd_x3fwd.py:37 hold sampled gradient entries of this engine to
BUTD_GTOL = {"f32": 3e-3, "bf16x3": 3e-3, "bf16": 6e-2, "bf16x3_fwd": 6e-2}
# tests/test_gpu_engine.py test_input_gradients_vs_golden / test_input_gradients_bf16x3_vs_f32_engine: the same kernels
UNITER_TOL = {"f32": 2e-4, "bf16x3": 1e-3, "bf16": 6e-2, "bf16x3_fwd": 6e-2}
SIGN_MASK = 0.01          # above every error bound of f32 / bf16x3 here (at most 3 * 3e-3 = 9e-3 of max|ref|)


# ------------------------------------------------------------------------------------------------ engines and references
def butd_engine(prec, filled, NT, NA, B, L, O):
    from rgqa_amd.engine import Engine
    e = Engine(arch=1, vocab_size=NT + 1, hidden=1024, emb_dim=300, feat_dim=2048, pos_dim=4, num_answers=NA, precision=prec,
               hidden_dropout=0.0, attn_dropout=0.0, heads=1, inter=8, l_layers=0, x_layers=0, r_layers=0).allocate("cuda")
    assert {sp.name for sp in e.specs} == set(filled)
    for sp in e.specs:
        e.view(e.params, sp).copy_(torch.from_numpy(np.asarray(filled[sp.name]).reshape(sp.shape)))
    e.ensure_shape(B, L, O)
    e.sync_weights()
    return e


def engine_input_grads(e, fwd, dl, rows, F, Pd, **kw):
    """backward without input gradients, then twice with them: (dfeats, dboxes) after checking the bit-identity conditions"""
    fwd_args = fwd
    e.forward(*fwd_args, **kw)
    e.backward(dl)
    g0 = e.grads.clone()
    runs = []
    for _ in range(2):
        df = torch.full((rows, F), 7.0, device="cuda")
        db = torch.full((rows, Pd), 7.0, device="cuda")
        e.set_input_grads(df, db)
        e.forward(*fwd_args, **kw)
        e.backward(dl)
        e.set_input_grads(None, None)
        runs.append((df, db, e.grads.clone()))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][2], g0), "parameter gradients changed by asking for input gradients"
    assert torch.equal(runs[1][2], g0) and torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1]), "second run differs from the first"
    # and back: with the pointers cleared nothing is written any more
    e.forward(*fwd_args, **kw)
    e.backward(dl)
    assert torch.equal(e.grads, g0)
    return runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()


@functools.lru_cache(None)
def butd_g7_ref():
    """G7 batch: dlogits from the fixture's column / target / logits, the oracle's gradients in f64"""
    g = g12(os.path.join(ROOT, "tests", "golden"))
    c, filled, feat, pos, toks = butd_g7_inputs()
    dl = odin_dlogits_from(g["butd_g7.logits"], g["butd_g7.col"], g["butd_g7.y"])
    _, df, db = butd_oracle_input_grads(c, filled, feat, pos, toks, dl, torch.float64)
    return filled, feat, pos, toks, dl, df.numpy().reshape(-1, 2048), db.numpy().reshape(-1, 4)


@functools.lru_cache(None)
def butd_b256_ref():
    """config-5 size: the oracle's own f64 logits choose column and target (torch statements), its f64 autograd gives the reference"""
    from oracle import butd_ref as BR
    from tests.test_oracle_golden import butd_fill
    B, L, NA, NT = 256, 40, 1842, 3000
    c = BR.ButdConfig(ntoken=NT, num_answers=NA)
    filled = butd_fill(c)
    b = synth.synth_batch(B, L, seed=515, uq_frac=0.25, vocab=NT)
    rng = np.random.RandomState(3)
    toks = np.full((B, L), NT, dtype=np.int64)
    for r in range(B):
        n = int(rng.randint(1, L + 1)) if r else L
        toks[r, L - n:] = rng.randint(0, NT, size=n)
    feat, pos, toks = torch.from_numpy(b["feats"]), torch.from_numpy(b["boxes"]), torch.from_numpy(toks)
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    P = {k: torch.from_numpy(np.asarray(v)).double() for k, v in filled.items()}
    f, p = feat.double().requires_grad_(True), pos.double().requires_grad_(True)
    lg = BR.butd_forward(P, c, f, p, toks)
    z = lg.detach().float()
    preds = torch.sigmoid(z / 1e5)
    col = torch.max(preds, 1)[1]
    y = (preds >= 0.5).float().gather(1, col.unsqueeze(1)).squeeze(1)
    dl = odin_dlogits_from(z, col, y)
    lg.backward(dl.double())
    return filled, feat, pos, toks, dl, f.grad.numpy().reshape(-1, 2048), p.grad.numpy().reshape(-1, 4)


@functools.lru_cache(None)
def uniter_ref(tag, T):
    """dlogits from the fixture's column / target / logits; the f32 oracle's gradients for them"""
    g = g12(os.path.join(ROOT, "tests", "golden"))
    case = "uniter_%s_T%d" % (tag, T)
    cfgd, raw = uniter_case(tag, T)
    dl = odin_dlogits_from(g[case + ".logits"], g[case + ".col"], g[case + ".y"])
    _, df, dp = uniter_oracle_input_grads(cfgd, raw, dl)
    return cfgd, raw, dl, df.numpy().reshape(-1, cfgd["feat_dim"]), dp.numpy().reshape(-1, 7)


def uniter_engine_grads(tag, T, prec, packed):
    from tests.test_uniter import make_engine, dev
    cfgd, raw, dl, rf, rp = uniter_ref(tag, T)
    b = dev(raw)
    B, O = raw["feats"].shape[:2]
    lens = [int(v) for v in raw["input_mask"].sum(1)] if packed else None
    e = make_engine(cfgd, prec)
    e.ensure_shape(B, T, O)
    e.sync_weights()
    df, dp = engine_input_grads(e, (b["feats"], b["pos7"], b["input_ids"], b["input_mask"], b["segment_ids"]), dl.cuda(), B * O, cfgd["feat_dim"], 7, lengths=lens)
    return df, dp, rf, rp


def rel_errors(tag, got_f, got_b, ref_f, ref_b, tol):
    assert np.abs(ref_f).max() > 0 and np.abs(ref_b).max() > 0
    ef = np.abs(got_f - ref_f).max() / np.abs(ref_f).max()
    eb = np.abs(got_b - ref_b).max() / np.abs(ref_b).max()
    print("%s: dfeats err / max|ref| %.3e, dboxes err / max|ref| %.3e (bound %.1e; max|ref| %.2e / %.2e)" % (tag, ef, eb, tol, np.abs(ref_f).max(), np.abs(ref_b).max()))
    return ef, eb


def sign_agreement(tag, got, ref, gate):
    got, ref = torch.from_numpy(np.ascontiguousarray(got)), torch.from_numpy(np.ascontiguousarray(ref)).float()
    mask = ref.abs() > SIGN_MASK * ref.abs().max()
    kept = float(mask.float().mean())
    agree = torch.ge(got, 0)[mask] == torch.ge(ref, 0)[mask]
    share_all = float((torch.ge(got, 0) == torch.ge(ref, 0)).float().mean())
    print("%s: sign agreement inside the mask %.6f (mask keeps %.1f %% of the elements), over all elements %.6f" % (tag, float(agree.float().mean()), 100 * kept, share_all))
    assert kept >= 0.90, (tag, kept)
    if gate:
        assert bool(agree.all()), (tag, int((~agree).sum()))


# ------------------------------------------------------------------------------------------------ 1. BUTD
@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16", "bf16x3_fwd"])
def test_butd_input_gradients_g7_vs_f64_oracle(prec):
    """Observed on MI355X (dfeats / dboxes, error / max|ref|): see docs/MEASUREMENTS.md "ODIN input gradients"."""
    filled, feat, pos, toks, dl, rf, rb = butd_g7_ref()
    e = butd_engine(prec, filled, len(BUTD_WORDS), 23, 5, 40, 36)
    kg = toks.cuda()
    df, db = engine_input_grads(e, (feat.cuda(), pos.cuda(), kg, kg, None), dl.cuda(), 5 * 36, 2048, 4)
    tol = 3 * BUTD_GTOL[prec]
    ef, eb = rel_errors("butd G7 %s" % prec, df, db, rf, rb, tol)
    sign_agreement("butd G7 %s dfeats" % prec, df, rf, gate=prec in ("f32", "bf16x3"))
    sign_agreement("butd G7 %s dboxes" % prec, db, rb, gate=prec in ("f32", "bf16x3"))
    assert ef <= tol and eb <= tol, (prec, ef, eb)
    if prec == "f32":       # and against the reference's own autograd (samples, norm, boxes in full)
        check_against_g12(g12(os.path.join(ROOT, "tests", "golden")), "butd_g7", df.reshape(5, 36, 2048), db.reshape(5, 36, 4), tol, "engine f32")


@pytest.mark.parametrize("prec", ["bf16", "bf16x3_fwd"])
def test_butd_input_gradients_at_config5_size(prec):
    """B = 256, L = 40: the M = 9216 dgrad GEMM path"""
    filled, feat, pos, toks, dl, rf, rb = butd_b256_ref()
    e = butd_engine(prec, filled, 3000, 1842, 256, 40, 36)
    kg = toks.cuda()
    df, db = engine_input_grads(e, (feat.cuda(), pos.cuda(), kg, kg, None), dl.cuda(), 256 * 36, 2048, 4)
    tol = 3 * BUTD_GTOL[prec]
    ef, eb = rel_errors("butd B=256 %s" % prec, df, db, rf, rb, tol)
    sign_agreement("butd B=256 %s dfeats" % prec, df, rf, gate=False)
    assert ef <= tol and eb <= tol, (prec, ef, eb)


def test_butd_only_one_of_the_two_buffers():
    """either pointer may be NULL: the other gradient is the one the full call gives"""
    filled, feat, pos, toks, dl, rf, rb = butd_g7_ref()
    e = butd_engine("bf16x3", filled, len(BUTD_WORDS), 23, 5, 40, 36)
    kg, fg, pg, dg = toks.cuda(), feat.cuda(), pos.cuda(), dl.cuda()
    out = {}
    for which in ("both", "feats", "boxes"):
        df = torch.full((180, 2048), 7.0, device="cuda") if which != "boxes" else None
        db = torch.full((180, 4), 7.0, device="cuda") if which != "feats" else None
        e.set_input_grads(df, db)
        e.forward(fg, pg, kg, kg, None)
        e.backward(dg)
        e.set_input_grads(None, None)
        out[which] = (df, db)
    assert torch.equal(out["feats"][0], out["both"][0]) and torch.equal(out["boxes"][1], out["both"][1])


# ------------------------------------------------------------------------------------------------ 2. UNITER
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("T", [5, 8])
def test_uniter_input_gradients_small_vs_reference(golden_dir, T, packed):
    df, dp, rf, rp = uniter_engine_grads("small", T, "f32", packed)
    B, O = 3, 6
    check_against_g12(g12(golden_dir), "uniter_small_T%d" % T, df.reshape(B, O, -1), dp.reshape(B, O, 7), UNITER_TOL["f32"], "engine f32 packed=%s" % packed)
    if T == 8:
        sign_agreement("uniter small T8 f32 packed=%s dfeats" % packed, df, rf, gate=True)
        sign_agreement("uniter small T8 f32 packed=%s dpos" % packed, dp, rp, gate=True)


# (sign agreement in bf16x3 is gated on the full config below: the split-f32 engine needs head size 64 and cannot be built at the small one)
@pytest.mark.parametrize("prec,packed", [("f32", False), ("f32", True), ("bf16x3", True), ("bf16x3", False), ("bf16", True), ("bf16", False), ("bf16x3_fwd", True),
                                         ("bf16x3_fwd", False)])
def test_uniter_input_gradients_full_vs_f32_oracle(prec, packed):
    df, dp, rf, rp = uniter_engine_grads("full", 20, prec, packed)
    tol = UNITER_TOL[prec]
    ef, eb = rel_errors("uniter full T20 %s packed=%s" % (prec, packed), df, dp, rf, rp, tol)
    gate = prec in ("f32", "bf16x3")
    sign_agreement("uniter full T20 %s packed=%s dfeats" % (prec, packed), df, rf, gate)
    sign_agreement("uniter full T20 %s packed=%s dpos" % (prec, packed), dp, rp, gate)
    assert ef <= tol and eb <= tol, (prec, packed, ef, eb)


# ------------------------------------------------------------------------------------------------ 5. operators
def _torch_odin_statements(z, label, max_score):
    """gqa_odin.py:103-110 on the host for the given column and the given value of preds at it: (d loss / d logits, loss)"""
    z = z.clone().requires_grad_(True)
    B = z.shape[0]
    labels = torch.zeros_like(z)
    labels[torch.arange(B), label] = (max_score >= 0.5).float()
    loss = torch.nn.BCEWithLogitsLoss(reduction="none")(z, labels)
    loss = torch.mean(torch.gather(loss, 1, label.unsqueeze(-1)))
    loss.backward()
    return z.grad, loss.detach()


def _odin_logits(B, NA, seed):
    rng = np.random.RandomState(seed)
    z = rng.uniform(-8.0, 4.0, size=(B, NA)).astype(np.float32)
    z[0] = rng.uniform(-1e-3, 1e-3, size=NA)                    # every sigmoid(z / 1e5) is exactly 0.5: all tied
    z[1] = rng.uniform(-9.0, -5.0, size=NA); z[1, NA // 3] = -0.005     # the chosen logit lies in (-0.012, 0): preds = 0.5 exactly, target 1
    z[2] = rng.uniform(-9.0, -5.0, size=NA); z[2, NA - 1] = -0.009
    z[3] = rng.uniform(-9.0, -5.0, size=NA); z[3, 0] = -3.0     # clearly below 0.5: target 0
    z[4, 5] = 30.0                                              # saturated
    return z


@pytest.mark.parametrize("NA", [23, 1842])
@pytest.mark.parametrize("T", [1e5, 1.0])
def test_odin_dlogits_vs_torch_statements(NA, T):
    from rgqa_amd import scoring, _lib
    B = 9
    ld = NA + 13
    full = torch.full((B, ld), 99.0)
    full[:, :NA] = torch.from_numpy(_odin_logits(B, NA, 7 + NA))
    zg = full.cuda()[:, :NA]                                    # row stride > NA
    s = scoring.score_rows(zg, T)
    dl, loss = scoring.odin_dlogits(zg, s.label, s.max_score)
    z = zg.cpu().contiguous()                                   # the same logits, copied from the device
    label, ms = s.label.cpu(), s.max_score.cpu()
    ref, ref_loss = _torch_odin_statements(z, label, ms)
    got = dl.cpu()
    r = torch.arange(B)
    print("odin_dlogits NA=%d T=%g: labels %s targets %s chosen-entry max rel err %.2e loss rel err %.2e" % (
        NA, T, label.tolist(), (ms >= 0.5).int().tolist(), float(((got[r, label] - ref[r, label]).abs() / ref[r, label].abs().clamp_min(1e-30)).max()),
        abs(loss.item() - ref_loss.item()) / abs(ref_loss.item())))
    np.testing.assert_allclose(got[r, label].numpy(), ref[r, label].numpy(), rtol=1e-4, atol=1e-7)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-5)
    other = got.clone()
    other[r, label] = 0.0
    assert float(other.abs().max()) == 0.0 and not torch.signbit(other).any()
    if T == 1e5:
        # rows 1 and 2: the f32 sigmoid of the chosen (negative) logit is exactly 0.5, so the reference's target is 1 and the gradient is negative
        preds = torch.sigmoid(z / T)
        assert label[1] == NA // 3 and label[2] == NA - 1 and float(preds[1, NA // 3]) == 0.5 and float(preds[2, NA - 1]) == 0.5
        assert float(got[1, NA // 3]) < 0 and float(got[2, NA - 1]) < 0 and float(got[3, label[3]]) > 0
        assert float(ms[0]) == 0.5 and float(got[0, label[0]]) < 0        # the all-tied row: target 1
    # padded columns through the C ABI: NAp = round_up(NA, 64) columns are written (exact zeros past NA), nothing beyond them
    NAp = (NA + 63) // 64 * 64
    buf = torch.full((B, NAp + 5), 7.0, device="cuda")
    lo = torch.zeros(1, device="cuda")
    p = _lib.ptr
    import ctypes as C
    _lib.check(_lib.load().rgqa_odin_dlogits(p(zg), zg.stride(0), p(s.label), p(s.max_score), B, NA, NAp, p(buf), buf.stride(0), p(lo),
                                             C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    assert torch.equal(buf[:, :NA], dl) and float(buf[:, NA:NAp].abs().max()) == 0.0 and bool((buf[:, NAp:] == 7.0).all()) and torch.equal(lo, loss)
    dl2, loss2 = scoring.odin_dlogits(zg, s.label, s.max_score)
    assert torch.equal(dl2, dl) and torch.equal(loss2, loss)


def test_odin_column_is_torch_max_when_no_two_sigmoids_tie():
    from rgqa_amd import scoring
    B, NA = 6, 1842
    rng = np.random.RandomState(5)
    z = np.stack([rng.permutation(np.linspace(-6.0, 6.0, NA)) for _ in range(B)]).astype(np.float32)
    zt = torch.from_numpy(z)
    preds = torch.sigmoid(zt / 1.0)
    assert all(len(np.unique(preds[b].numpy())) == NA for b in range(B))
    s = scoring.score_rows(zt.cuda(), 1.0)
    assert torch.equal(s.label.cpu(), torch.max(preds, 1)[1])
    dl, _ = scoring.odin_dlogits(zt.cuda(), s.label, s.max_score)
    assert torch.equal((dl != 0).sum(1).cpu(), torch.ones(B, dtype=torch.long)) and torch.equal(dl.abs().argmax(1).cpu(), torch.max(preds, 1)[1])


def test_odin_operators_reject_bad_arguments():
    from rgqa_amd import scoring
    z = torch.zeros(3, 8, device="cuda")
    s = scoring.score_rows(z, 1.0)
    with pytest.raises(ValueError):
        scoring.odin_dlogits(z, s.label.int(), s.max_score)
    with pytest.raises(ValueError):
        scoring.odin_dlogits(z, s.label[:2], s.max_score[:2])
    with pytest.raises(ValueError):
        scoring.sign_step(z, z[:, :4], 0.1)
    # a label outside [0, NA) writes nothing out of bounds: the row is all zeros
    bad = s.label.clone(); bad[1] = 8
    dl, _ = scoring.odin_dlogits(z, bad, s.max_score)
    assert float(dl[1].abs().max()) == 0.0 and float(dl[0].abs().max()) > 0


@pytest.mark.parametrize("n", [1, 7, 1027, 5 * 36 * 2048])
def test_sign_step_is_the_torch_statements_bit_for_bit(n):
    from rgqa_amd import scoring
    rng = np.random.RandomState(n)
    x = torch.from_numpy(rng.uniform(-3, 3, size=n + 1).astype(np.float32))
    g = torch.from_numpy((rng.standard_normal(n + 1) * 1e-9).astype(np.float32))
    special = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1e-45, -1e-45]
    for i, v in enumerate(special[:n]):
        g[i] = v
    noise = 1e-4
    for off in (0, 1):                      # off = 1: a 4-byte aligned start (the scalar path)
        xs, gs = x[off:off + n].clone(), g[off:off + n].clone()
        ref = torch.add(xs, (torch.ge(gs, 0).float() - 0.5) * 2, alpha=-noise)
        xd, gd = x.cuda()[off:off + n], g.cuda()[off:off + n]
        out = scoring.sign_step(xd, gd, noise)
        assert torch.equal(out.cpu(), ref)
        buf = x.cuda().clone()
        xin = buf[off:off + n]
        r = scoring.sign_step(xin, gd, noise, out=xin)      # in place
        assert r.data_ptr() == xin.data_ptr() and torch.equal(xin.cpu(), ref)
        if off == 0:
            assert float(buf[n]) == float(x[n])             # nothing past n is touched
    if n >= 3:
        xs = x[:n]
        ref = torch.add(xs, (torch.ge(g[:n], 0).float() - 0.5) * 2, alpha=-noise)
        assert ref[0] == xs[0] - noise and ref[1] == xs[1] - noise and ref[2] == xs[2] + noise       # 0, -0.0 step by -noise; NaN by +noise


# ------------------------------------------------------------------------------------------------ drop-in classes
def build_butd(precision):
    from tests.test_gpu_butd import build
    return build(precision, dropout=False)


@contextlib.contextmanager
def uniter_dropin(golden_dir, monkeypatch, precision="f32"):
    """GQAUNITER at the small size, as tests/test_uniter.py test_dropin_gqauniter_matches_oracle builds it"""
    from oracle import lxmert_ref as R
    from oracle import uniter_ref as U
    monkeypatch.setenv("RGQA_BERT_VOCAB", os.path.join(golden_dir, "g4_vocab.txt"))
    monkeypatch.setenv("RGQA_PRECISION", precision)
    monkeypatch.setenv("RGQA_UNITER_ANY_ROIS", "1")
    sys.path.insert(0, os.path.join(ROOT, "dropin"))
    try:
        import rgqa_amd.uniter.modeling as M
        cfgd = dict(U_SMALL, vocab_size=80, max_pos=64)
        monkeypatch.setattr(M.VISUAL_CONFIG, "visual_feat_dim", cfgd["feat_dim"])
        monkeypatch.setattr(M.UniterFeatureExtraction, "from_pretrained", classmethod(
            lambda cls, name, **kw: cls(M.BertConfig(cfgd["vocab_size"], hidden_size=cfgd["hidden"], num_hidden_layers=cfgd["l_layers"],
                                                     num_attention_heads=cfgd["heads"], intermediate_size=cfgd["inter"],
                                                     max_position_embeddings=cfgd["max_pos"], hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0), **kw)))
        from uniter.uniter import GQAUNITER
        m = GQAUNITER(cfgd["num_answers"], model_args=types.SimpleNamespace(from_scratch=False))
        filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
        m = m.cuda().eval()
        sents = ["What color is the dog?", "is it", "who is holding the red bottle on the left side of the table near the window today"]
        raw = synth.uniter_batch(cfgd, 20, 3, 6, 55)
        ids, mask, _ = R.sents_to_features(sents, 20, m.encoder.tokenizer.vocab)

        def oracle_logits(feats, pos7):
            P = {k: torch.from_numpy(v.copy()) for k, v in filled.items()}
            with torch.no_grad():
                return U.gqa_forward(P, R.RefConfig(**cfgd), feats, pos7, torch.tensor(ids), torch.tensor(mask))[0]
        yield m, sents, torch.from_numpy(raw["feats"]), torch.from_numpy(raw["pos7"]), oracle_logits
    finally:
        sys.path.remove(os.path.join(ROOT, "dropin"))


def reference_odin_statements(model, feats, boxes, sent, temperature):
    """tasks/gqa_odin.py:97-112, unchanged but for the device the constants are made on"""
    from torch.autograd import Variable
    bceloss = torch.nn.BCEWithLogitsLoss(reduction="none")
    feats, boxes = Variable(feats, requires_grad=True), Variable(boxes, requires_grad=True)
    logit = model(feats, boxes, sent)
    preds = torch.sigmoid(logit / temperature)
    labels = torch.ones(preds.shape).cuda() * (preds >= 0.5)
    labels = Variable(labels.float())
    loss = bceloss(logit, labels)
    idx = torch.max(preds, dim=1)[1].unsqueeze(-1)
    loss = torch.mean(torch.gather(loss, 1, idx))
    loss.backward()
    return feats, boxes, logit.detach(), idx.squeeze(-1), torch.gather(labels, 1, idx).squeeze(-1)


def _dlogits_on_device(logit, col, y):
    B = logit.shape[0]
    d = torch.zeros_like(logit)
    r = torch.arange(B, device=logit.device)
    d[r, col] = (torch.sigmoid(logit[r, col]) - y) / B
    return d


def test_reference_statements_through_gqabutd():
    """GQABUTD in train() with dropout=False (tasks/gqa_odin.py:87-88): feats.grad / boxes.grad are populated and are what the engine-level call gives
    for the dlogits autograd handed the boundary"""
    m, c, filled = build_butd("f32")
    m.train()
    _, _, feat, pos, _ = butd_g7_inputs()
    f, b, logit, col, y = reference_odin_statements(m, feat.cuda(), pos.cuda(), BUTD_SENTS, 1e5)
    assert f.grad is not None and b.grad is not None and f.grad.shape == f.shape and b.grad.shape == b.shape
    assert float(f.grad.abs().max()) > 0 and float(b.grad.abs().max()) > 0
    pg = {k: p.grad.clone() for k, p in m.named_parameters()}
    assert all(v is not None for v in pg.values())                 # the parameters' .grad hold the scoring pass's gradients
    # the engine-level call on the same module's engine: autograd's dlogits for these statements are (sigmoid(z) - y) / B at the chosen column
    e = m._binding.engine
    toks = m.tokenize(BUTD_SENTS).cuda()
    lg = e.forward(feat.cuda(), pos.cuda(), toks, toks, None, train=True)[0].clone()
    assert torch.equal(lg, logit)
    captured = {}
    f2 = feat.cuda().requires_grad_(True)
    l2 = m(f2, pos.cuda(), BUTD_SENTS)
    l2.register_hook(lambda gr: captured.setdefault("dl", gr.clone()))
    preds = torch.sigmoid(l2 / 1e5)
    labels = (torch.ones(preds.shape).cuda() * (preds >= 0.5)).float()
    idx = torch.max(preds, dim=1)[1].unsqueeze(-1)
    torch.mean(torch.gather(torch.nn.BCEWithLogitsLoss(reduction="none")(l2, labels), 1, idx)).backward()
    df = torch.empty(5 * 36, 2048, device="cuda"); db = torch.empty(5 * 36, 4, device="cuda")
    e.set_input_grads(df, db)
    e.forward(feat.cuda(), pos.cuda(), toks, toks, None, train=True)
    e.backward(captured["dl"])
    e.set_input_grads(None, None)
    assert torch.equal(df.view(5, 36, 2048), f.grad) and torch.equal(db.view(5, 36, 4), b.grad)
    np.testing.assert_allclose(captured["dl"].cpu().numpy(), _dlogits_on_device(logit, col, y).cpu().numpy(), rtol=1e-5, atol=1e-9)


def test_reference_statements_through_gqauniter(golden_dir, monkeypatch):
    with uniter_dropin(golden_dir, monkeypatch) as (m, sents, feats, pos7, _):
        f, b, logit, col, y = reference_odin_statements(m, feats.cuda(), pos7.cuda(), sents, 1e5)
        assert f.grad is not None and b.grad is not None and f.grad.shape == f.shape and b.grad.shape == b.shape
        assert float(f.grad.abs().max()) > 0 and float(b.grad.abs().max()) > 0
        captured = {}
        f2 = feats.cuda().requires_grad_(True)
        l2 = m(f2, pos7.cuda(), sents)
        l2.register_hook(lambda gr: captured.setdefault("dl", gr.clone()))
        preds = torch.sigmoid(l2 / 1e5)
        labels = (torch.ones(preds.shape).cuda() * (preds >= 0.5)).float()
        idx = torch.max(preds, dim=1)[1].unsqueeze(-1)
        torch.mean(torch.gather(torch.nn.BCEWithLogitsLoss(reduction="none")(l2, labels), 1, idx)).backward()
        e = m.encoder.model._binding.engine
        ids, seg, mask, lens = m.encoder._prepare(sents, feats.cuda(), pos7.cuda())
        B, O = feats.shape[:2]
        df = torch.empty(B * O, feats.shape[2], device="cuda"); db = torch.empty(B * O, 7, device="cuda")
        e.set_input_grads(df, db)
        lg = e.forward(feats.cuda(), pos7.cuda(), ids, mask, seg, train=False, lengths=lens)[0].clone()
        e.backward(captured["dl"])
        e.set_input_grads(None, None)
        assert torch.equal(lg, logit)
        assert torch.equal(df.view(f.shape), f.grad) and torch.equal(db.view(b.shape), b.grad)


# ------------------------------------------------------------------------------------------------ 7. end to end
def _by_hand(model, feats, boxes, sent, temperature, noise):
    from rgqa_amd import scoring
    f, b = feats.clone().requires_grad_(True), boxes.clone().requires_grad_(True)
    logit = model(f, b, sent)
    s = scoring.score_rows(logit.detach(), temperature)
    dl, _ = scoring.odin_dlogits(logit.detach(), s.label, s.max_score)
    logit.backward(dl)
    fp, bp = scoring.sign_step(feats, f.grad, noise), scoring.sign_step(boxes, b.grad, noise)
    with torch.no_grad():
        l2 = model(fp, bp, sent)
    s2 = scoring.score_rows(l2, temperature)
    return s2.max_score, s2.label, l2, fp, bp, f.grad, b.grad


def _check_end_to_end(tag, model, feats, boxes, sent, temperature, noise, oracle_logits, tol):
    from rgqa_amd import scoring
    out = scoring.odin_scores(model, feats, boxes, sent, temperature, noise)
    hand = _by_hand(model, feats, boxes, sent, temperature, noise)
    for a, h, name in zip(out, hand[:5], scoring.OdinScores._fields):
        assert torch.equal(a, h), (tag, name)
    assert out.feats_pt.shape == feats.shape and out.boxes_pt.shape == boxes.shape
    # every element moved by exactly one step of +-noise against the sign of its gradient
    assert torch.equal(out.feats_pt, torch.add(feats, (torch.ge(hand[5], 0).float() - 0.5) * 2, alpha=-noise))
    assert torch.equal(out.boxes_pt, torch.add(boxes, (torch.ge(hand[6], 0).float() - 0.5) * 2, alpha=-noise))
    ref = oracle_logits(out.feats_pt.cpu(), out.boxes_pt.cpu())
    err = float((out.logits.cpu() - ref).abs().max())
    print("odin_scores %s T=%g: second-pass logits vs the oracle on the perturbed inputs: max err %.3e (bound %.1e); labels %s" % (tag, temperature, err, tol, out.label.tolist()))
    assert err <= tol, (tag, err)
    # the oracle, given the device's column on its own logits for the perturbed inputs, scores within what that logits error allows
    r = torch.arange(ref.shape[0])
    so = torch.sigmoid(ref[r, out.label.cpu()] / temperature)
    assert float((so - out.score.cpu()).abs().max()) <= tol / temperature * 0.25 + 1e-6


@pytest.mark.parametrize("temperature", [1e5, 1.0])
def test_odin_scores_butd(temperature):
    from oracle import butd_ref as BR
    m, c, filled = build_butd("f32")
    m.train()                                   # as the reference scores BUTD
    _, _, feat, pos, toks = butd_g7_inputs()
    P = {k: torch.from_numpy(np.asarray(v)) for k, v in filled.items()}

    def oracle_logits(f, p):
        with torch.no_grad():
            return BR.butd_forward(P, c, f, p, toks)
    _check_end_to_end("butd", m, feat.cuda(), pos.cuda(), BUTD_SENTS, temperature, 1e-4, oracle_logits, 2e-4)      # tests/test_gpu_butd.py:37 (f32)


@pytest.mark.parametrize("temperature", [1e5, 1.0])
def test_odin_scores_uniter(golden_dir, monkeypatch, temperature):
    with uniter_dropin(golden_dir, monkeypatch) as (m, sents, feats, pos7, oracle_logits):
        _check_end_to_end("uniter", m, feats.cuda(), pos7.cuda(), sents, temperature, 1e-4, oracle_logits, 1e-4)   # tests/test_uniter.py:202 (f32)


@pytest.mark.parametrize("temperature", [1e5, 1.0])
def test_odin_scores_lxmert(env, golden_dir, temperature):      # noqa: F811
    from oracle import lxmert_ref as R
    from tests.test_gpu_dropin import build, batch, SENTS, CFG
    T = 20
    m, filled = build("f32", T)
    m.eval()
    feats, boxes, _ = batch(T)
    vocab = {w.rstrip("\n"): i for i, w in enumerate(open(os.path.join(golden_dir, "g4_vocab.txt"), encoding="utf-8"))}
    ids, mask, _ = R.sents_to_features(SENTS, T, vocab)
    P = {k: torch.from_numpy(v.copy()) for k, v in filled.items()}

    def oracle_logits(f, b):
        with torch.no_grad():
            return R.gqa_forward(P, R.RefConfig(**CFG), f, b, torch.tensor(ids), torch.tensor(mask))[0]
    _check_end_to_end("lxmert", m, feats.cuda(), boxes.cuda(), SENTS, temperature, 1e-4, oracle_logits, 1e-4)      # tests/test_gpu_dropin.py (f32 logits: 1e-4)


# ------------------------------------------------------------------------------------------------ 8. no collective
def test_odin_scores_runs_no_collective_in_train_mode(tmp_path, monkeypatch):
    """Under an initialised process group with RGQA_DP_REHEARSAL=1 a training backward exchanges gradients; odin_scores on GQABUTD in train()
    (how the reference scores BUTD) must not: no collective is issued and no exchange object is made."""
    import torch.distributed as dist
    from rgqa_amd import scoring
    from rgqa_amd.lxrt import modeling as M
    monkeypatch.setenv("RGQA_DP_REHEARSAL", "1")
    m, c, filled = build_butd("bf16x3_fwd")
    m.train()
    _, _, feat, pos, _ = butd_g7_inputs()
    calls = []
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "rendezvous"), rank=0, world_size=1)
    try:
        for name in ("all_reduce", "reduce_scatter_tensor", "all_gather_into_tensor", "all_gather", "broadcast", "reduce_scatter", "barrier"):
            if hasattr(dist, name):
                monkeypatch.setattr(dist, name, (lambda n: lambda *a, **k: calls.append(n))(name))
        assert M._dp_exchanging()
        out = scoring.odin_scores(m, feat.cuda(), pos.cuda(), BUTD_SENTS, 1e5, 1e-4)
        torch.cuda.synchronize()
        assert torch.isfinite(out.score).all() and out.logits.shape == (5, 23)
        assert calls == [] and m.__dict__.get("_dp_ex") is None
        assert M._SCORING_DEPTH == 0
    finally:
        dist.destroy_process_group()
