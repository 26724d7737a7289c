"""The confidence-branch model on the device (reference tasks/gqa_model_branched.py, tasks/gqa_branched.py): the stand-alone loss operator
(rgqa_amd/csrc/branched_loss.hip) against the reference statements (tests/branched_reference.py: torch on the CPU in f64, and in f32 for the bound), the
engine with rgqa_config.conf_branch = 1 against the fixture of the reference's own GQAModel_branched (tests/golden/g15_branched.npz) and against f64
restatements, its bit-level conditions, and the drop-in GQAModel_branched with scoring.branched_finetune_loss / branched_scores.

Accuracy bound of the operator (loss, loss_ce, loss_conf: relative; conf, score1: absolute; dlogits, dconf: relative to their largest magnitude): the device's
deviation from the f64 evaluation is at most MARGIN = 8 x the deviation of the statements' own f32 CPU evaluation from f64 on the same inputs - the
project's margin (tests/test_gpu_energy_loss.py), for the other summation order over up to 1842 terms and the hardware exp behind the shared sigmoid.

Tolerances of the f32 engine against f64 at the full head width (hidden 768: rows of 1536, K = 768): those of the f32 engine against the fixture
(conf logit 1e-4 absolute; gradients rtol 2e-3, atol 1e-6 + 2e-4 max|ref|) - the same arithmetic with sums 12 / 24 times longer, whose f32 rounding grows
with the square root of the length (< 5x) from a level three orders below these gates."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from rgqa_amd import synth
from tests import branched_reference as BR
from tests.test_gpu_energy_loss import MARGIN, SHAPES

pytestmark = pytest.mark.gpu


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ operator
@functools.lru_cache(None)
def case(B, NA, mce, uq="third"):
    """inputs and the f64 / f32 evaluations of the reference statements on the CPU (computed once, shared, left unchanged)"""
    z, c, t = BR.draw(B, NA, 2000 + 7 * B + NA + (1 if mce else 0), uq=uq)
    return dict(z=z, c=c, t=t, r64=BR.evaluate(z, c, t, mce, torch.float64), r32=BR.evaluate(z, c, t, mce, torch.float32))


def run_op(z, c, t, mce, NAp=None, ldd=None, grad_scale=1.0):
    """rgqa_op_branched_loss through the C ABI on device tensors: z [B, NA] (any row stride), c [B], t [B, NA + 1].  dlogits live in a buffer of B * ldd + 8
    floats filled with 7: guard columns NAp .. ldd and 8 guard words behind the last row; every [B] output has 2 guard words."""
    from rgqa_amd import _lib
    lib = _lib.load()
    B, NA = z.shape
    NAp = NAp or NA
    ldd = ldd or NAp
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_branched_loss_scratch_floats(B, C.byref(n)))
    scratch = torch.full((n.value + 8,), 5.0, device="cuda")
    buf = torch.full((B * ldd + 8,), 7.0, device="cuda")
    loss = torch.full((5,), 9.0, device="cuda")
    dc, cf, s1 = (torch.full((B + 2,), 9.0, device="cuda") for _ in range(3))
    lab = torch.full((B + 2,), -5, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    _lib.check(lib.rgqa_op_branched_loss(p(z), z.stride(0), p(c), p(t), t.stride(0), B, NA, NAp, 1 if mce else 0, grad_scale, p(loss), p(buf), ldd, p(dc), p(cf),
                                         p(lab), p(s1), p(scratch), _stream()))
    torch.cuda.synchronize()
    full = buf[:B * ldd].view(B, ldd)
    assert bool((scratch[n.value:] == 5.0).all()) and bool((loss[3:] == 9.0).all()) and bool((lab[B:] == -5).all()), "guard words overwritten"
    assert all(bool((v[B:] == 9.0).all()) for v in (dc, cf, s1)), "guard words overwritten"
    assert bool((buf[B * ldd:] == 7.0).all()) and bool((full[:, NAp:] == 7.0).all()), "dlogits written past NAp / past the last row"
    return dict(loss=loss[:3].clone(), dl=full[:, :NA].clone(), pad=full[:, NA:NAp].clone(), dconf=dc[:B].clone(), conf=cf[:B].clone(), score1=s1[:B].clone(),
                label=lab[:B].clone())


def on_device(c, layout):
    """'padded' = contiguous logits, dlogits with ldd = NAp = round_up(NA, 64); 'strided' = logits rows 13 floats apart from contiguous (row starts at odd
    words), ldd = NAp + 5"""
    z, t = c["z"], c["t"]
    B, NA = z.shape
    NAp = (NA + 63) // 64 * 64
    if layout == "padded":
        return z.cuda(), c["c"].cuda(), t.cuda(), NAp, NAp
    wide = torch.full((B, NA + 13), 99.0)
    wide[:, :NA] = z
    return wide.cuda()[:, :NA], c["c"].cuda(), t.cuda(), NAp, NAp + 5


def deviations(got, r64):
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    relmax = lambda a, b: float((a.double() - b).abs().max() / b.abs().max())
    out = dict(loss_conf=rel(got["loss_conf"], r64["loss_conf"]), conf=float((got["conf"].double() - r64["conf"]).abs().max()),
               score1=float((got["score1"].double() - r64["score1"]).abs().max()), dconf=relmax(got["dconf"], r64["dconf"]))
    if float(r64["dlogits"].abs().max()) > 0:
        out["dlogits"] = relmax(got["dlogits"], r64["dlogits"])
    if not torch.isnan(r64["loss"]):
        out["loss"], out["loss_ce"] = rel(got["loss"], r64["loss"]), rel(got["loss_ce"], r64["loss_ce"])
    return out


def check_bound(tag, dev, r32, r64):
    got = dict(loss=dev["loss"][0].cpu(), loss_ce=dev["loss"][1].cpu(), loss_conf=dev["loss"][2].cpu(), conf=dev["conf"].cpu(), score1=dev["score1"].cpu(),
               dlogits=dev["dl"].cpu(), dconf=dev["dconf"].cpu())
    d, r = deviations(got, r64), deviations(r32, r64)
    print("%s: device / f32-reference deviation from f64: %s" % (tag, "  ".join("%s %.2e / %.2e" % (k, d[k], r[k]) for k in d)))
    for k in d:
        assert d[k] <= MARGIN * r[k], (tag, k, d[k], r[k])


@pytest.mark.parametrize("layout", ["padded", "strided"])
@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA", SHAPES)
def test_operator_against_the_reference_statements(B, NA, mce, layout):
    c = case(B, NA, mce)
    uq = c["t"][:, -1] != 0
    assert int(uq.sum()) >= 1 and int((~uq).sum()) >= 1 and float(c["c"].abs().max()) <= 8.0
    z, cl, t, NAp, ldd = on_device(c, layout)
    dev = run_op(z, cl, t, mce, NAp, ldd)
    check_bound("B=%d NA=%d %s %s" % (B, NA, "mce" if mce else "bce", layout), dev, c["r32"], c["r64"])
    # label: torch's on the device's logits copied to the CPU, wherever the two largest logits of a row are apart
    top = z.cpu().topk(2, dim=1).values
    apart = top[:, 0] - top[:, 1] > 1e-6
    assert int(apart.sum()) >= B - 1
    assert torch.equal(dev["label"].cpu()[apart], z.cpu().max(1)[1][apart])
    # unanswerable rows and padded columns: exact (positive) zeros
    for blk in (dev["dl"][uq.cuda()], dev["pad"]):
        assert blk.numel() > 0 and bool((blk == 0).all()) and not bool(torch.signbit(blk).any())
    assert float(dev["dl"][(~uq).cuda()].abs().min()) > 0 or mce


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA", SHAPES)
def test_operator_bit_level_conditions(B, NA, mce):
    c = case(B, NA, mce)
    zp, cp, tp, NAp, lddp = on_device(c, "padded")
    zs, cs, ts, _, ldds = on_device(c, "strided")
    a, b, s = run_op(zp, cp, tp, mce, NAp, lddp), run_op(zp, cp, tp, mce, NAp, lddp), run_op(zs, cs, ts, mce, NAp, ldds)
    for k in ("loss", "dl", "dconf", "conf", "score1", "label"):
        assert torch.equal(a[k], b[k]), "two runs differ in %s" % k
        assert torch.equal(a[k], s[k]), "%s depends on the operands' alignment" % k
    h = run_op(zs, cs, ts, mce, NAp, ldds, grad_scale=0.5)
    assert torch.equal(h["dl"], a["dl"] * 0.5) and torch.equal(h["dconf"], a["dconf"] * 0.5) and torch.equal(h["loss"], a["loss"]) and float(a["dl"].abs().max()) > 0


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
def test_operator_empty_answerable_subset_follows_torch(mce):
    """B = 4, NA = 67, no answerable row: loss_ce (and the loss) NaN as the statements' are, gradients finite: dlogits exact zeros, dconf within the bound"""
    c = case(4, 67, mce, "all")
    assert torch.isnan(c["r64"]["loss_ce"]) and torch.isfinite(c["r64"]["dconf"]).all() and float(c["r64"]["dlogits"].abs().max()) == 0
    z, cl, t, NAp, ldd = on_device(c, "padded")
    dev = run_op(z, cl, t, mce, NAp, ldd)
    assert bool(torch.isnan(dev["loss"][0])) and bool(torch.isnan(dev["loss"][1])) and bool(torch.isfinite(dev["loss"][2]))
    assert bool((dev["dl"] == 0).all()) and bool(torch.isfinite(dev["dconf"]).all())
    check_bound("B=4 NA=67 %s no answerable row" % ("mce" if mce else "bce"), dev, c["r32"], c["r64"])


def test_python_wrapper_is_the_operator():
    from rgqa_amd import scoring
    c = case(7, 300, False)
    z, cl, t, NAp, ldd = on_device(c, "strided")
    dev = run_op(z, cl, t, False, NAp, ldd)
    r = scoring.branched_loss_rows(z, cl.view(-1, 1), t)
    assert isinstance(r, scoring.BranchedLoss)
    assert torch.equal(torch.stack([r.loss, r.loss_ce, r.loss_conf]), dev["loss"]) and torch.equal(r.dlogits, dev["dl"]) and torch.equal(r.dconf, dev["dconf"])
    assert torch.equal(r.conf, dev["conf"]) and torch.equal(r.label, dev["label"]) and torch.equal(r.score1, dev["score1"])
    with pytest.raises(ValueError):
        scoring.branched_loss_rows(z, cl, t[:, :-1])
    with pytest.raises(ValueError):
        scoring.branched_loss_rows(z, cl[:-1], t)


# ------------------------------------------------------------------------------------------------ engine
def make_engine(cfgd, precision, conf_branch=True):
    from rgqa_amd.engine import Engine
    e = Engine(precision=precision, hidden_dropout=0.0, attn_dropout=0.0, conf_branch=conf_branch, **cfgd).allocate("cuda")
    for sp in e.specs:
        e.view(e.params, sp).copy_(torch.from_numpy(synth.fill_value(sp.name, sp.shape)))
    return e


def dev_batch(b):
    return {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}


def fwd(e, b):
    return e.forward(b["feats"], b["boxes"], b["input_ids"], b["input_mask"], b["segment_ids"])


def conf_range(e):
    a = min(sp.offset for sp in e.specs if sp.name.startswith("conf_fc."))
    return a, e.arena_elems


def fixture_grad(g, form, name, numel):
    """(reference values, index into the flattened tensor or None = whole)"""
    return g["%s.grad.%s" % (form, name)], BR.fixture_index(form, name, numel)


@pytest.mark.parametrize("form", ["bce", "mce"])
def test_f32_small_vs_fixture(golden_dir, form):
    """the f32 engine against the reference's own GQAModel_branched: the tolerances of tests/test_gpu_engine.py::test_f32_small_vs_golden"""
    g = np.load(os.path.join(golden_dir, "g15_branched.npz"))
    e = make_engine(synth.SMALL, "f32")
    b = dev_batch(synth.small_batch(8))
    e.ensure_shape(3, 8, 6)
    e.sync_weights()
    lg, _ = fwd(e, b)
    np.testing.assert_allclose(lg.cpu().numpy(), g["logits"], rtol=0, atol=1e-4)
    np.testing.assert_allclose(e.conf_logit.cpu().numpy(), g["conf"].reshape(-1), rtol=0, atol=1e-4)
    t = torch.from_numpy(g["target_with_uq"]).cuda()
    assert np.array_equal(g["target_with_uq"], synth.branched_target())
    loss, conf, label = e.branched_loss_backward(t, mce=form == "mce")
    parts = e.branched_loss_parts.cpu().numpy()
    for k, v in zip(("loss", "loss_ce", "loss_conf"), parts):
        np.testing.assert_allclose(v, g[form + "." + k], rtol=1e-5, err_msg=k)
    assert torch.equal(label.cpu(), torch.from_numpy(g["logits"]).max(1)[1])
    np.testing.assert_allclose(conf.cpu().numpy(), 1.0 / (1.0 + np.exp(-g["conf"].reshape(-1).astype(np.float64))), rtol=1e-5)
    dead = set(g["dead"].tolist())
    seen = 0
    for sp in e.specs:
        got = e.view(e.grads, sp).cpu().numpy()
        if sp.name in dead:
            assert sp.dead and float(np.abs(got).max()) == 0.0
            continue
        ref, idx = fixture_grad(g, form, sp.name, sp.numel)
        if idx is not None:
            got = got.reshape(-1)[idx]
        np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-6 + 2e-4 * np.abs(ref).max(), err_msg=sp.name)
        seen += 1
    assert seen > 100 and all(float(np.abs(g["%s.grad.%s" % (form, k)]).max()) > 0 for k in BR.CONF_KEYS)


def test_x3fwd_medium_vs_f64_restatement():
    """bf16x3_fwd at the sizes the existing bf16x3_fwd tests build (MED, B = 6, T = 12, O = 10) against the oracle's encoder + the restated conf head and
    trainer statements in f64: the logit bound and the per-tensor gradient gate of tests/test_gpu_engine.py::test_medium_config_vs_oracle (imported), the
    conf logit held to the logits' bound"""
    from oracle import lxmert_ref as R
    from tests import test_gpu_engine as TE
    tol, gtol = {p: (a, b) for p, a, b in TE.test_medium_config_vs_oracle.pytestmark[0].args[1]}["bf16x3_fwd"]
    MED, (B, T, O) = TE.MED, (6, 12, 10)
    raw = synth.synth_batch(B, T, O=O, F=MED["feat_dim"], NA=MED["num_answers"], vocab=MED["vocab_size"], seed=5, min_len=2)
    e = make_engine(MED, "bf16x3_fwd")
    cfg = R.RefConfig(**MED)
    P = {sp.name: torch.from_numpy(synth.fill_value(sp.name, sp.shape)).double().requires_grad_(True) for sp in e.specs}
    tt = {k: torch.from_numpy(v) for k, v in raw.items() if k != "lengths"}
    lg_r, pl_r = R.gqa_forward({k: v for k, v in P.items() if not k.startswith("conf_fc.")}, cfg, tt["feats"].double(), tt["boxes"].double(), tt["input_ids"],
                               tt["input_mask"], tt["segment_ids"])
    cf_r = BR.conf_head(pl_r, P)
    tuq = torch.zeros(B, MED["num_answers"] + 1)
    tuq[:, :-1] = tt["target"]
    tuq[1] = 0.0
    tuq[1, -1] = 1.0
    BR.trainer_statements(lg_r, cf_r, tuq.double())[0].backward()
    d = dev_batch(raw)
    e.ensure_shape(B, T, O)
    e.sync_weights()
    lg, _ = fwd(e, d)
    lerr, cerr = float((lg.cpu().double() - lg_r.detach()).abs().max()), float((e.conf_logit.cpu().double() - cf_r.detach().reshape(-1)).abs().max())
    print("bf16x3_fwd medium: logits %.2e conf %.2e (bound %.1e)" % (lerr, cerr, tol))
    assert lerr < tol and cerr < tol
    e.branched_loss_backward(tuq.cuda())
    worst = 0.0
    for sp in e.specs:
        got, ref = e.view(e.grads, sp).cpu().double(), P[sp.name].grad
        if ref is None or sp.dead:
            assert float(got.abs().max()) == 0.0, sp.name
            continue
        den = float(ref.norm())
        if den < 1e-8:
            continue
        err = float((got - ref).norm()) / den
        worst = max(worst, err)
        assert err < gtol, (sp.name, err)
    print("bf16x3_fwd medium: worst tensor %.2e (gate %.1e)" % (worst, gtol))


WIDE = dict(vocab_size=64, hidden=768, heads=12, inter=256, max_pos=32, type_vocab=2, l_layers=1, x_layers=1, r_layers=1, feat_dim=32, pos_dim=4, num_answers=67)


@pytest.mark.parametrize("B", [5, 70, 300])
def test_full_head_width_f32_vs_f64(B):
    """hidden 768: the 1536-wide row kernels, with B = 70 the column sums over more than 64 rows and with B = 300 the bias sum over more rows than a workgroup
    has threads; conf logit and the six conf_fc gradients against f64
    from the engine's own pooled output"""
    T, O = 6, 4
    raw = synth.synth_batch(B, T, O=O, F=WIDE["feat_dim"], NA=WIDE["num_answers"], vocab=WIDE["vocab_size"], seed=31, min_len=2)
    e = make_engine(WIDE, "f32")
    e.ensure_shape(B, T, O)
    e.sync_weights()
    _, pooled = fwd(e, dev_batch(raw))
    w = {sp.name: torch.from_numpy(synth.fill_value(sp.name, sp.shape)).double().requires_grad_(True) for sp in e.specs if sp.name in BR.CONF_KEYS}
    cf = BR.conf_head(pooled.cpu().double(), w).reshape(-1)
    np.testing.assert_allclose(e.conf_logit.cpu().numpy(), cf.detach().numpy(), rtol=0, atol=1e-4)
    assert float(cf.detach().abs().max()) > 1e-3
    dconf = torch.from_numpy(synth.uniform("wide.dconf%d" % B, (B,), -1.0, 1.0))
    (cf * dconf.double()).sum().backward()
    e.backward(None, dconf=dconf.cuda())
    for sp in e.specs:
        if sp.name in BR.CONF_KEYS:
            got, ref = e.view(e.grads, sp).cpu().numpy(), w[sp.name].grad.numpy()
            assert float(np.abs(ref).max()) > 0
            np.testing.assert_allclose(got, ref, rtol=2e-3, atol=1e-6 + 2e-4 * np.abs(ref).max(), err_msg=sp.name)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_engine_bit_level_conditions(prec):
    from rgqa_amd import scoring
    b = dev_batch(synth.small_batch(8))
    t = torch.from_numpy(synth.branched_target()).cuda()
    in_shapes = ((3 * 6, synth.SMALL["feat_dim"]), (3 * 6, 4))
    e = make_engine(synth.SMALL, prec)
    c0, c1 = conf_range(e)
    e.ensure_shape(3, 8, 6)
    e.sync_weights()
    lg = fwd(e, b)[0].clone()
    r = scoring.branched_loss_rows(lg, e.conf_logit, t)
    # branched_loss_backward = backward(dlogits, dconf) with the operator's outputs; its loss / conf / label are the operator's
    loss, conf, label = e.branched_loss_backward(t)
    g1 = e.grads.clone()
    assert torch.equal(e.branched_loss_parts, torch.stack([r.loss, r.loss_ce, r.loss_conf])) and torch.equal(conf, r.conf) and torch.equal(label, r.label)
    assert bool(torch.isfinite(g1).all()) and float(g1[:c0].abs().max()) > 0 and float(g1[c0:].abs().max()) > 0
    fwd(e, b)
    e.backward(r.dlogits, dconf=r.dconf)
    assert torch.equal(e.grads, g1), "branched_loss_backward is not backward(the operator's dlogits, dconf)"
    # two runs are bit-identical
    fwd(e, b)
    e.branched_loss_backward(t)
    assert torch.equal(e.grads, g1)
    # input-gradient buffers change no parameter gradient
    df, db = torch.full(in_shapes[0], 7.0, device="cuda"), torch.full(in_shapes[1], 7.0, device="cuda")
    e.set_input_grads(df, db)
    fwd(e, b)
    e.branched_loss_backward(t)
    e.set_input_grads(None, None)
    torch.cuda.synchronize()
    assert torch.equal(e.grads, g1), "parameter gradients changed by asking for input gradients"
    assert bool(torch.isfinite(df).all()) and float(df.abs().max()) > 0 and not bool((df == 7.0).all()) and not bool((db == 7.0).all())
    # grad_scale and accumulate go the way the energy head's do
    fwd(e, b)
    e.backward(r.dlogits * 0.5, dconf=r.dconf * 0.5)
    g_half = e.grads.clone()
    fwd(e, b)
    e.branched_loss_backward(t, grad_scale=0.5)
    assert torch.equal(e.grads, g_half)
    e.backward(r.dlogits * 0.5, dconf=r.dconf * 0.5, accumulate=True)
    g_acc = e.grads.clone()
    fwd(e, b)
    e.branched_loss_backward(t, grad_scale=0.5)
    e.branched_loss_backward(t, grad_scale=0.5, accumulate=True)
    assert torch.equal(e.grads, g_acc) and not torch.equal(g_acc, g_half)
    # either gradient alone; both together is their sum's pass, not two passes
    fwd(e, b)
    e.backward(r.dlogits)
    g_l = e.grads.clone()
    e.backward(None, dconf=r.dconf)
    g_c = e.grads.clone()
    assert float(g_l[c0:].abs().max()) == 0 and float(g_c[c0:].abs().max()) > 0 and float(g_c[:c0].abs().max()) > 0
    # conf_only: every element outside the six tensors exactly 0, the six have the full pass's bits
    fwd(e, b)
    e.branched_loss_backward(t, conf_only=True)
    assert float(e.grads[:c0].abs().max()) == 0.0 and torch.equal(e.grads[c0:], g1[c0:])
    assert torch.equal(e.branched_loss_parts, torch.stack([r.loss, r.loss_ce, r.loss_conf]))
    e.backward_conf_only(r.dconf)
    assert float(e.grads[:c0].abs().max()) == 0.0 and torch.equal(e.grads[c0:], g1[c0:])
    # ... also with no answerable row
    t_all = t.clone()
    t_all[:, :-1] = 0
    t_all[:, -1] = 1
    e.branched_loss_backward(t_all, conf_only=True)
    assert bool(torch.isnan(e.branched_loss_parts[1])) and bool(torch.isfinite(e.grads).all()) and float(e.grads[c0:].abs().max()) > 0
    with pytest.raises(ValueError):
        e.branched_loss_backward(t[:, :-1])


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_zero_conf_projection_leaves_the_plain_engines_gradients(prec):
    """conf_fc.3.weight = 0: nothing flows from the conf head into the pooler - the gradient arena outside conf_fc has the bits of a plain engine's
    backward(dlogits) with the same weights and the operator's dlogits; conf_fc.3's own gradients are not zero"""
    from rgqa_amd import scoring
    b = dev_batch(synth.small_batch(8))
    t = torch.from_numpy(synth.branched_target()).cuda()
    eb, ep = make_engine(synth.SMALL, prec), make_engine(synth.SMALL, prec, conf_branch=False)
    for e in (eb, ep):
        e.ensure_shape(3, 8, 6)
    w3 = next(sp for sp in eb.specs if sp.name == "conf_fc.3.weight")
    eb.view(eb.params, w3).zero_()
    eb.sync_weights()
    ep.sync_weights()
    lg_b, lg_p = fwd(eb, b)[0].clone(), fwd(ep, b)[0].clone()
    assert torch.equal(lg_b, lg_p)
    r = scoring.branched_loss_rows(lg_b, eb.conf_logit, t)
    eb.branched_loss_backward(t)
    ep.backward(r.dlogits)
    for sp in ep.specs:
        assert torch.equal(eb.view(eb.grads, sp), ep.view(ep.grads, sp)), sp.name
    for k in ("conf_fc.3.weight", "conf_fc.3.bias"):
        assert float(eb.view(eb.grads, next(sp for sp in eb.specs if sp.name == k)).abs().max()) > 0
    for k in ("conf_fc.0.weight", "conf_fc.0.bias", "conf_fc.2.weight", "conf_fc.2.bias"):
        assert float(eb.view(eb.grads, next(sp for sp in eb.specs if sp.name == k)).abs().max()) == 0


def test_parameter_table_and_coverage():
    from rgqa_amd.engine import Engine
    ep, eb = Engine(precision="bf16", **synth.SMALL), Engine(precision="bf16", conf_branch=True, **synth.SMALL)
    e0 = Engine(precision="bf16", conf_branch=False, **synth.SMALL)
    key = lambda e: [(sp.name, sp.offset, sp.shape, sp.linear, sp.dead, sp.f32_read) for sp in e.specs]
    assert key(e0) == key(ep) and e0.arena_elems == ep.arena_elems and not any(sp.name.startswith("conf") for sp in ep.specs)
    assert key(eb)[:len(ep.specs)] == key(ep)
    H = synth.SMALL["hidden"]
    extra = {sp.name: sp for sp in eb.specs[len(ep.specs):]}
    assert [sp.name for sp in eb.specs[len(ep.specs):]] == list(BR.CONF_KEYS)
    assert [extra[k].shape for k in BR.CONF_KEYS] == [(2 * H, H), (2 * H,), (2 * H,), (2 * H,), (1, 2 * H), (1,)]
    assert extra["conf_fc.0.weight"].linear and not extra["conf_fc.0.weight"].f32_read and extra["conf_fc.3.weight"].f32_read
    for arch in (1, 2):
        with pytest.raises(RuntimeError, match="conf"):
            Engine(precision="bf16", conf_branch=True, arch=arch, **dict(synth.U_SMALL if arch == 2 else synth.SMALL))
    # the six tensors lie inside a gradient segment and a live range
    eb.allocate("cuda")
    segs, live = eb.grad_segments(), eb.live_ranges()
    for sp in extra.values():
        assert any(a <= sp.offset and sp.offset + sp.numel <= z for a, z, _ in segs), sp.name
        assert any(a <= sp.offset and sp.offset + sp.numel <= z for a, z in live), sp.name
    for sp in eb.specs:
        eb.view(eb.params, sp).copy_(torch.from_numpy(synth.fill_value(sp.name, sp.shape)))
    b = dev_batch(synth.small_batch(8))
    eb.ensure_shape(3, 8, 6)
    eb.sync_weights()
    eb.enable_segment_sumsq(True)
    fwd(eb, b)
    eb.branched_loss_backward(torch.from_numpy(synth.branched_target()).cuda())
    want = float(sum(float((eb.grads[a:z].double() ** 2).sum()) for a, z in live) ** 0.5)
    assert abs(float(eb.grad_norm()) - want) <= 1e-6 * want
    assert abs(float(eb._seg_sumsq.double().sum()) ** 0.5 - want) <= 1e-5 * want            # the shares backward left, conf_fc's among them
    w0 = extra["conf_fc.0.weight"]
    before = eb.view(eb.params, w0).clone()
    eb.adam_step(1e-3)
    torch.cuda.synchronize()
    assert not torch.equal(eb.view(eb.params, w0), before)


# ------------------------------------------------------------------------------------------------ drop-in
from tests.test_gpu_dropin import env                                # noqa: E402,F401  (fixture: the small LXMERT drop-in model)


def build_branched(precision, T=20):
    import types
    from tasks.gqa_model_branched import GQAModel_branched
    from tests.test_gpu_dropin import CFG
    os.environ["RGQA_PRECISION"] = precision
    args = types.SimpleNamespace(llayers=CFG["l_layers"], xlayers=CFG["x_layers"], rlayers=CFG["r_layers"], from_scratch=False)
    m = GQAModel_branched(CFG["num_answers"], max_seq_length=T, model_args=args)
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return m.cuda(), filled


def count_backwards(eng, monkeypatch):
    calls = []
    for name in ("backward", "backward_pooled", "backward_conf_only", "loss_backward", "branched_loss_backward"):
        orig = getattr(eng, name)
        monkeypatch.setattr(eng, name, (lambda o, n: lambda *a, **k: (calls.append(n), o(*a, **k))[1])(orig, name))
    return calls


def uq_target(target, rows):
    t = torch.zeros(target.shape[0], target.shape[1] + 1)
    t[:, :-1] = target
    for b in rows:
        t[b] = 0.0
        t[b, -1] = 1.0
    return t


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
def test_branched_trainer_statements_through_the_dropin_model(env, mce, monkeypatch):      # noqa: F811
    """the reference's own statements over (logit, conf) and scoring.branched_finetune_loss give the same arena within the operator's bound; exactly one
    engine backward per step; clip_grad_norm_ stays on the arena path; BertAdam steps conf_fc"""
    from rgqa_amd import scoring
    from tests.test_gpu_dropin import batch, SENTS
    import tasks.gqa_model_branched as GB
    assert GB.MAX_GQA_LENGTH == 20
    m, filled = build_branched("f32")
    assert set(m.state_dict().keys()) == set(filled.keys()) and all(k in filled for k in BR.CONF_KEYS)
    m.eval()
    feats, boxes, target = batch(20)
    tuq = uq_target(target, {1, 4}).cuda()
    eng = m.lxrt_encoder.model._binding.engine
    calls = count_backwards(eng, monkeypatch)
    # the trainer's statements (gqa_branched.py:126-143)
    logit, conf = m(feats.cuda(), boxes.cuda(), SENTS)
    assert logit.shape == (len(SENTS), 17) and conf.shape == (len(SENTS), 1) and logit.requires_grad and conf.requires_grad
    loss_t = BR.trainer_statements(logit, conf, tuq, mce)[0]
    loss_t.backward()
    assert calls == ["backward"], calls
    g_t = eng.grads.clone()
    named = dict(m.named_parameters())
    for sp in eng.specs:
        if not sp.dead:
            assert torch.equal(named[sp.name].grad, eng.view(g_t, sp)), sp.name
    # the fused loss
    m.zero_grad()
    del calls[:]
    logit, conf = m(feats.cuda(), boxes.cuda(), SENTS)
    lg, cf = logit.detach().clone(), conf.detach().clone()
    loss, loss_ce, loss_conf, sconf, label = scoring.branched_finetune_loss(logit, conf, tuq, mce_loss=mce)
    assert loss.dim() == 0 and loss.requires_grad and not sconf.requires_grad and label.dtype == torch.int64
    loss.backward()
    assert calls == ["backward"], calls
    g_f = eng.grads.clone()
    l2, c2, lab2 = eng.branched_loss_backward(tuq, mce=mce)                 # engine-direct, on the forward the model recorded
    assert torch.equal(eng.grads, g_f) and torch.equal(l2[0], loss.detach()) and torch.equal(c2, sconf) and torch.equal(lab2, label)
    # the loss within the operator's bound; the two arenas come out of the same (linear) backward pass from gradients that differ by the operator's
    # deviation from torch's f32 statements, a few 1e-7 of their largest magnitude: held to the f32 engine's gradient gates (rtol 2e-3, atol 1e-6 + 2e-4 max|ref|)
    r64, r32 = BR.evaluate(lg.cpu(), cf.cpu(), tuq.cpu(), mce, torch.float64), BR.evaluate(lg.cpu(), cf.cpu(), tuq.cpu(), mce, torch.float32)
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    d, r = rel(loss.detach().cpu(), r64["loss"]), rel(r32["loss"], r64["loss"])
    print("drop-in %s: loss %.7f, device / f32-reference deviation from f64: %.2e / %.2e" % ("mce" if mce else "bce", float(loss.detach()), d, r))
    assert d <= MARGIN * r, (d, r)
    for sp in eng.specs:
        if not sp.dead:
            a, b = eng.view(g_t, sp).cpu().numpy(), eng.view(g_f, sp).cpu().numpy()
            np.testing.assert_allclose(a, b, rtol=2e-3, atol=1e-6 + 2e-4 * np.abs(b).max(), err_msg=sp.name)
    assert torch.equal(label.cpu(), lg.cpu().max(1)[1])
    # clip on the arena path, and the step moves conf_fc
    hits = []
    orig = type(eng).clip_grads_
    monkeypatch.setattr(type(eng), "clip_grads_", lambda self, *a, **k: (hits.append(1), orig(self, *a, **k))[1])
    from lxrt.optimization import BertAdam
    optim = BertAdam(list(m.parameters()), lr=1e-3)
    before = {k: named[k].detach().clone() for k in ("conf_fc.0.weight", "conf_fc.3.bias", "logit_fc.3.bias")}
    torch.nn.utils.clip_grad_norm_(m.parameters(), 5.)
    assert hits == [1], "clip_grad_norm_ left the arena path"
    optim.step()
    torch.cuda.synchronize()
    for k, v in before.items():
        assert not torch.equal(named[k].detach(), v), k


def test_frozen_answer_branch_takes_the_conf_only_path(env, monkeypatch):      # noqa: F811
    """--freeze_vqa_branch as the reference does it (gqa_branched.py:80-83): the trainer's statements run the engine's conf_only pass; frozen parameters keep
    .grad None and a constant-rate BertAdam step leaves them bit-identical (no weight decay), conf_fc moves"""
    from tests.test_gpu_dropin import batch, SENTS
    m, _ = build_branched("f32")
    for name, param in m.named_parameters():
        if not name.startswith('conf'):
            param.requires_grad = False
    m.train()
    feats, boxes, target = batch(20)
    tuq = uq_target(target, {1, 4}).cuda()
    eng = m.lxrt_encoder.model._binding.engine
    calls = count_backwards(eng, monkeypatch)
    from lxrt.optimization import BertAdam
    optim = BertAdam(list(m.parameters()), lr=1e-3)
    optim.zero_grad()
    logit, conf = m(feats.cuda(), boxes.cuda(), SENTS)
    BR.trainer_statements(logit, conf, tuq)[0].backward()
    assert calls == ["backward_conf_only"], calls
    named = dict(m.named_parameters())
    c0, _ = conf_range(eng)
    assert float(eng.grads[:c0].abs().max()) == 0.0
    before = {k: v.detach().clone() for k, v in named.items()}
    for k, p in named.items():
        assert (p.grad is None) == (not k.startswith("conf")), k
    torch.nn.utils.clip_grad_norm_(m.parameters(), 5.)
    optim.step()
    torch.cuda.synchronize()
    for k, p in named.items():
        assert torch.equal(p.detach(), before[k]) == (not k.startswith("conf")), k
    # the next forward sees the stepped conf_fc and the unchanged answer branch
    with torch.no_grad():
        logit2, conf2 = m(feats.cuda(), boxes.cuda(), SENTS)
    assert torch.equal(logit2, logit.detach()) and not torch.equal(conf2, conf.detach())


def test_loading_a_plain_gqa_model_and_scoring(env):      # noqa: F811
    from rgqa_amd import scoring
    from tests.test_gpu_dropin import build, batch, SENTS
    plain, _ = build("f32")
    sd = {k: v.detach().cpu().clone() for k, v in plain.state_dict().items()}
    m, filled = build_branched("f32")
    init = {k: torch.from_numpy(filled[k]) for k in BR.CONF_KEYS}
    for v in sd.values():
        v.mul_(1.5)
    res = m.load_state_dict(sd, strict=False)
    assert sorted(res.missing_keys) == sorted(BR.CONF_KEYS) and not res.unexpected_keys
    now = m.state_dict()
    assert all(torch.equal(now[k].cpu(), init[k]) for k in BR.CONF_KEYS) and all(torch.equal(now[k].cpu(), sd[k]) for k in sd)
    m.eval()
    feats, boxes, _ = batch(20)
    with torch.no_grad():
        logit, conf = m(feats.cuda(), boxes.cuda(), SENTS)
    for mix in (False, True):
        score, label = scoring.branched_scores(m, feats.cuda(), boxes.cuda(), SENTS, mix=mix)
        want, wlab = BR.scores(logit, conf, mix)
        np.testing.assert_allclose(score.cpu().numpy(), want.cpu().numpy(), rtol=1e-6)
        assert torch.equal(label, wlab)
