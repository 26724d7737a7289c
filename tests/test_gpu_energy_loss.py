"""The loss head of the energy fine-tuning on the device (tasks/gqa_energy.py:117-145; rgqa_amd/csrc/energy_loss.hip): the stand-alone operator
against the reference statements (tests/energy_reference.py: evaluated with torch on the CPU in f64, and in f32 for the bound), its bit-level
conditions, the engines' `energy_loss_backward` on all three backbones and `scoring.energy_finetune_loss` through the drop-in GQAModel.

Accuracy bound (loss, base loss, regulariser: relative; energy: absolute; dlogits: relative to max|dlogits|): the device's deviation from the f64
evaluation is at most 8 x the deviation of the statements' own f32 CPU evaluation from f64 on the same inputs.  The 8 is a margin for the other
summation order over up to 1842 terms and the hardware exp behind the shared sigmoid, not a measurement.  Observed figures: docs/MEASUREMENTS.md
"Energy fine-tuning loss".

Inputs: logits 3 randn - 6, every third row (from row 1) flagged OOD - so the smallest batch (B = 5) has 3 ID and 2 OOD rows: with margins at the
(lower) medians a subset needs 3 (ID) / 2 (OOD) rows to hold an active hinge -, two soft target entries per ID row; m_in / m_out are the negated f64
medians of the ID / OOD energies rounded to f32 (the C ABI's type), so each subset has active and inactive rows."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.energy_reference import draw, evaluate, margins

pytestmark = pytest.mark.gpu

SHAPES = [(5, 67), (7, 300), (32, 1842), (300, 67)]
MARGIN = 8.0
EDGE = 1e-3          # a row counts as active / inactive only this far from its hinge's edge (f32 energies carry errors of 1e-5 and less)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(None)
def case(B, NA, mce, ood="third"):
    """inputs, margins and the f64 / f32 evaluations of the reference statements on the CPU (computed once, shared, left unchanged)"""
    z, t = draw(B, NA, 1000 + 7 * B + NA + (1 if mce else 0), ood=ood)
    m_in, m_out, E = margins(z, t, mce)
    idm = t[:, -1] == 0
    arg = torch.where(idm, -E - m_in, m_out + E)           # the hinge's argument per row, f64
    return dict(z=z, t=t, m_in=m_in, m_out=m_out, idm=idm, arg=arg, r64=evaluate(z, t, m_in, m_out, mce, torch.float64), r32=evaluate(z, t, m_in, m_out, mce, torch.float32))


def run_op(z, t, m_in, m_out, mce, NAp=None, ldd=None, weight=0.1, grad_scale=1.0):
    """rgqa_op_energy_loss through the C ABI on device tensors: z [B, NA] (any row stride), t [B, NA + 1].  dlogits live in a buffer of B * ldd + 8
    floats filled with 7: guard columns NAp .. ldd and 8 guard words behind the last row."""
    from rgqa_amd import _lib
    lib = _lib.load()
    B, NA = z.shape
    NAp = NAp or NA
    ldd = ldd or NAp
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_energy_loss_scratch_floats(B, C.byref(n)))
    scratch = torch.full((n.value + 8,), 5.0, device="cuda")
    buf = torch.full((B * ldd + 8,), 7.0, device="cuda")
    loss = torch.full((5,), 9.0, device="cuda")
    en = torch.full((B + 2,), 9.0, device="cuda")
    lab = torch.full((B + 2,), -5, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    _lib.check(lib.rgqa_op_energy_loss(p(z), z.stride(0), p(t), t.stride(0), C.c_void_p(t.data_ptr() + 4 * NA), t.stride(0), B, NA, NAp, 1 if mce else 0, weight,
                                       m_in, m_out, grad_scale, p(loss), p(buf), ldd, p(en), p(lab), p(scratch), _stream()))
    torch.cuda.synchronize()
    full = buf[:B * ldd].view(B, ldd)
    assert bool((scratch[n.value:] == 5.0).all()) and bool((loss[3:] == 9.0).all()) and bool((en[B:] == 9.0).all()) and bool((lab[B:] == -5).all()), "guard words overwritten"
    assert bool((buf[B * ldd:] == 7.0).all()) and bool((full[:, NAp:] == 7.0).all()), "dlogits written past NAp / past the last row"
    return dict(loss=loss[:3].clone(), dl=full[:, :NA].clone(), pad=full[:, NA:NAp].clone(), energy=en[:B].clone(), label=lab[:B].clone())


def on_device(c, layout):
    """the two operand layouts of the issue: 'padded' = contiguous logits, dlogits with ldd = NAp = round_up(NA, 64); 'strided' = logits rows 13 floats
    apart from contiguous (row starts at odd words), ldd = NAp + 5"""
    z, t = c["z"], c["t"]
    B, NA = z.shape
    NAp = (NA + 63) // 64 * 64
    if layout == "padded":
        return z.cuda(), t.cuda(), NAp, NAp
    wide = torch.full((B, NA + 13), 99.0)
    wide[:, :NA] = z
    return wide.cuda()[:, :NA], t.cuda(), NAp, NAp + 5


def deviations(got, r64):
    """loss / base / reg: relative; energy: absolute; dlogits: relative to max|dlogits| - all against the f64 evaluation"""
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    out = dict(base=rel(got["base"], r64["base"]), energy=float((got["energy"].double() - r64["energy"]).abs().max()),
               dlogits=float((got["dlogits"].double() - r64["dlogits"]).abs().max() / r64["dlogits"].abs().max()))
    if not torch.isnan(r64["loss"]):
        out["loss"], out["reg"] = rel(got["loss"], r64["loss"]), rel(got["reg"], r64["reg"])
    return out


def check_bound(tag, dev, r32, r64):
    got = dict(loss=dev["loss"][0].cpu(), base=dev["loss"][1].cpu(), reg=dev["loss"][2].cpu(), energy=dev["energy"].cpu(), dlogits=dev["dl"].cpu())
    d, r = deviations(got, r64), deviations(r32, r64)
    print("%s: device / f32-reference deviation from f64: %s" % (tag, "  ".join("%s %.2e / %.2e" % (k, d[k], r[k]) for k in d)))
    for k in d:
        assert d[k] <= MARGIN * r[k], (tag, k, d[k], r[k])


def bce_rows(z, t):
    """rgqa_op_bce on contiguous logits and the target without its UQ column"""
    from rgqa_amd import _lib
    zc, tc = z.contiguous(), t[:, :-1].contiguous()
    B, NA = zc.shape
    dl = torch.empty(B, NA, device="cuda")
    loss = torch.zeros(1, device="cuda")
    p = _lib.ptr
    _lib.check(_lib.load().rgqa_op_bce(p(zc), p(tc), p(loss), p(dl), B, NA, _stream()))
    return dl


# ------------------------------------------------------------------------------------------------ operator
@pytest.mark.parametrize("layout", ["padded", "strided"])
@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA", SHAPES)
def test_operator_against_the_reference_statements(B, NA, mce, layout):
    c = case(B, NA, mce)
    idm, arg = c["idm"], c["arg"]
    act, inact = arg > 0, arg <= 0
    for name, sub in (("ID", idm), ("OOD", ~idm)):
        n, na = int(sub.sum()), int((act & sub).sum())
        print("B=%d NA=%d %s: %d of %d %s rows active" % (B, NA, "mce" if mce else "bce", na, n, name))
        assert na >= 1, "no active %s hinge: the case would pass on the base loss alone" % name
        assert n < 2 or int((inact & sub).sum()) >= 1
    z, t, NAp, ldd = on_device(c, layout)
    dev = run_op(z, t, c["m_in"], c["m_out"], mce, NAp, ldd)
    check_bound("B=%d NA=%d %s %s" % (B, NA, "mce" if mce else "bce", layout), dev, c["r32"], c["r64"])
    # label: the statement on the device's logits copied to the CPU; the two largest sigmoid values of every row are apart
    s = torch.sigmoid(z.cpu())
    top = s.topk(2, dim=1).values
    assert bool((top[:, 0] - top[:, 1] > 1e-6).all())
    assert torch.equal(dev["label"].cpu(), s.max(1)[1])
    # padded columns: exact (positive) zeros
    assert dev["pad"].numel() == B * (NAp - NA) and bool((dev["pad"] == 0).all()) and not bool(torch.signbit(dev["pad"]).any())


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA", SHAPES)
def test_operator_bit_level_conditions(B, NA, mce):
    c = case(B, NA, mce)
    zp, tp, NAp, lddp = on_device(c, "padded")
    zs, ts, _, ldds = on_device(c, "strided")
    a = run_op(zp, tp, c["m_in"], c["m_out"], mce, NAp, lddp)
    b = run_op(zp, tp, c["m_in"], c["m_out"], mce, NAp, lddp)
    s = run_op(zs, ts, c["m_in"], c["m_out"], mce, NAp, ldds)
    for k in ("loss", "dl", "energy", "label"):
        assert torch.equal(a[k], b[k]), "two runs differ in %s" % k
        assert torch.equal(a[k], s[k]), "%s depends on the operands' alignment" % k
    h = run_op(zs, ts, c["m_in"], c["m_out"], mce, NAp, ldds, grad_scale=0.5)
    assert torch.equal(h["dl"], a["dl"] * 0.5) and torch.equal(h["loss"], a["loss"]) and float(a["dl"].abs().max()) > 0
    if mce:
        return
    ref = bce_rows(zp, tp)
    w0 = run_op(zp, tp, c["m_in"], c["m_out"], False, NAp, lddp, weight=0.0)
    assert torch.equal(w0["dl"], ref), "weight = 0: dlogits are not rgqa_op_bce's"
    assert torch.equal(run_op(zs, ts, c["m_in"], c["m_out"], False, NAp, ldds, weight=0.0)["dl"], ref)
    # with the weight on: rows with an inactive hinge keep the bits, rows with an active one do not
    quiet, loud = (c["arg"] < -EDGE).cuda(), (c["arg"] > EDGE).cuda()
    assert int(quiet.sum()) >= 1 and int(loud.sum()) >= 2
    assert torch.equal(a["dl"][quiet], ref[quiet])
    assert bool((a["dl"][loud] != ref[loud]).any(dim=1).all())


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("ood", ["none", "all"])
def test_operator_empty_subset_follows_torch(ood, mce):
    """B = 4, NA = 67, no OOD row / no ID row: the loss is NaN as the statements' is (tests/test_energy_loss_host.py pins that), dlogits are finite and
    within the bound, and they carry the other subset's hinge"""
    c = case(4, 67, mce, ood)
    assert torch.isnan(c["r64"]["loss"]) and torch.isfinite(c["r64"]["dlogits"]).all() and int((c["arg"] > EDGE).sum()) >= 1
    z, t, NAp, ldd = on_device(c, "padded")
    dev = run_op(z, t, c["m_in"], c["m_out"], mce, NAp, ldd)
    assert bool(torch.isnan(dev["loss"][0])) and bool(torch.isnan(dev["loss"][2])) and bool(torch.isfinite(dev["loss"][1]))
    assert bool(torch.isfinite(dev["dl"]).all()) and bool(torch.isfinite(dev["energy"]).all())
    check_bound("B=4 NA=67 %s ood=%s" % ("mce" if mce else "bce", ood), dev, c["r32"], c["r64"])
    w0 = run_op(z, t, c["m_in"], c["m_out"], mce, NAp, ldd, weight=0.0)
    assert not torch.equal(w0["dl"], dev["dl"])


def test_python_wrapper_is_the_operator():
    from rgqa_amd import scoring
    c = case(7, 300, False)
    z, t, NAp, ldd = on_device(c, "strided")
    dev = run_op(z, t, c["m_in"], c["m_out"], False, NAp, ldd)
    r = scoring.energy_loss_rows(z, t, c["m_in"], c["m_out"])
    assert isinstance(r, scoring.EnergyLoss)
    assert torch.equal(torch.stack([r.loss, r.base, r.reg]), dev["loss"]) and torch.equal(r.dlogits, dev["dl"]) and torch.equal(r.energy, dev["energy"]) and torch.equal(r.label, dev["label"])
    s = scoring.score_rows(z)                      # the energy score and label of the test scripts: the same formulas
    assert torch.equal(s.label, r.label)
    np.testing.assert_allclose(s.energy.cpu().numpy(), r.energy.cpu().numpy(), rtol=1e-5)
    with pytest.raises(ValueError):
        scoring.energy_loss_rows(z, t[:, :-1], 25.0, 0.0)
    with pytest.raises(ValueError):
        scoring.energy_finetune_loss(z, t, 25.0, 0.0, weight=-0.1)
    with pytest.raises(ValueError):
        scoring.energy_loss_rows(z, t.cpu(), 25.0, 0.0)


# ------------------------------------------------------------------------------------------------ engines
def with_uq(target, ood_rows):
    """[B, NA] answers -> [B, NA + 1]: the listed rows unanswerable (UQ column 1, no answers), a second soft entry in the others"""
    B, NA = target.shape
    t = torch.zeros(B, NA + 1)
    t[:, :NA] = target
    for b in range(B):
        if b in ood_rows:
            t[b] = 0.0
            t[b, NA] = 1.0
        else:
            t[b, (int(target[b].argmax()) + 3) % NA] = 0.3
    return t


def margins_for(lg, tuq, mce):
    """margins that leave active and inactive hinges for the engine's own logits: the mean of the ID energies, just below the largest OOD energy"""
    from rgqa_amd import scoring
    E = scoring.energy_loss_rows(lg, tuq, weight=0.0, mce_loss=mce).energy.cpu().double()
    idm = tuq[:, -1].cpu() == 0
    return float(np.float32(-float(E[idm].mean()))), float(np.float32(-float(E[~idm].max()) + 0.25))


_ENGINE = {}


def engine_case(kind, prec):
    """(engine, forward arguments, forward keywords, target [B, NA] on the CPU, input-gradient buffer shapes); the last one built is kept for the next
    case.  The split-f32 forward needs head size 64, which synth.SMALL / U_SMALL (hidden 64, 4 heads) do not have, so bf16x3_fwd runs at the sizes the
    existing bf16x3_fwd tests build: tests/test_gpu_engine.py's MED (hidden 128, 2 heads, 70 answers) with its B = 6 batch, and for UNITER the same sizes
    with UNITER's layer layout and 7 position features."""
    if _ENGINE.get("key") != (kind, prec):
        _ENGINE.clear()
        _ENGINE.update(key=(kind, prec), val=_engine_case(kind, prec))
    return _ENGINE["val"]


def _engine_case(kind, prec):
    from rgqa_amd import synth
    if kind == "lxmert":
        from tests.test_gpu_engine import make_engine, dev, MED
        if prec == "bf16x3_fwd":
            cfgd, (B, T, O) = MED, (6, 12, 10)
            raw = synth.synth_batch(B, T, O=O, F=MED["feat_dim"], NA=MED["num_answers"], vocab=MED["vocab_size"], seed=5, min_len=2)
        else:
            cfgd, (B, T, O) = synth.SMALL, (3, 8, 6)
            raw = synth.small_batch(T)
        b = dev(raw)
        e = make_engine(cfgd, prec)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        return e, (b["feats"], b["boxes"], b["input_ids"], b["input_mask"], b["segment_ids"]), {}, torch.from_numpy(raw["target"]), ((B * O, cfgd["feat_dim"]), (B * O, 4))
    if kind == "uniter":
        from tests.test_uniter import make_engine, dev
        if prec == "bf16x3_fwd":
            from tests.test_gpu_engine import MED
            cfgd, (B, T, O) = dict(MED, l_layers=3, x_layers=0, r_layers=0, pos_dim=7), (6, 12, 10)
        else:
            cfgd, (B, T, O) = synth.U_SMALL, (3, 8, 6)
        raw = synth.uniter_batch(cfgd, T, B, O, 55)
        b = dev(raw)
        e = make_engine(cfgd, prec)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        return e, (b["feats"], b["pos7"], b["input_ids"], b["input_mask"], b["segment_ids"]), {}, torch.from_numpy(raw["target"]), ((B * O, cfgd["feat_dim"]), (B * O, 7))
    from tests.test_gpu_odin import butd_engine
    from tests.test_input_grads_oracle import butd_g7_inputs
    c, filled, feat, pos, toks = butd_g7_inputs()
    e = butd_engine(prec, filled, len(synth.BUTD_WORDS), 23, 5, 40, 36)
    kg = toks.cuda()
    target = torch.zeros(5, 23)
    target[torch.arange(5), torch.tensor([3, 7, 11, 0, 22])] = 1.0
    return e, (feat.cuda(), pos.cuda(), kg, kg, None), {}, target, ((5 * 36, 2048), (5 * 36, 4))


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("prec", ["f32", "bf16x3_fwd"])
@pytest.mark.parametrize("kind", ["lxmert", "uniter", "butd"])
def test_engine_energy_loss_backward(kind, prec, mce):
    """after a forward: the gradient arena of energy_loss_backward = the arena of backward(dlogits) with the operator's dlogits on the engine's own
    logits (and loss / energy / label are the operator's); weight = 0 in BCE form = the arena of loss_backward; input-gradient buffers change no
    parameter gradient.  Every comparison is torch.equal."""
    from rgqa_amd import scoring
    e, fwd, kw, target, in_shapes = engine_case(kind, prec)
    tuq = with_uq(target, {1}).cuda()
    NA = target.shape[1]
    lg = e.forward(*fwd, **kw)[0].clone()
    m_in, m_out = margins_for(lg, tuq, mce)
    r = scoring.energy_loss_rows(lg, tuq, m_in, m_out, 0.1, mce)
    assert float(r.reg) > 0 and bool(torch.isfinite(r.loss))

    loss, en, lab = e.energy_loss_backward(tuq, m_in, m_out, 0.1, mce)
    g1, loss, en, lab, parts = e.grads.clone(), loss.clone(), en.clone(), lab.clone(), e.energy_loss_parts.clone()
    assert loss.shape == (1,) and torch.equal(loss[0], r.loss) and torch.equal(parts, torch.stack([r.loss, r.base, r.reg])) and torch.equal(en, r.energy) and torch.equal(lab, r.label)
    e.forward(*fwd, **kw)
    e.backward(r.dlogits)
    assert torch.equal(e.grads, g1), "energy_loss_backward is not backward(the operator's dlogits)"
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0

    e.forward(*fwd, **kw)
    e.loss_backward(tuq[:, :NA])
    g_bce = e.grads.clone()
    assert not torch.equal(g_bce, g1)                       # the regulariser (or the MCE form) reaches the parameters
    if not mce:
        e.forward(*fwd, **kw)
        e.energy_loss_backward(tuq, m_in, m_out, 0.0, False)
        assert torch.equal(e.grads, g_bce), "weight = 0 in BCE form is not loss_backward"

    df, db = torch.full(in_shapes[0], 7.0, device="cuda"), torch.full(in_shapes[1], 7.0, device="cuda")
    e.set_input_grads(df, db)
    e.forward(*fwd, **kw)
    e.energy_loss_backward(tuq, m_in, m_out, 0.1, mce)
    e.set_input_grads(None, None)
    torch.cuda.synchronize()
    assert torch.equal(e.grads, g1), "parameter gradients changed by asking for input gradients"
    assert bool(torch.isfinite(df).all()) and bool(torch.isfinite(db).all()) and float(df.abs().max()) > 0 and not bool((df == 7.0).all()) and not bool((db == 7.0).all())
    # grad_scale and accumulate go the way loss_backward's do
    e.forward(*fwd, **kw)
    e.energy_loss_backward(tuq, m_in, m_out, 0.1, mce, grad_scale=0.5)
    e.forward(*fwd, **kw)
    e.backward(r.dlogits * 0.5)
    g_half = e.grads.clone()
    e.forward(*fwd, **kw)
    e.energy_loss_backward(tuq, m_in, m_out, 0.1, mce, grad_scale=0.5)
    assert torch.equal(e.grads, g_half)
    with pytest.raises(ValueError):
        e.energy_loss_backward(tuq[:, :NA], m_in, m_out)
    with pytest.raises(ValueError):
        e.energy_loss_backward(tuq, m_in, m_out, weight=-1.0)


# ------------------------------------------------------------------------------------------------ drop-in
from tests.test_gpu_dropin import env                                # noqa: E402,F401  (fixture: the small LXMERT drop-in model)


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
def test_energy_finetune_loss_through_the_dropin_model(env, mce):      # noqa: F811
    """the trainer's statements with gqa_energy.py:122-138 / :144-145 replaced by the one call: every .grad equals the engine-direct arena, the loss
    agrees with the torch statements on the same logits within the operator's bound"""
    from rgqa_amd import scoring
    from tests.test_gpu_dropin import build, batch, SENTS
    T = 20
    m, _ = build("f32", T)
    m.eval()
    feats, boxes, target = batch(T)
    tuq = with_uq(target, {1, 4}).cuda()
    logit = m(feats.cuda(), boxes.cuda(), SENTS)
    lg = logit.detach().clone()
    m_in, m_out = margins_for(lg, tuq, mce)
    loss, score, label = scoring.energy_finetune_loss(logit, tuq, m_in, m_out, mce_loss=mce)
    assert loss.dim() == 0 and loss.requires_grad and not score.requires_grad and score.shape == (len(SENTS),) and label.dtype == torch.int64
    loss.backward()
    eng = m.lxrt_encoder.model._binding.engine
    arena = eng.grads.clone()
    named = dict(m.named_parameters())
    live = 0
    for sp in eng.specs:
        g = named[sp.name].grad
        if g is not None:
            live += 1
            assert torch.equal(g, eng.view(arena, sp)), sp.name
    assert live > 50
    l2, e2, lab2 = eng.energy_loss_backward(tuq, m_in, m_out, 0.1, mce)          # engine-direct, on the forward the model recorded
    assert torch.equal(eng.grads, arena), "the drop-in's gradients are not the engine-direct step's"
    assert torch.equal(l2[0], loss.detach()) and torch.equal(e2, score) and torch.equal(lab2, label)
    assert torch.equal(label.cpu(), torch.sigmoid(lg.cpu()).max(1)[1])
    r64, r32 = evaluate(lg.cpu(), tuq.cpu(), m_in, m_out, mce, torch.float64), evaluate(lg.cpu(), tuq.cpu(), m_in, m_out, mce, torch.float32)
    rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
    d, r = rel(loss.detach().cpu(), r64["loss"]), rel(r32["loss"], r64["loss"])
    print("drop-in %s: loss %.7f, device / f32-reference deviation from f64: %.2e / %.2e" % ("mce" if mce else "bce", float(loss.detach()), d, r))
    assert float(r64["reg"]) > 0 and d <= MARGIN * r, (d, r)
    # clip and step stay as they are
    from lxrt.optimization import BertAdam
    optim = BertAdam(list(m.parameters()), lr=1e-3)          # t_total = -1: a constant rate (under warmup_linear the rate of the FIRST step is 0)
    before = named["logit_fc.3.bias"].detach().clone() if "logit_fc.3.bias" in named else None
    torch.nn.utils.clip_grad_norm_(m.parameters(), 5.)
    optim.step()
    if before is not None:
        assert not torch.equal(named["logit_fc.3.bias"].detach(), before)
