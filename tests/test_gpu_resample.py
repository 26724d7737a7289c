"""The soft-resampling step on the device (tasks/gqa_resampling.py:176-220; rgqa_amd/csrc/resample.hip): batch weights, the row-weighted BCE head and the
fused weight-parameter gradient + SGD-momentum update against the reference statements (tests/resample_reference.py: torch on the CPU in f64, and in
f32 for the bound), their bit-level conditions, the engines' `resample_loss_backward` on all three backbones and `scoring.resample_finetune_loss` with
`ResampleWeights` through the drop-in GQAModel.

Accuracy bound, for every compared quantity: the device's deviation from the f64 evaluation is at most 8 x max(d32, 2^-24), d32 the deviation of the
statements' own f32 CPU evaluation from f64 on the same inputs.  The 8 is the margin tests/test_gpu_energy_loss.py grants for another summation order
and the hardware exp; 2^-24 is half an f32 ulp - no f32 result can be expected closer.  Deviations are relative for the losses, relative to the
maximum magnitude for weights, dlogits, row_loss and dtheta (and the momentum buffer), relative to lr_w max|buf| for theta after stepping.  The two
means over N are carried in f64 on the device and held to 1e-12 relative: f64 sums of at most a few hundred terms per thread and a 10-level tree
(a few tens of ulps of 1.1e-16, with exp / log1p / sqrt good to a few ulps), four orders of magnitude below the bound.

Inputs (tests/resample_reference.draw): logits 3 randn - 6, two soft entries per positive row, all-zero targets for the negative rows; theta = 2 randn with
theta[N // 2] = 25 (above softplus's threshold) and theta[N - 1] = -12; wid holds 0, N - 1, N // 2 and, from Bn = 7, one index three times.

Deviation from the issue's text in the duplicate case: Bn enters the gradient as 1 / Bn, so `wid = [j, j, j]` cannot have the bits of a batch of ONE row;
it is compared with `wid = [j, k, k]` carrying the f32 sum (a + b) + c on j and zero row losses on k - the same Bn, the same s_j, the same S."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.resample_reference import draw, draw_steps, evaluate

pytestmark = pytest.mark.gpu

MARGIN = 8.0
FLOOR = 2.0 ** -24
LR_W, MOMENTUM = 0.5, 0.9
NS = [2, 37, 4099, 262147]


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _lib_():
    from rgqa_amd import _lib
    return _lib, _lib.load()


def scratch_for(N, B):
    _lib, lib = _lib_()
    n = C.c_size_t()
    _lib.check(lib.rgqa_resample_scratch_floats(N, B, C.byref(n)))
    return torch.full((n.value + 8,), 5.0, device="cuda"), n.value


@functools.lru_cache(None)
def case(N, n_pos, Bn, NA, k_more=0):
    """inputs and the f64 / f32 evaluations of the reference statements on the CPU (computed once, shared, left unchanged)"""
    theta, wids, z, t = draw(N, n_pos, Bn, NA, 2000 + 3 * N + 5 * Bn + 7 * n_pos + NA)
    more = tuple(draw_steps(N, Bn, k_more, 77 + N)) if k_more else ()
    ev = lambda dt: evaluate(theta, wids, z, t, n_pos, dt, LR_W, MOMENTUM, more)
    return dict(theta=theta, wids=wids, z=z, t=t, more=more, r64=ev(torch.float64), r32=ev(torch.float32))


def run_weights(theta, wids):
    """rgqa_resample_weights on device tensors; 8 guard words behind weights, 2 guard doubles behind stats"""
    _lib, lib = _lib_()
    N, Bn = theta.numel(), wids.numel()
    scratch, ns = scratch_for(N, Bn)
    w = torch.full((Bn + 8,), 9.0, device="cuda")
    stats = torch.full((4,), 11.0, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    _lib.check(lib.rgqa_resample_weights(p(theta), N, p(wids), Bn, p(stats), p(w), p(scratch), _stream()))
    torch.cuda.synchronize()
    assert bool((w[Bn:] == 9.0).all()) and bool((stats[2:] == 11.0).all()) and bool((scratch[ns:] == 5.0).all()), "guard words overwritten"
    return w[:Bn].clone(), stats[:2].clone()


def run_loss(z, t, n_pos, weights, NAp=None, ldd=None, grad_scale=1.0):
    """rgqa_op_resample_loss through the C ABI: z [B, NA] (any row stride), t [B, NA + 1].  dlogits live in a buffer of B * ldd + 8 floats filled with 7:
    guard columns NAp .. ldd and 8 guard words behind the last row."""
    _lib, lib = _lib_()
    B, NA = z.shape
    NAp = NAp or NA
    ldd = ldd or NAp
    scratch, ns = scratch_for(1, B)
    buf = torch.full((B * ldd + 8,), 7.0, device="cuda")
    loss = torch.full((5,), 9.0, device="cuda")
    rl = torch.full((B - n_pos + 2,), 9.0, device="cuda")
    p = _lib.ptr
    _lib.check(lib.rgqa_op_resample_loss(p(z), z.stride(0), p(t), t.stride(0), B, n_pos, NA, NAp, p(weights), grad_scale, p(loss), p(buf), ldd, p(rl), p(scratch), _stream()))
    torch.cuda.synchronize()
    full = buf[:B * ldd].view(B, ldd)
    assert bool((scratch[ns:] == 5.0).all()) and bool((loss[3:] == 9.0).all()) and bool((rl[B - n_pos:] == 9.0).all()), "guard words overwritten"
    assert bool((buf[B * ldd:] == 7.0).all()) and bool((full[:, NAp:] == 7.0).all()), "dlogits written past NAp / past the last row"
    return dict(loss=loss[:3].clone(), dl=full[:, :NA].clone(), pad=full[:, NA:NAp].clone(), row_loss=rl[:B - n_pos].clone())


def run_step(theta, buf, wids, row_loss, stats, lr=LR_W, momentum=MOMENTUM):
    """rgqa_resample_step on copies of theta / buf with 8 guard words behind each and behind grad_out: (theta', buf', g)"""
    _lib, lib = _lib_()
    N, Bn = theta.numel(), wids.numel()
    scratch, ns = scratch_for(N, Bn)
    th, bf, g = (torch.full((N + 8,), 3.0, device="cuda") for _ in range(3))
    th[:N], bf[:N] = theta, buf
    p = _lib.ptr
    _lib.check(lib.rgqa_resample_step(p(th), p(bf), N, p(wids), p(row_loss), Bn, p(stats), lr, momentum, p(g), p(scratch), _stream()))
    torch.cuda.synchronize()
    assert bool((th[N:] == 3.0).all()) and bool((bf[N:] == 3.0).all()) and bool((g[N:] == 3.0).all()) and bool((scratch[ns:] == 5.0).all()), "guard words overwritten"
    return th[:N].clone(), bf[:N].clone(), g[:N].clone()


def on_device(c, layout):
    """'padded' = contiguous logits, dlogits with ldd = NAp = round_up(NA, 64); 'strided' = logits rows 13 floats apart from contiguous (row starts at odd
    words), ldd = NAp + 5 (as tests/test_gpu_energy_loss.py)"""
    z, t = c["z"], c["t"]
    B, NA = z.shape
    NAp = (NA + 63) // 64 * 64
    if layout == "padded":
        return z.cuda(), t.cuda(), NAp, NAp
    wide = torch.full((B, NA + 13), 99.0)
    wide[:, :NA] = z
    return wide.cuda()[:, :NA], t.cuda(), NAp, NAp + 5


def rel(a, ref):
    return abs(float(a) - float(ref)) / abs(float(ref))


def relmax(a, ref, scale=None):
    ref = ref.double()
    return float((a.detach().cpu().double() - ref).abs().max() / (ref.abs().max() if scale is None else scale))


def check_bound(tag, dev, r32):
    """dev / r32: {name: deviation from f64}"""
    print("%s: device / f32-reference deviation from f64: %s" % (tag, "  ".join("%s %.2e / %.2e" % (k, dev[k], r32[k]) for k in dev)))
    for k in dev:
        assert dev[k] <= MARGIN * max(r32[k], FLOOR), (tag, k, dev[k], r32[k])


# ------------------------------------------------------------------------------------------------ A: weights
@pytest.mark.parametrize("Bn", [1, 7, 32])
@pytest.mark.parametrize("N", NS)
def test_weights_against_the_reference_statements(N, Bn):
    c = case(N, 2, Bn, 67)
    w, stats = run_weights(c["theta"].cuda(), c["wids"].cuda())
    sp = torch.nn.functional.softplus(c["theta"].double())
    m1, mh = float(sp.mean()), float(sp.sqrt().mean())
    assert rel(stats[0], m1) <= 1e-12 and rel(stats[1], mh) <= 1e-12, (stats.tolist(), m1, mh)
    check_bound("weights N=%d Bn=%d" % (N, Bn), dict(weights=relmax(w, c["r64"]["weights"])), dict(weights=relmax(c["r32"]["weights"], c["r64"]["weights"])))


def test_a_single_weight_parameter_runs():
    """N = 1: weights are identically 1 and the gradient an exact zero in exact arithmetic - no relative measure; the calls run, the weights are within the
    bound of 1 and theta stays finite"""
    theta, wids = torch.tensor([0.3], device="cuda"), torch.tensor([0, 0, 0], device="cuda")
    w, stats = run_weights(theta, wids)
    assert float((w - 1.0).abs().max()) <= MARGIN * FLOOR
    th, bf, g = run_step(theta, torch.zeros(1, device="cuda"), wids, torch.tensor([3.0, 4.0, 6.0], device="cuda"), stats)
    assert bool(torch.isfinite(th).all()) and bool(torch.isfinite(bf).all()) and float(g.abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------ B: loss
LOSS_SHAPES = [(5, 2, 67), (12, 5, 300), (64, 32, 1842), (300, 150, 67)]


@pytest.mark.parametrize("layout", ["padded", "strided"])
@pytest.mark.parametrize("B,n_pos,NA", LOSS_SHAPES)
def test_loss_against_the_reference_statements(B, n_pos, NA, layout):
    c = case(37, n_pos, B - n_pos, NA)
    r64, r32 = c["r64"], c["r32"]
    w, _ = run_weights(c["theta"].cuda(), c["wids"].cuda())
    z, t, NAp, ldd = on_device(c, layout)
    d = run_loss(z, t, n_pos, w, NAp, ldd)
    dev = dict(loss=rel(d["loss"][0], r64["loss"]), loss_pos=rel(d["loss"][1], r64["loss_pos"]), loss_neg=rel(d["loss"][2], r64["loss_neg"]),
               dlogits=relmax(d["dl"], r64["dlogits"]), row_loss=relmax(d["row_loss"], r64["row_loss"]))
    ref = dict(loss=rel(r32["loss"], r64["loss"]), loss_pos=rel(r32["loss_pos"], r64["loss_pos"]), loss_neg=rel(r32["loss_neg"], r64["loss_neg"]),
               dlogits=relmax(r32["dlogits"], r64["dlogits"]), row_loss=relmax(r32["row_loss"], r64["row_loss"]))
    check_bound("loss B=%d n_pos=%d NA=%d %s" % (B, n_pos, NA, layout), dev, ref)
    # padded columns: exact (positive) zeros
    assert d["pad"].numel() == B * (NAp - NA) and bool((d["pad"] == 0).all()) and not bool(torch.signbit(d["pad"]).any())
    h = run_loss(z, t, n_pos, w, NAp, ldd, grad_scale=0.5)
    assert torch.equal(h["dl"], d["dl"] * 0.5) and torch.equal(h["loss"], d["loss"]) and torch.equal(h["row_loss"], d["row_loss"]) and float(d["dl"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ C: step
def pipeline(c, n_pos):
    """weights -> loss -> step on the device for the case's own batch: (weights, stats, loss dict, theta', buf', g)"""
    theta, wids = c["theta"].cuda(), c["wids"].cuda()
    w, stats = run_weights(theta, wids)
    d = run_loss(c["z"].cuda(), c["t"].cuda(), n_pos, w)
    th, bf, g = run_step(theta, torch.zeros_like(theta), wids, d["row_loss"], stats)
    return w, stats, d, th, bf, g


@pytest.mark.parametrize("Bn", [7, 32])
@pytest.mark.parametrize("N", NS)
def test_weight_gradient_against_autograd_of_the_statements(N, Bn):
    c = case(N, 2, Bn, 67)
    _, _, _, th, bf, g = pipeline(c, 2)
    r64, r32 = c["r64"], c["r32"]
    check_bound("dtheta N=%d Bn=%d" % (N, Bn), dict(dtheta=relmax(g, r64["dtheta"])), dict(dtheta=relmax(r32["dtheta"], r64["dtheta"])))
    assert torch.equal(bf, g)                                # a zero buffer: torch's first step, buf = g
    # dense: an index no row of the batch names still moves, through m1 and mh.  Which ones MUST move in f32: those whose update lr_w |g_j| (f64 reference)
    # is at least two ulps of theta_j - below that an f32 theta may round back to itself, in torch's SGD as well (sigmoid(theta_j) is small for negative
    # theta_j, and the untouched gradient cancels where sqrt(w_j) is near m1 / (2 mh)): at N = 262147, Bn = 32 that is 1.4 % of the entries.
    if N >= 37:
        untouched = torch.ones(N, dtype=torch.bool)
        untouched[c["wids"]] = False
        ulp = torch.from_numpy(np.spacing(np.abs(c["theta"].numpy()))).double()
        must = untouched & (LR_W * r64["dtheta"].abs() >= 2.0 * ulp)
        assert int(untouched.sum()) >= N - Bn and int(must.sum()) >= (N - Bn) // 2
        assert bool((th.cpu() != c["theta"])[must].all()), "untouched indices must move"
        assert float((g.cpu() != 0).float().mean()) > 0.999


@pytest.mark.parametrize("N", [37, 4099])
def test_three_steps_against_torch_sgd(N):
    """theta and the momentum buffer after 3 consecutive steps with fresh wid / row_loss per step, against torch.optim.SGD(momentum=0.9) in f64.  (N = 37 and
    4099: the measure is a maximum over the entries, and each entry of theta carries its own f32 rounding of up to half an ulp in the device's run and in
    the f32 reference's alike; over two entries that comparison would be a draw of two roundings, over dozens it is stable.)"""
    Bn = 7
    c = case(N, 2, Bn, 67, 2)
    r64, r32 = c["r64"], c["r32"]
    _, _, d, th, bf, _ = pipeline(c, 2)
    for wk, rk in c["more"]:
        wk = wk.cuda()
        _, stats = run_weights(th, wk)
        th, bf, _ = run_step(th, bf, wk, rk.cuda(), stats)
    scale = LR_W * max(r64["max_buf"])
    dev = dict(theta=relmax(th, r64["theta"], scale), buf=relmax(bf, r64["buf"]))
    ref = dict(theta=relmax(r32["theta"], r64["theta"], scale), buf=relmax(r32["buf"], r64["buf"]))
    check_bound("3 steps N=%d" % N, dev, ref)
    assert float((th.cpu() != c["theta"]).float().mean()) > 0.99          # (all but entries at the cancellation point of the untouched gradient)


# ------------------------------------------------------------------------------------------------ D: bit-level conditions
def bce_rows(z, t):
    """rgqa_op_bce on contiguous logits and the target without its UQ column: dlogits"""
    _lib, lib = _lib_()
    zc, tc = z.contiguous(), t[:, :-1].contiguous()
    B, NA = zc.shape
    dl = torch.empty(B, NA, device="cuda")
    loss = torch.zeros(1, device="cuda")
    p = _lib.ptr
    _lib.check(lib.rgqa_op_bce(p(zc), p(tc), p(loss), p(dl), B, NA, _stream()))
    return dl


@pytest.mark.parametrize("N", [37, 4099])
def test_every_output_repeats_bit_for_bit(N):
    c = case(N, 2, 7, 67)
    a, b = pipeline(c, 2), pipeline(c, 2)
    for x, y in zip(a, b):
        if isinstance(x, dict):
            assert all(torch.equal(x[k], y[k]) for k in x)
        else:
            assert torch.equal(x, y)


@pytest.mark.parametrize("B,n_pos,NA", [(12, 5, 300), (64, 32, 1842)])
def test_rows_have_the_bits_of_the_bce_operator(B, n_pos, NA):
    c = case(37, n_pos, B - n_pos, NA)
    w, _ = run_weights(c["theta"].cuda(), c["wids"].cuda())
    for layout in ("padded", "strided"):
        z, t, NAp, ldd = on_device(c, layout)
        d = run_loss(z, t, n_pos, w, NAp, ldd)
        assert torch.equal(d["dl"][:n_pos], bce_rows(z[:n_pos], t[:n_pos])), "positive rows are not rgqa_op_bce's on the positive rows alone"
        one = run_loss(z, t, n_pos, torch.ones(B - n_pos, device="cuda"), NAp, ldd)
        assert torch.equal(one["dl"][n_pos:], bce_rows(z[n_pos:], t[n_pos:])), "unit weights: negative rows are not rgqa_op_bce's on the negative rows alone"
        assert torch.equal(one["dl"][:n_pos], d["dl"][:n_pos]) and not torch.equal(one["dl"][n_pos:], d["dl"][n_pos:])
    assert float(d["dl"].abs().max()) > 0


def test_duplicates_are_summed_by_one_owner():
    """wid = [j, j, j] with row_loss [a, b, c] against wid = [j, k, k] with [(a + b) + c, 0, 0] (small integers: the f32 sum is exact): the same bits in
    the gradient, theta and the buffer.  (Equal Bn on both sides: the module docstring says why.)"""
    c = case(37, 2, 7, 67)
    theta = c["theta"].cuda()
    buf = torch.linspace(-0.01, 0.01, 37, device="cuda")
    j, k = 5, 9
    w3, st = run_weights(theta, torch.tensor([j, j, j], device="cuda"))
    w1, st1 = run_weights(theta, torch.tensor([j, k, k], device="cuda"))
    assert torch.equal(st, st1) and torch.equal(w3[0], w1[0]) and float(w3[0]) == float(w3[1]) == float(w3[2])
    a = run_step(theta, buf, torch.tensor([j, j, j], device="cuda"), torch.tensor([3.0, 4.0, 6.0], device="cuda"), st)
    b = run_step(theta, buf, torch.tensor([j, k, k], device="cuda"), torch.tensor([13.0, 0.0, 0.0], device="cuda"), st)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    # and the order of the batch does not matter where the sums are exact
    p = run_step(theta, buf, torch.tensor([j, k, j], device="cuda"), torch.tensor([7.0, 0.0, 6.0], device="cuda"), st)
    assert all(torch.equal(x, y) for x, y in zip(a, p))
    assert float(a[2].abs().max()) > 0


def test_python_objects_are_the_operators():
    from rgqa_amd import scoring
    from rgqa_amd.resample import ResampleWeights
    c = case(4099, 5, 7, 300)
    rw = ResampleWeights(4099, LR_W)
    assert rw.theta.is_cuda and float(rw.theta.abs().max()) == 0
    rw.load_state_dict(dict(theta=c["theta"], momentum_buffer=torch.zeros(4099)))
    w, stats = run_weights(c["theta"].cuda(), c["wids"].cuda())
    w_py = rw.batch_weights(c["wids"].tolist())
    assert torch.equal(w_py, w) and torch.equal(rw.stats, stats)
    assert torch.equal(rw.batch_weights(c["wids"]), w)                      # a CPU int64 tensor as well
    z, t, NAp, ldd = on_device(c, "strided")
    d = run_loss(z, t, 5, w, NAp, ldd)
    r = scoring.resample_loss_rows(z, t, 5, w)
    assert isinstance(r, scoring.ResampleLoss)
    assert torch.equal(torch.stack([r.loss, r.loss_pos, r.loss_neg]), d["loss"]) and torch.equal(r.dlogits, d["dl"]) and torch.equal(r.row_loss, d["row_loss"])
    th, bf, g = run_step(c["theta"].cuda(), torch.zeros(4099, device="cuda"), c["wids"].cuda(), d["row_loss"], stats)
    g_py = torch.empty(4099, device="cuda")
    rw.step(r.row_loss, grad_out=g_py)
    assert torch.equal(g_py, g) and torch.equal(rw.theta, th) and torch.equal(rw.momentum_buffer, bf)
    with pytest.raises(RuntimeError):
        rw.step(r.row_loss)                                                 # the indices and statistics were those of the theta before the update
    rw.batch_weights([1, 2])
    with pytest.raises(ValueError):
        rw.step(r.row_loss)                                                 # 7 row losses for 2 indices
    with pytest.raises(ValueError):
        rw.batch_weights([0, 4099])
    sw = rw.sampler_weights()
    assert sw.device.type == "cpu" and sw.shape == (4099,)
    torch.testing.assert_close(sw, torch.nn.functional.softplus(th.cpu()).sqrt())
    sd = rw.state_dict()
    rw2 = ResampleWeights(4099, 1.0)
    rw2.load_state_dict(sd)
    assert torch.equal(rw2.theta, rw.theta) and torch.equal(rw2.momentum_buffer, rw.momentum_buffer) and rw2.lr_w == LR_W


# ------------------------------------------------------------------------------------------------ E: engines
_ENGINE = {}


def engine_case(kind, prec):
    """(engine, forward arguments, target [B, NA] on the CPU, input-gradient buffer shapes) with an EVEN batch; the last one built is kept for the next
    case.  The split-f32 forward needs head size 64, which synth.SMALL / U_SMALL do not have, so bf16x3_fwd runs at the sizes the existing bf16x3_fwd
    tests build (tests/test_gpu_engine.py's MED with B = 6), as tests/test_gpu_energy_loss.py does."""
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
            cfgd, (B, T, O) = synth.SMALL, (4, 8, 6)
            raw = synth.synth_batch(B, T, O=O, F=32, NA=11, vocab=64, seed=85, uq_frac=0.34, min_len=2)
        b = dev(raw)
        e = make_engine(cfgd, prec)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        return e, (b["feats"], b["boxes"], b["input_ids"], b["input_mask"], b["segment_ids"]), torch.from_numpy(raw["target"]), ((B * O, cfgd["feat_dim"]), (B * O, 4))
    if kind == "uniter":
        from tests.test_uniter import make_engine, dev
        if prec == "bf16x3_fwd":
            from tests.test_gpu_engine import MED
            cfgd, (B, T, O) = dict(MED, l_layers=3, x_layers=0, r_layers=0, pos_dim=7), (6, 12, 10)
        else:
            cfgd, (B, T, O) = synth.U_SMALL, (4, 8, 6)
        raw = synth.uniter_batch(cfgd, T, B, O, 55)
        b = dev(raw)
        e = make_engine(cfgd, prec)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        return e, (b["feats"], b["pos7"], b["input_ids"], b["input_mask"], b["segment_ids"]), torch.from_numpy(raw["target"]), ((B * O, cfgd["feat_dim"]), (B * O, 7))
    from tests.test_gpu_odin import butd_engine
    from tests.test_input_grads_oracle import butd_g7_inputs
    c, filled, feat, pos, toks = butd_g7_inputs()
    B = 4                                                    # the first four of the five sentences: an even batch
    e = butd_engine(prec, filled, len(synth.BUTD_WORDS), 23, B, 40, 36)
    kg = toks[:B].contiguous().cuda()
    target = torch.zeros(B, 23)
    target[torch.arange(B), torch.tensor([3, 7, 11, 0])] = 1.0
    return e, (feat[:B].contiguous().cuda(), pos[:B].contiguous().cuda(), kg, kg, None), target, ((B * 36, 2048), (B * 36, 4))


def pos_neg_target(target, n_pos):
    """[B, NA] answers -> [B, NA + 1]: rows from n_pos on unanswerable (no answers, UQ column 1), a second soft entry in the positive rows"""
    B, NA = target.shape
    t = torch.zeros(B, NA + 1)
    for b in range(n_pos):
        t[b, :NA] = target[b]
        a = int(target[b].argmax())
        t[b, a], t[b, (a + 3) % NA] = 0.9, 0.3
    t[n_pos:, NA] = 1.0
    return t


@pytest.mark.parametrize("prec", ["f32", "bf16x3_fwd"])
@pytest.mark.parametrize("kind", ["lxmert", "uniter", "butd"])
def test_engine_resample_loss_backward(kind, prec):
    """after a forward: the gradient arena of resample_loss_backward = the arena of backward(dlogits) with the operator's dlogits on the engine's own logits
    (and loss / row_loss are the operator's); n_pos = B / 2 with unit weights = the arena of loss_backward(grad_scale=2) (both scale by exact powers of
    two); input-gradient buffers change no parameter gradient; grad_scale and accumulate go the way backward's do.  Every comparison is torch.equal."""
    from rgqa_amd import scoring
    e, fwd, target, in_shapes = engine_case(kind, prec)
    B, NA = target.shape
    n_pos = B // 2
    assert 2 * n_pos == B
    tuq = pos_neg_target(target, n_pos).cuda()
    weights = torch.linspace(0.4, 1.7, B - n_pos, device="cuda")
    lg = e.forward(*fwd)[0].clone()
    r = scoring.resample_loss_rows(lg, tuq, n_pos, weights)
    assert bool(torch.isfinite(r.loss)) and float(r.loss_neg) > 0 and float(r.loss_pos) > 0

    loss, rl = e.resample_loss_backward(tuq, n_pos, weights)
    g1, loss, rl, parts = e.grads.clone(), loss.clone(), rl.clone(), e.resample_loss_parts.clone()
    assert loss.shape == (1,) and torch.equal(loss[0], r.loss) and torch.equal(parts, torch.stack([r.loss, r.loss_pos, r.loss_neg])) and torch.equal(rl, r.row_loss)
    e.forward(*fwd)
    e.backward(r.dlogits)
    assert torch.equal(e.grads, g1), "resample_loss_backward is not backward(the operator's dlogits)"
    assert bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    e.forward(*fwd)
    e.resample_loss_backward(tuq[:, :NA], n_pos, weights)                  # a target without the UQ column is the same thing
    assert torch.equal(e.grads, g1)

    ones = torch.ones(B - n_pos, device="cuda")
    e.forward(*fwd)
    e.resample_loss_backward(tuq, n_pos, ones)
    g_unit = e.grads.clone()
    e.forward(*fwd)
    e.loss_backward(tuq[:, :NA], grad_scale=2.0)
    assert torch.equal(e.grads, g_unit), "n_pos = B / 2 with unit weights is not loss_backward(grad_scale=2)"
    assert not torch.equal(g_unit, g1)                                     # the weights reach the parameters

    df, db = torch.full(in_shapes[0], 7.0, device="cuda"), torch.full(in_shapes[1], 7.0, device="cuda")
    e.set_input_grads(df, db)
    e.forward(*fwd)
    e.resample_loss_backward(tuq, n_pos, weights)
    e.set_input_grads(None, None)
    torch.cuda.synchronize()
    assert torch.equal(e.grads, g1), "parameter gradients changed by asking for input gradients"
    assert bool(torch.isfinite(df).all()) and bool(torch.isfinite(db).all()) and float(df.abs().max()) > 0 and not bool((df == 7.0).all()) and not bool((db == 7.0).all())

    e.forward(*fwd)
    e.backward(r.dlogits * 0.5)
    e.forward(*fwd)
    e.backward(r.dlogits * 0.5, accumulate=True)
    g_acc = e.grads.clone()
    e.forward(*fwd)
    e.resample_loss_backward(tuq, n_pos, weights, grad_scale=0.5)
    e.forward(*fwd)
    e.resample_loss_backward(tuq, n_pos, weights, grad_scale=0.5, accumulate=True)
    assert torch.equal(e.grads, g_acc)
    for bad in (lambda: e.resample_loss_backward(tuq, 0, weights), lambda: e.resample_loss_backward(tuq, B, weights), lambda: e.resample_loss_backward(tuq, n_pos, weights[:-1]),
                lambda: e.resample_loss_backward(tuq[:, :NA - 1], n_pos, weights), lambda: e.resample_loss_backward(tuq, n_pos, weights.cpu())):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ F: drop-in
from tests.test_gpu_dropin import env                                # noqa: E402,F401  (fixture: the small LXMERT drop-in model)


def test_resample_finetune_through_the_dropin_model(env):      # noqa: F811
    """two steps of the trainer with gqa_resampling.py:181-220 replaced by one forward on the concatenated batch, `resample_finetune_loss`, the model's
    optimizer step and `rw.step()`: the loss agrees with the f64 statements on the model's own logits within the bound, loss_w is -loss_neg, a
    parameter and theta have both moved"""
    from rgqa_amd import scoring
    from rgqa_amd.resample import ResampleWeights
    from tests.test_gpu_dropin import build, batch, SENTS
    from lxrt.optimization import BertAdam
    T, N, n_pos = 20, 37, 3
    m, _ = build("f32", T)
    m.train()
    feats, boxes, target = batch(T)
    tuq = pos_neg_target(target, n_pos).cuda()
    feats, boxes = feats.cuda(), boxes.cuda()
    rw = ResampleWeights(N, LR_W)
    with pytest.raises(RuntimeError):
        rw.step(torch.ones(3, device="cuda"))                    # no batch_weights yet
    rw.theta.copy_(draw(N, 1, 1, 5, 9)[0])
    optim = BertAdam(list(m.parameters()), lr=1e-3)              # t_total = -1: a constant rate (under warmup_linear the rate of the FIRST step is 0)
    named = dict(m.named_parameters())
    head = [k for k in named if "logit_fc" in k and k.endswith("bias")]
    par = named[head[-1] if head else list(named)[-1]]             # the last bias of the answer head
    p0, theta0 = par.detach().clone(), rw.theta.clone()
    for step, wids in enumerate(([36, 0, 18], [7, 7, 36])):
        theta_in = rw.theta.cpu().clone()
        logit = m(feats, boxes, SENTS)
        loss, loss_w = scoring.resample_finetune_loss(logit, tuq, n_pos, rw, wids)
        assert loss.dim() == 0 and loss.requires_grad and loss_w.dim() == 0 and not loss_w.requires_grad
        r = scoring.resample_loss_rows(logit.detach(), tuq, n_pos, rw.weights)
        assert torch.equal(loss.detach(), r.loss) and torch.equal(loss_w, -r.loss_neg) and torch.equal(rw.row_loss, r.row_loss)
        lg, wt = logit.detach().cpu(), torch.tensor(wids)
        r64, r32 = evaluate(theta_in, wt, lg, tuq.cpu(), n_pos, torch.float64), evaluate(theta_in, wt, lg, tuq.cpu(), n_pos, torch.float32)
        dev = dict(loss=rel(loss.detach().cpu(), r64["loss"]), loss_w=rel(loss_w.cpu(), r64["loss_w"]))
        check_bound("drop-in step %d (loss %.7f)" % (step, float(loss.detach())), dev, dict(loss=rel(r32["loss"], r64["loss"]), loss_w=rel(r32["loss_w"], r64["loss_w"])))
        optim.zero_grad()
        loss.backward()
        assert par.grad is not None and float(par.grad.abs().max()) > 0
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.)
        optim.step()
        g = torch.empty(N, device="cuda")
        rw.step(grad_out=g)
        check_bound("drop-in step %d" % step, dict(dtheta=relmax(g, r64["dthetas"][0])), dict(dtheta=relmax(r32["dthetas"][0], r64["dthetas"][0])))
    assert not torch.equal(par.detach(), p0)
    assert float((rw.theta != theta0).float().mean()) > 0.9 and bool((rw.theta != theta0)[[36, 0, 18, 7]].all())
