"""UNITER engine (arch 2) shape sweep against the f64 oracle, in every precision: logits, pooled, loss, EVERY parameter gradient tensor and the input gradients,
at the shapes where its own code can go wrong - one sample with one region, the 64-row maximum, both sides of the 16- / 32- / 48-row attention tile edges,
head size 16, 2072 rows, width 768 - in both row layouts, with the filler weights and with three times larger ones (at which a wrong mask edge or a wrong front
end moves logits and gradients far beyond the bounds: tests/test_uniter_sweep_host.py).  Cases, oracle, bounds and the comparator: tests/uniter_reference.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import uniter_reference as S                  # noqa: E402
from tests.test_gpu_engine import _report                # noqa: E402

SPLIT = ("bf16x3", "bf16x3_fwd")


def head_size(case):
    cfgd = S.CASES[case][0]
    return cfgd["hidden"] // cfgd["heads"]


def run_id(case, packed, gain):
    return "%s-%s-gain%d" % (case, "packed" if packed else "padded", gain)


# the split-f32 precisions exist at head size 64 only (rgqa_engine_create refuses any other: test_split_f32_is_refused_at_head_size_16), so the head-size-16 case
# runs the generic attention kernels in f32 and in bf16
SWEEP = [pytest.param(c, p, g, prec, id=run_id(c, p, g) + "-" + prec) for c, p, g in S.RUNS for prec in S.PRECISIONS if head_size(c) == 64 or prec not in SPLIT]


def make_engine(case, gain, precision):
    from rgqa_amd.engine import Engine
    e = Engine(precision=precision, hidden_dropout=0.0, attn_dropout=0.0, arch=2, **S.CASES[case][0]).allocate("cuda")
    W = S.case_weights(case, gain)
    assert {sp.name: tuple(sp.shape) for sp in e.specs} == {k: v.shape for k, v in W.items()}
    for sp in e.specs:
        e.view(e.params, sp).copy_(torch.from_numpy(W[sp.name]))
    return e


def device_batch(case):
    _, b = S.case_inputs(case)
    return {k: torch.tensor(v).cuda() for k, v in b.items() if k != "lengths"}, [int(v) for v in b["lengths"]]


def train_pass(e, d, lens, bufs=(None, None)):
    """forward + BCE x NA backward -> clones of (logits, pooled, loss, gradient arena); bufs: dL/dfeats and dL/dpos buffers for this pass alone"""
    e.set_input_grads(*bufs)
    lg, pl = e.forward(d["feats"], d["pos7"], d["input_ids"], d["input_mask"], d["segment_ids"], lengths=lens)
    loss = e.loss_backward(d["target"])
    e.set_input_grads(None, None)
    return lg.clone(), pl.clone(), loss.clone(), e.grads.clone()


def engine_result(e, case, packed):
    """the engine's side of uniter_reference.compare for one case and layout: two plain passes and one with the input-gradient buffers, after the bit-identity
    assertions between them (a train step is bit-reproducible; asking for input gradients changes no parameter gradient)"""
    d, lens = device_batch(case)
    B, O, F = d["feats"].shape
    e.ensure_shape(B, d["input_ids"].shape[1], O)
    e.sync_weights()
    first = train_pass(e, d, lens if packed else None)
    second = train_pass(e, d, lens if packed else None)
    df, dp = torch.full((B * O, F), 7.0, device="cuda"), torch.full((B * O, 7), 7.0, device="cuda")
    third = train_pass(e, d, lens if packed else None, (df, dp))
    torch.cuda.synchronize()
    for other, what in ((second, "second pass"), (third, "pass with input-gradient buffers")):
        assert torch.equal(first[0], other[0]) and torch.equal(first[2], other[2]), "logits or loss differ: " + what
        assert torch.equal(first[3], other[3]), "parameter gradients differ: " + what
    g = first[3].cpu()
    return dict(logits=first[0].cpu(), pooled=first[1].cpu(), loss=float(first[2].item()), grads={sp.name: e.view(g, sp) for sp in e.specs}, dfeats=df.cpu(), dpos=dp.cpu())


def check(tag, e, got, case, gain, tol, gtol, ztol):
    failed, worst = S.compare(got, S.reference(case, gain), tol, gtol, ztol, dead=tuple(sp.name for sp in e.specs if sp.dead))
    _report("uniter sweep %s vs f64 oracle" % tag, logits_max=worst["logits"], pooled_max=worst["pooled"], loss_abs=worst["loss"], worst_tensor_rel=worst["tensor"],
            zero_grad_norm=worst["zero"], worst_over_bound=worst["ratio"])
    print("    worst tensor: %s; nearest its bound: %s; bounds tol %.1e gtol %.1e ztol %.1e" % (worst["tensor_name"], worst["ratio_name"], tol, gtol, ztol))
    assert not failed, (tag, failed[:6], len(failed))


_X3_LOGITS = {}      # (case, packed, gain) -> the bf16x3 engine's logits


def x3_logits(case, packed, gain):
    key = (case, packed, gain)
    if key not in _X3_LOGITS:
        e = make_engine(case, gain, "bf16x3")
        d, lens = device_batch(case)
        e.ensure_shape(d["feats"].shape[0], d["input_ids"].shape[1], d["feats"].shape[1])
        e.sync_weights()
        _X3_LOGITS[key] = train_pass(e, d, lens if packed else None)[0].cpu()
    return _X3_LOGITS[key]


@pytest.mark.parametrize("case,packed,gain,precision", SWEEP)
def test_sweep_vs_f64_oracle(case, packed, gain, precision):
    """Bounds: uniter_reference.START_BOUNDS (those of the LXMERT sweep, tests/test_gpu_engine.py test_shape_sweep_vs_oracle) unless RAISED_BOUNDS names the run.
    Observed on MI355X: docs/MEASUREMENTS.md "UNITER shape sweep"."""
    e = make_engine(case, gain, precision)
    got = engine_result(e, case, packed)
    if precision == "bf16x3":
        _X3_LOGITS[(case, packed, gain)] = got["logits"]
    if precision == "bf16x3_fwd":
        assert torch.equal(got["logits"], x3_logits(case, packed, gain)), "bf16x3_fwd: the forward pass is not the bf16x3 forward pass"
    check("%s %s" % (run_id(case, packed, gain), precision), e, got, case, gain, *S.bounds(case, packed, gain, precision))


@pytest.mark.parametrize("precision", SPLIT)
def test_split_f32_is_refused_at_head_size_16(precision):
    from rgqa_amd.engine import Engine
    with pytest.raises(RuntimeError, match="head size 64"):
        Engine(precision=precision, hidden_dropout=0.0, attn_dropout=0.0, arch=2, **S.CASES["generic"][0])


@pytest.mark.parametrize("case", ["max64", "edges"])
def test_f32_layouts_in_turn_on_one_engine(case):
    """packed, padded, packed again on ONE engine (the row maps are rebuilt at every change of layout): each pass within the f32 bounds of the oracle"""
    e = make_engine(case, 3, "f32")
    for i, packed in enumerate((True, False, True)):
        got = engine_result(e, case, packed)
        check("%s f32 layouts in turn, pass %d (%s)" % (case, i, "packed" if packed else "padded"), e, got, case, 3, *S.bounds(case, packed, 3, "f32"))


def test_bind_refuses_more_than_64_joint_rows():
    """T = 30, O = 36: each within 64, their sum - the rows of one UNITER sequence - is not; refused when the shape is bound, before any launch, and the engine
    then serves a 64-row case"""
    e = make_engine("max64", 1, "f32")
    with pytest.raises(RuntimeError, match=r"T \+ O"):
        e.ensure_shape(2, 30, 36)
    got = engine_result(e, "max64", True)
    check("max64 f32 after a refused bind", e, got, "max64", 1, *S.bounds("max64", True, 1, "f32"))
    with pytest.raises(RuntimeError, match=r"T \+ O"):      # and with a shape bound before
        e.ensure_shape(2, 30, 36)
    got = engine_result(e, "max64", True)
    check("max64 f32 after a second refused bind", e, got, "max64", 1, *S.bounds("max64", True, 1, "f32"))
