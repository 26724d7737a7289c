"""The UNITER shape sweep can fail (CPU only): at every precision's bounds the comparator of tests/uniter_reference.py rejects four deliberately wrong variants
of the oracle on a gain-3 case with a margin of 1.5, it passes the f32 oracle at the f32 bounds on every case, and the explicit question lengths give exactly
the row counts the tile-edge cases are named for.  The GPU side is tests/test_gpu_uniter_sweep.py."""
import functools

import numpy as np
import pytest
import torch

from oracle import lxmert_ref as R
from oracle import uniter_ref as U
from tests import uniter_reference as S

MARGIN = 1.5


def test_explicit_lengths_give_the_tile_edge_row_counts():
    for name, rows in S.PACKED_ROWS.items():
        cfgd, B, T, O, lens, _ = S.CASES[name]
        _, b = S.case_inputs(name)
        assert tuple(int(v) for v in b["input_mask"].sum(1)) == tuple(lens), name
        assert S.packed_rows(b) == rows, (name, S.packed_rows(b))
        assert b["input_ids"].shape == (B, T) and b["feats"].shape == (B, O, cfgd["feat_dim"]) and T + O <= 64
        assert (b["input_ids"][:, 0] != 0).all() and ((b["input_ids"] != 0) == (b["input_mask"] != 0)).all()
    assert max(S.PACKED_ROWS["max64"]) == 64                       # four full 16-row tiles each way
    assert {16, 17, 31, 32} <= set(S.PACKED_ROWS["edges"]) and {32, 33, 47, 48} <= set(S.PACKED_ROWS["edges48"])
    for name, (cfgd, B, T, O, _, _) in S.CASES.items():
        _, b = S.case_inputs(name)
        assert b["feats"].shape == (B, O, cfgd["feat_dim"]) and b["pos7"].shape == (B, O, 7) and b["input_ids"].shape == (B, T), name
    ids = S.case_inputs("rows")[1]["input_ids"]
    counts = np.bincount(ids[ids != 0])
    assert ids.size == 740 and (counts >= 2).sum() >= 50           # repeated words: word-table rows that sum several text rows


def test_helper_forward_is_the_oracles_forward():
    """with the plain key mask and no option, uniter_reference.forward is oracle.uniter_ref.gqa_forward (pinned to the reference's vectors by
    tests/test_uniter.py test_oracle_matches_reference_vectors): equal bits in f32"""
    cfgd, b = S.case_inputs("edges")
    cfg = R.RefConfig(**cfgd)
    P = {k: torch.from_numpy(v) for k, v in S.weights(cfgd, 3).items()}
    t = {k: torch.tensor(v) for k, v in b.items()}
    lg, pl = U.gqa_forward(P, cfg, t["feats"], t["pos7"], t["input_ids"], t["input_mask"], t["segment_ids"])
    lg2, pl2 = S.forward(P, cfg, t["feats"], t["pos7"], t["input_ids"], torch.from_numpy(S.key_mask(b)), t["segment_ids"])
    assert torch.equal(lg, lg2) and torch.equal(pl, pl2)


def test_gain_scales_weights_only():
    cfgd, _ = S.case_inputs("edges")
    w1, w3 = S.weights(cfgd, 1), S.weights(cfgd, 3)
    for k in w1:
        leaf = k.rsplit(".", 1)[-1]
        plain = "LayerNorm" in k or "layer_norm" in k or k.startswith("logit_fc.2.") or leaf == "bias"
        assert np.array_equal(w3[k], w1[k] if plain else w1[k] * np.float32(3)), k
    assert float(S.reference("max64", 3)["logits"].abs().max()) < 4.0        # not saturated


@pytest.mark.parametrize("case,gain", sorted({(c, g) for c, _, g in S.RUNS}))
def test_f32_oracle_passes_at_the_f32_bounds(case, gain):
    cfgd, b = S.case_inputs(case)
    got = S.oracle_run(cfgd, b, gain, dtype=torch.float32)
    ref = S.reference(case, gain)
    failed, worst = S.compare(got, ref, *S.START_BOUNDS["f32"])
    print("uniter sweep host %s gain %d: f32 oracle vs f64 oracle: logits %.3e pooled %.3e loss %.3e worst tensor %.3e (%s) zero-gradient norm %.3e"
          % (case, gain, worst["logits"], worst["pooled"], worst["loss"], worst["tensor"], worst["tensor_name"], worst["zero"]))
    assert not failed, failed


@functools.lru_cache(None)
def wrong_run(variant, case):
    cfgd, b = S.case_inputs(case)
    return S.oracle_run(cfgd, b, 3, **S.WRONG[variant](b))


@pytest.mark.parametrize("precision", S.PRECISIONS)
@pytest.mark.parametrize("variant", sorted(S.WRONG))
def test_wrong_variant_is_rejected(variant, precision):
    """on at least one gain-3 case the worst measured / bound ratio of the wrong oracle is >= 1.5, at the loosest bounds the sweep holds that case to in this
    precision (a raised bound in uniter_reference.RAISED_BOUNDS that breaks this must come down again: the case would no longer discriminate)"""
    best = 0.0
    for case in S.GAIN3_CASES:
        runs = [(c, p, g) for c, p, g in S.RUNS if c == case and g == 3]
        tol = max(S.bounds(c, p, g, precision)[0] for c, p, g in runs)
        gtol = max(S.bounds(c, p, g, precision)[1] for c, p, g in runs)
        failed, worst = S.compare(wrong_run(variant, case), S.reference(case, 3), tol, gtol)
        print("uniter sweep host %s on %s gain 3 at %s bounds (%.1e, %.1e): logits %.3e worst tensor %.3e (%s) ratio %.2f (%s), %d checks fail"
              % (variant, case, precision, tol, gtol, worst["logits"], worst["tensor"], worst["tensor_name"], worst["ratio"], worst["ratio_name"], len(failed)))
        if failed:
            best = max(best, worst["ratio"])
    assert best >= MARGIN, (variant, precision, best)


def test_raised_bounds_name_runs_of_the_sweep_and_stay_below_the_live_gradients():
    """a raised entry names a run of the sweep and raises, never lowers; the norm it allows a zero-gradient key bias stays below the ERROR the same bounds allow
    the smallest query-bias gradient of the case (gtol * its norm): the noise admitted where nothing should be is less than the error admitted next to it"""
    for key, (tol, gtol, ztol) in S.RAISED_BOUNDS.items():
        case, packed, gain, precision = key
        assert key[:3] in S.RUNS and precision in S.PRECISIONS, key
        t0, g0 = S.START_BOUNDS[precision]
        assert tol >= t0 and gtol >= g0 and ztol >= 1e-3 * g0, key
        grads = S.reference(case, gain)["grads"]
        floor = min(float(g.norm()) for k, g in grads.items() if k.endswith("attention.self.query.bias"))
        print("uniter sweep host raised %s: ztol %.3e, gtol * smallest query-bias gradient %.3e" % (key, ztol, gtol * floor))
        assert ztol < gtol * floor, (key, ztol, gtol * floor)


def test_compare_flags_a_missing_tensor_and_a_written_dead_range():
    ref = S.reference("one", 1)
    got = dict(ref, grads={k: v for k, v in ref["grads"].items() if k != "logit_fc.3.bias"})
    failed, _ = S.compare(got, ref, 1e-4, 1e-3)
    assert [f[0] for f in failed] == ["logit_fc.3.bias"]
    failed, _ = S.compare(ref, ref, 1e-4, 1e-3, dead=("logit_fc.3.bias",))
    assert [f[0] for f in failed] == ["logit_fc.3.bias (dead)"]
    failed, worst = S.compare(ref, ref, 1e-4, 1e-3)
    assert not failed and worst["ratio"] < 1e-3
