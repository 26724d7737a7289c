"""The UNITER shape sweep's reference side: the cases (configs, batches with explicit question lengths), the filler at a gain, the f64 oracle run with every
parameter gradient and the input gradients, four deliberately wrong variants of it, the starting bounds and ONE comparator.  Shared by
tests/test_uniter_sweep_host.py (which proves that the comparator at the sweep's bounds rejects the wrong variants) and tests/test_gpu_uniter_sweep.py (the
engine, arch 2, against the same oracle).  Runs on the CPU in the dtype it is asked for.  Not a test module."""
import functools

import numpy as np
import torch

from oracle import lxmert_ref as R
from oracle import uniter_ref as U
from rgqa_amd import synth
from rgqa_amd.synth import U_SMALL

PRECISIONS = ("f32", "bf16", "bf16x3", "bf16x3_fwd")

# head size 64: bf16 and split-f32 attention run the MFMA core; feature size 64: split-f32 rows are whole 128-byte lines
U_MED = dict(vocab_size=300, hidden=128, heads=2, inter=256, max_pos=64, type_vocab=2, l_layers=3, x_layers=0, r_layers=0, feat_dim=64, pos_dim=7, num_answers=9)
U_WIDE = dict(vocab_size=3000, hidden=768, heads=12, inter=3072, max_pos=64, type_vocab=2, l_layers=2, x_layers=0, r_layers=0, feat_dim=2048, pos_dim=7,
              num_answers=1842)

# name -> (config, B, T, O, explicit question lengths or None, seed)
CASES = {
    "one":     (U_MED, 1, 3, 1, None, 201),                       # single sample, single region: 4 rows
    "max64":   (U_MED, 5, 28, 36, (22, 1, 28, 2, 6), 202),        # the 64-row maximum; trimmed and untrimmed attention bodies in one launch
    "edges":   (U_MED, 6, 20, 12, (4, 5, 20, 19, 1, 2), 203),     # both sides of the 16- and 32-row tile edges
    "edges48": (U_MED, 4, 20, 28, (4, 5, 20, 19), 204),           # ... and of the 32- and 48-row ones
    "generic": (U_SMALL, 3, 8, 6, None, 92),                      # head size 16: the generic attention kernels
    "rows":    (U_MED, 37, 20, 36, None, 205),                    # 2072 padded rows: three 256-row slabs of text rows, 1332 region rows
    "width":   (U_WIDE, 24, 20, 36, None, 206),                   # the width-768 specialisations, split-K [CLS] GEMMs, the padded 1842-answer head
}
PACKED_ROWS = {"max64": (58, 37, 64, 38, 42), "edges": (16, 17, 32, 31, 13, 14), "edges48": (32, 33, 48, 47)}      # text tokens + regions per sample

# (case, packed, gain): packed rows everywhere; padded rows and the larger weights where the issue of this sweep asks for them (padded rows at gain 3 as well:
# only the padded layout HAS padding keys, so only there can a mask that opens one show)
RUNS = ([(c, True, 1) for c in CASES] + [(c, False, 1) for c in ("max64", "edges", "width")] + [(c, True, 3) for c in ("max64", "edges", "rows")]
        + [(c, False, 3) for c in ("max64", "edges")])
GAIN3_CASES = ("max64", "edges", "rows")

# (tol, gtol) as tests/test_gpu_engine.py test_shape_sweep_vs_oracle holds the LXMERT engine to; bf16x3_fwd: the bf16x3 forward, the bf16 backward
START_BOUNDS = {"f32": (2e-4, 3e-3), "bf16x3": (3e-4, 3e-3), "bf16": (2e-2, 4.5e-2), "bf16x3_fwd": (3e-4, 4.5e-2)}
# (case, packed, gain, precision) -> (tol, gtol, ztol) where a run exceeds a starting bound by rounding alone: 2 x the error measured on an MI355X against the
# f64 oracle, the measured value beside it and in docs/MEASUREMENTS.md "UNITER shape sweep".  Only ztol - the norm allowed to a key-bias gradient, whose true
# value is zero - is raised anywhere.  The starting 1e-3 * gtol is an ABSOLUTE norm, and what the bf16 backward leaves there is relative: the attention backward
# rounds dS = P (dP - delta) to bf16 before dK = dS^T Q, so sum_key dS[q][key] is no longer 0 but about 2^-9 of its terms, and the key bias collects
# sum_q Q[q] * that.  Measured, it is 1e-3 (bf16) to 2e-3 (bf16x3_fwd, whose backward also reads bf16 images of Q and K) of the norm of the same layer's
# query-bias gradient at gain 1 and at gain 3 alike; that gradient is 110 times larger at gain 3 and 1300 times larger at width 768 than at the medium config
# with the filler, and the noise with it.  tests/test_uniter_sweep_host.py caps every entry.
_T16, _TX = START_BOUNDS["bf16"], START_BOUNDS["bf16x3_fwd"]
RAISED_BOUNDS = {
    ("width", True, 1, "bf16"):              _T16 + (4.268e-04,),      # observed: 2.134e-04
    ("width", True, 1, "bf16x3_fwd"):        _TX + (1.094e-03,),      # observed: 5.470e-04
    ("width", False, 1, "bf16"):             _T16 + (4.580e-04,),      # observed: 2.290e-04
    ("width", False, 1, "bf16x3_fwd"):       _TX + (1.306e-03,),      # observed: 6.530e-04
    ("max64", True, 3, "bf16"):              _T16 + (1.429e-04,),      # observed: 7.147e-05
    ("max64", True, 3, "bf16x3_fwd"):        _TX + (3.194e-04,),      # observed: 1.597e-04
    ("max64", False, 3, "bf16"):             _T16 + (1.429e-04,),      # observed: 7.147e-05
    ("max64", False, 3, "bf16x3_fwd"):       _TX + (2.256e-04,),      # observed: 1.128e-04
    ("edges", True, 3, "bf16"):              _T16 + (1.730e-04,),      # observed: 8.652e-05
    ("edges", True, 3, "bf16x3_fwd"):        _TX + (2.866e-04,),      # observed: 1.433e-04
    ("edges", False, 3, "bf16"):             _T16 + (1.730e-04,),      # observed: 8.652e-05
    ("edges", False, 3, "bf16x3_fwd"):       _TX + (2.342e-04,),      # observed: 1.171e-04
    ("rows", True, 3, "bf16x3_fwd"):         _TX + (2.334e-04,),      # observed: 1.167e-04
}


def bounds(case, packed, gain, precision):
    """(tol, gtol, ztol) of uniter_reference.compare for a run of the sweep"""
    tol, gtol = START_BOUNDS[precision]
    return RAISED_BOUNDS.get((case, packed, gain, precision), (tol, gtol, 1e-3 * gtol))


def _set_lengths(b, lens, vocab):
    """question b gets lens[b] tokens: [CLS] body ... [SEP], zeros behind (the prefix masks the tokenizer builds); one token: [CLS] alone"""
    B, T = b["input_ids"].shape
    cls_id, sep_id = (101, 102) if vocab > 200 else (2, 3)
    body = 5 + (synth.hash_u32("uniter_sweep.ids", B * T) % np.uint64(vocab - 5)).astype(np.int64).reshape(B, T)
    ids = np.zeros((B, T), dtype=np.int64)
    for i, L in enumerate(lens):
        ids[i, :L] = body[i, :L]
        ids[i, L - 1] = sep_id
        ids[i, 0] = cls_id
    b["input_ids"] = ids
    b["input_mask"] = (ids != 0).astype(np.int64)
    b["lengths"] = np.asarray(lens, dtype=np.int64)


@functools.lru_cache(None)
def case_inputs(name):
    """-> (cfgd, batch of numpy arrays: feats, pos7, input_ids, input_mask, segment_ids, target, lengths = text tokens per sample).  Shared: do not modify."""
    cfgd, B, T, O, lens, seed = CASES[name]
    b = synth.uniter_batch(cfgd, T, B, O, seed)
    if lens is not None:
        _set_lengths(b, lens, cfgd["vocab_size"])
    b["lengths"] = b["input_mask"].sum(1).astype(np.int64)
    assert (b["input_mask"] == (np.arange(T)[None, :] < b["lengths"][:, None])).all(), "question masks must be prefixes"
    for v in b.values():
        v.setflags(write=False)
    return cfgd, b


def packed_rows(batch):
    return tuple(int(v) + batch["feats"].shape[1] for v in batch["lengths"])


def weights(cfgd, gain):
    """{state_dict key: f32 array}: the deterministic filler with every Linear / embedding weight times `gain`; LayerNorm parameters, biases and logit_fc.2.* as
    they are (the rule of synth.maha_fill).  The engine's arena is filled from these arrays."""
    out = synth.fill_state_dict(U.param_shapes(R.RefConfig(**cfgd)))
    for k, v in out.items():
        leaf = k.rsplit(".", 1)[-1]
        parent = k.rsplit(".", 2)[-2] if k.count(".") >= 1 else ""
        if "LayerNorm" in parent or "layer_norm" in parent or k.startswith("logit_fc.2.") or leaf == "bias":
            continue
        out[k] = (v * np.float32(gain)).astype(np.float32)
    return out


@functools.lru_cache(None)
def case_weights(case, gain):
    """weights(config of the case, gain), made once and shared: do not modify"""
    return weights(CASES[case][0], gain)


# ------------------------------------------------------------------------------------------------ the oracle and its wrong variants
def key_mask(batch):
    """[B, T + O] the keys every query may attend to: the question's real tokens and every region (uniter/entry.py:85-101)"""
    B, O = batch["feats"].shape[:2]
    return np.concatenate([batch["input_mask"], np.ones((B, O), dtype=np.int64)], 1)


def _mask_first_pad_open(batch):
    m = key_mask(batch).copy()
    T = batch["input_ids"].shape[1]
    for i, L in enumerate(batch["lengths"]):
        if L < T:
            m[i, L] = 1
    return m


def _mask_last_region_closed(batch):
    m = key_mask(batch).copy()
    m[:, -1] = 0
    return m


# the mistakes a UNITER front end or a mask edge can make: name -> keyword arguments of oracle_run for a batch
WRONG = {
    "first_pad_key_open": lambda batch: dict(mask_override=_mask_first_pad_open(batch)),
    "last_region_key_masked": lambda batch: dict(mask_override=_mask_last_region_closed(batch)),
    "pos_w_h_swapped": lambda batch: dict(pos_swap=(4, 5)),
    "no_type1_on_regions": lambda batch: dict(zero_type1=True),
}


def forward(P, cfg, feats, pos7, input_ids, mask, segment_ids, pos_swap=None, zero_type1=False):
    """oracle.uniter_ref.gqa_forward with the key mask [B, T + O] as an argument and the two front-end mistakes as options; with mask = key_mask(batch) and no
    option it is that function statement by statement (tests/test_uniter_sweep_host.py holds the two to equal bits)"""
    B, O = feats.shape[:2]
    ext = (1.0 - mask.unsqueeze(1).unsqueeze(2).to(torch.float32)) * -10000.0
    txt = U.text_embeddings(P, cfg, input_ids, segment_ids)
    type1 = torch.nn.functional.embedding(torch.ones(B, O, dtype=torch.long), P[U.PRE + "embeddings.token_type_embeddings.weight"])
    if zero_type1:
        type1 = torch.zeros_like(type1)
    if pos_swap is not None:
        cols = list(range(pos7.shape[2]))
        cols[pos_swap[0]], cols[pos_swap[1]] = cols[pos_swap[1]], cols[pos_swap[0]]
        pos7 = pos7[:, :, cols]
    x = torch.cat([txt, U.image_embeddings(P, cfg, feats, pos7, type1)], 1)
    for i in range(cfg.l_layers):
        x = R.bert_layer(P, U.PRE + "encoder.layer.%d" % i, cfg, x, ext)
    pooled = torch.tanh(R.linear(x[:, 0], P, U.PRE + "pooler.dense"))
    return R.head_forward(P, cfg, pooled), pooled


def oracle_run(cfgd, batch, gain, dtype=torch.float64, mask_override=None, pos_swap=None, zero_type1=False):
    """One forward + BCE x NA backward of the oracle on the CPU in `dtype`.  -> dict(logits [B, NA], pooled [B, H], loss (float), grads {key: tensor}, dfeats
    [B, O, F], dpos [B, O, 7]), every tensor in `dtype`.  dpos is the gradient w.r.t. the pos7 array as given (a column swap happens inside)."""
    cfg = R.RefConfig(**cfgd)
    P = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in weights(cfgd, gain).items()}
    feats = torch.tensor(batch["feats"]).to(dtype).requires_grad_(True)
    pos7 = torch.tensor(batch["pos7"]).to(dtype).requires_grad_(True)
    mask = torch.from_numpy(np.ascontiguousarray(key_mask(batch) if mask_override is None else mask_override))
    logits, pooled = forward(P, cfg, feats, pos7, torch.tensor(batch["input_ids"]), mask, torch.tensor(batch["segment_ids"]), pos_swap, zero_type1)
    loss = R.bce_loss(logits, torch.tensor(batch["target"]).to(dtype))
    loss.backward()
    return dict(logits=logits.detach(), pooled=pooled.detach(), loss=float(loss.detach()), grads={k: p.grad for k, p in P.items()}, dfeats=feats.grad, dpos=pos7.grad)


@functools.lru_cache(None)
def reference(case, gain):
    """the f64 oracle's result for a case, computed once and shared: do not modify"""
    cfgd, b = case_inputs(case)
    return oracle_run(cfgd, b, gain)


# ------------------------------------------------------------------------------------------------ the comparator
def compare(got, ref, tol, gtol, ztol=None, dead=()):
    """got / ref: dicts as oracle_run returns them (`got` in any dtype, gradients in any shape of the right size; a parameter gradient or an input gradient that
    `got` lacks is a failure).  `dead`: keys whose range no backward ever writes.  -> (failed, worst):
      failed  list of (what, measured, bound) - empty when everything holds;
      worst   dict(logits, pooled, loss, tensor = largest relative Frobenius error over the live gradient tensors and dfeats / dpos, tensor_name, zero = largest
              norm of a tensor whose true gradient is zero, ratio = largest measured / bound over all of these, ratio_name).
    Rules: logits and pooled max abs error < tol * max(1, max |ref|); loss error < 50 * tol * max(1, |ref|) (tests/test_gpu_engine.py test_shape_sweep_vs_oracle);
    live gradient tensors, dfeats, dpos: |got - ref|_F / |ref|_F < gtol; true gradient zero (|ref|_F < 1e-8: the key biases - softmax is shift-invariant):
    |got|_F < ztol (default 1e-3 * gtol); dead ranges exactly 0."""
    ztol = 1e-3 * gtol if ztol is None else ztol
    failed = []
    worst = dict(logits=0.0, pooled=0.0, loss=0.0, tensor=0.0, tensor_name="", zero=0.0, ratio=0.0, ratio_name="")

    def hold(what, measured, bound, slot):
        measured = float(measured)
        if not measured < bound:
            failed.append((what, measured, bound))
        if slot == "tensor" and measured >= worst["tensor"]:
            worst["tensor"], worst["tensor_name"] = measured, what
        elif slot != "tensor":
            worst[slot] = max(worst[slot], measured)
        r = measured / bound if np.isfinite(measured) else float("inf")
        if r >= worst["ratio"]:
            worst["ratio"], worst["ratio_name"] = r, what

    for k in ("logits", "pooled"):
        r = ref[k].double()
        hold(k, (got[k].double().reshape(r.shape) - r).abs().max(), tol * max(1.0, float(r.abs().max())), k)
    hold("loss", abs(float(got["loss"]) - ref["loss"]), 50 * tol * max(1.0, abs(ref["loss"])), "loss")
    tensors = [(k, got["grads"].get(k), r) for k, r in ref["grads"].items()] + [(k, got.get(k), ref[k]) for k in ("dfeats", "dpos")]
    for k, g, r in tensors:
        if g is None:
            failed.append((k, float("nan"), 0.0))
            continue
        g, r = g.double().reshape(-1), r.double().reshape(-1)
        if g.numel() != r.numel():
            failed.append((k + " (size)", float(g.numel()), float(r.numel())))
            continue
        if k in dead:
            if float(g.abs().max()) != 0.0:
                failed.append((k + " (dead)", float(g.abs().max()), 0.0))
            continue
        den = float(r.norm())
        if den < 1e-8:
            hold(k, g.norm(), ztol, "zero")
        else:
            hold(k, (g - r).norm() / den, gtol, "tensor")
    return failed, worst
