"""The bf16x3_fwd precision on the BUTD engine (rgqa_config.arch = 1, BASELINE config 5): the bf16x3 engine's split-f32 forward pass - with the
GRU recurrence as one persistent split-f32 launch (csrc/butd_gru.hip gru_fwd_persist_x3_kernel) - and the bf16 engine's backward pass, against the
golden fixture of the reference's GQABUTD, the oracle, the bf16x3 engine and the host-driven recurrence."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgqa_amd.synth import BUTD_WORDS, BUTD_SENTS, sample_idx     # noqa: E402
from rgqa_amd import synth                                           # noqa: E402
from tests import test_gpu_butd as TGB                             # noqa: E402
from tests.test_gpu_butd import build                                # noqa: E402

P = "bf16x3_fwd"
L, O, NA, NT = 40, 36, 1842, 3000


def test_butd_x3fwd_vs_reference_golden(golden_dir):
    """G7 through the drop-in GQABUTD: logits and attention as the bf16x3 row of test_butd_vs_reference_golden, gradients as its bf16 row."""
    g = np.load(os.path.join(golden_dir, "g7_butd.npz"))
    m, c, filled = build(P)
    b = synth.synth_batch(len(BUTD_SENTS), 8, O=36, F=2048, NA=23, vocab=64, seed=606, uq_frac=0.2)
    feat, pos, target = (torch.from_numpy(b[k]).cuda() for k in ("feats", "boxes", "target"))
    assert np.array_equal(m.tokenize(BUTD_SENTS).numpy(), g["toks"])
    m.eval()
    logits, att = m(feat, pos, BUTD_SENTS, attention=True)
    lerr = np.abs(logits.detach().cpu().numpy() - g["logits"]).max()
    aerr = np.abs(att.cpu().numpy() - g["att"]).max()
    print("butd %s: logits max err %.3e, att max err %.3e" % (P, lerr, aerr))
    assert lerr <= 1e-3 and aerr <= 2.5e-4
    loss = torch.nn.BCEWithLogitsLoss()(logits, target) * logits.size(1)
    np.testing.assert_allclose(loss.item(), g["loss"], rtol=50 * 1e-3 / 15)
    loss.backward()
    gtol = 6e-2       # the bf16 row: the backward pass is the bf16 engine's
    wn = ws = 0.0
    for k, p in m.named_parameters():
        gr = p.grad.cpu().numpy()
        ref_norm = float(g["gnorm." + k])
        ref = g["gsamp." + k]
        got = gr.reshape(-1)[sample_idx(k, gr.size)]
        wn = max(wn, abs(np.sqrt((gr.astype(np.float64) ** 2).sum()) - ref_norm) / max(ref_norm, 1e-12))
        ws = max(ws, float(np.abs(got - ref).max() / max(np.abs(ref).max(), 1e-6)))
        assert abs(np.sqrt((gr.astype(np.float64) ** 2).sum()) - ref_norm) <= gtol * ref_norm + 1e-7, k
        assert np.abs(got - ref).max() <= 3 * gtol * max(np.abs(ref).max(), 1e-6) + 1e-7, k
    print("butd %s: worst gradient-norm rel err %.3e, worst sampled-entry err / max %.3e, loss rel %.3e" % (P, wn, ws, abs(loss.item() - g["loss"]) / abs(g["loss"])))
    assert float(dict(m.named_parameters())["w_emb.emb.weight"].grad[-1].abs().max()) == 0.0


def test_butd_x3fwd_step_at_config5_size_vs_oracle():
    """B = 256, 40 tokens, 3000 words, 1842 answers against the oracle: logits and loss as the bf16x3 row; gradients at about twice the observed
    error (all tensors 1.8e-3, worst tensor - the word table - 6.0e-3 on an MI355X), far inside the bf16 row's gtol 8e-2."""
    TGB.test_butd_step_at_config5_size_vs_oracle(P, 1e-3, 1e-2, 1.2e-2)


def _batch(B, seed):
    b = synth.synth_batch(B, L, seed=seed, uq_frac=0.25, vocab=NT)
    rng = np.random.RandomState(seed + 1)
    toks = np.full((B, L), NT, dtype=np.int64)
    for r in range(B):
        n = int(rng.randint(1, L + 1)) if r else L
        toks[r, L - n:] = rng.randint(0, NT, size=n)
    return b, toks


def _engine(precision, filled, B):
    from rgqa_amd.engine import Engine
    e = Engine(arch=1, vocab_size=NT + 1, hidden=1024, emb_dim=300, feat_dim=2048, pos_dim=4, num_answers=NA, precision=precision,
               hidden_dropout=0.0, attn_dropout=0.0, heads=1, inter=8, l_layers=0, x_layers=0, r_layers=0).allocate("cuda")
    for sp in e.specs:
        e.view(e.params, sp).copy_(torch.from_numpy(np.asarray(filled[sp.name]).reshape(sp.shape)))
    e.ensure_shape(B, L, O)
    e.sync_weights()
    return e


def _filled():
    from oracle import butd_ref as BR
    from tests.test_oracle_golden import butd_fill
    c = BR.ButdConfig(ntoken=NT, num_answers=NA)
    return c, butd_fill(c)


def test_butd_x3fwd_forward_is_the_bf16x3_forward():
    """With the host-driven recurrence (key 18 = 0) the mixed engine's forward pass is the bf16x3 engine's, kernel for kernel: same logits, same loss."""
    from rgqa_amd import _lib
    L_ = _lib.load()
    B = 70
    _, filled = _filled()
    b, toks = _batch(B, 31)
    fg, pg, tg, kg = (torch.from_numpy(x).cuda() for x in (b["feats"], b["boxes"], b["target"], toks))
    res = {}
    try:
        assert L_.rgqa_debug_set(18, 0) == 0
        for prec in ("bf16x3", P):
            e = _engine(prec, filled, B)
            lg = e.forward(fg, pg, kg, kg, None, train=False)[0].clone()
            loss = e.loss_backward(tg).clone()
            torch.cuda.synchronize()
            res[prec] = (lg, loss)
            del e
    finally:
        L_.rgqa_debug_set(18, 3)
    assert torch.isfinite(res[P][0]).all()
    assert torch.equal(res[P][0], res["bf16x3"][0]) and torch.equal(res[P][1], res["bf16x3"][1])


@pytest.mark.parametrize("B", [5, 70, 256])
def test_butd_x3fwd_gru_forms_agree(B):
    """The mixed engine's forward recurrence as one persistent split-f32 launch (key 18 = 3) and as the host-driven loop (0), on batch sizes that end
    inside a 32-sample row group: each form bit-reproducible over two passes (a counter left behind would show), logits equal up to the order of
    the f32 sums, gradients to bf16 rounding."""
    from rgqa_amd import _lib
    L_ = _lib.load()
    _, filled = _filled()
    b, toks = _batch(B, 99)
    fg, pg, tg, kg = (torch.from_numpy(x).cuda() for x in (b["feats"], b["boxes"], b["target"], toks))
    res = {}
    try:
        for form in (0, 3):
            assert L_.rgqa_debug_set(18, form) == 0
            e = _engine(P, filled, B)
            out = []
            for _ in range(2):
                lg = e.forward(fg, pg, kg, kg, None, train=False)[0].clone()
                e.loss_backward(tg)
                out.append((lg, e.grads.clone()))
            torch.cuda.synchronize()
            assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1]), form
            res[form] = out[0]
            del e
    finally:
        L_.rgqa_debug_set(18, 3)
    (l0, g0), (l3, g3) = res[0], res[3]
    assert torch.isfinite(l0).all() and torch.isfinite(g0).all() and float(g0.abs().max()) > 0
    assert torch.isfinite(l3).all() and torch.isfinite(g3).all()
    lerr = float((l3 - l0).abs().max())
    grel = float((g3 - g0).norm()) / float(g0.norm())
    print("butd %s B=%d: persistent vs host-driven recurrence: logits max diff %.3e (|logits| max %.3e), gradients rel %.3e" % (
        P, B, lerr, float(l0.abs().max()), grel))
    assert lerr < 1e-7 * max(1.0, float(l0.abs().max()))      # observed 3.7e-9 at B = 5, 70 and 256 (|logits| <= 0.05)
    assert grel < 3e-2                                          # bf16 tolerance (observed <= 2e-9: the bf16 images of h_t rarely differ)


def test_butd_x3fwd_above_the_persistent_range_vs_oracle():
    """B = 260 (past the persistent launch's 256): the host-driven split-f32 recurrence, logits within 1e-3 of the oracle."""
    from oracle import butd_ref as BR
    B = 260
    c, filled = _filled()
    b, toks = _batch(B, 515)
    e = _engine(P, filled, B)
    fg, pg, kg = (torch.from_numpy(x).cuda() for x in (b["feats"], b["boxes"], toks))
    lg = e.forward(fg, pg, kg, kg, None, train=False)[0].clone()
    torch.cuda.synchronize()
    torch.set_num_threads(max(1, min(32, len(os.sched_getaffinity(0)))))
    Pm = {k: torch.from_numpy(np.asarray(v)).clone() for k, v in filled.items()}
    with torch.no_grad():
        lo = BR.butd_forward(Pm, c, torch.from_numpy(b["feats"]), torch.from_numpy(b["boxes"]), torch.from_numpy(toks))
    err = float((lg.cpu() - lo).abs().max())
    print("butd %s B=%d: logits max err %.3e (|logits| max %.3e)" % (P, B, err, float(lo.abs().max())))
    assert torch.isfinite(lg).all()
    assert err < min(1e-3, 1e-2 * float(lo.abs().max()))


def _train(seed):
    from rgqa_amd.lxrt.optimization import BertAdam
    torch.manual_seed(seed)
    m, c, _ = build(P, dropout=True)
    b = synth.synth_batch(len(BUTD_SENTS), 8, O=36, F=2048, NA=23, vocab=64, seed=607)
    feat, pos, target = (torch.from_numpy(b[k]).cuda() for k in ("feats", "boxes", "target"))
    opt = BertAdam(list(m.parameters()), lr=1e-3, warmup=0.1, t_total=10)
    m.train()
    losses = []
    for _ in range(4):
        opt.zero_grad()
        logit = m(feat, pos, BUTD_SENTS)
        loss = torch.nn.BCEWithLogitsLoss()(logit, target) * logit.size(1)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(m.parameters(), 5.)
        opt.step()
        losses.append(loss.item())
    torch.cuda.synchronize()
    return losses, {k: p.detach().clone() for k, p in m.named_parameters()}


def test_butd_x3fwd_train_steps_with_dropout_are_reproducible():
    la, pa = _train(1234)
    lb, pb = _train(1234)
    assert all(np.isfinite(la)) and la[-1] < la[0]
    assert la == lb
    assert all(torch.isfinite(pa[k]).all() and torch.equal(pa[k], pb[k]) for k in pa)


@pytest.mark.parametrize("backend,world", [("nccl", 1), ("gloo", 2)])
def test_butd_x3fwd_under_the_sharded_exchange(backend, world):
    """The data-parallel exchange around the mixed BUTD engine (bf16 payload): ranks agree bit for bit, and two optimizer steps are the plain step
    on the whole batch within the bounds of the bf16 rows of test_butd_engine_under_the_exchange."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _butd_batch, _make_butd, _butd_step, _butd_worker
    from rgqa_amd.parallel import exchange_payload
    assert exchange_payload("sharded", P) == torch.bfloat16
    e, d = _make_butd(_butd_batch(), P)
    for _ in range(2):
        _butd_step(e, d, None, 1)
    ref = e.params.cpu().numpy()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 28800 + (os.getpid() % 500) + 7 * world
    procs = [ctx.Process(target=_butd_worker, args=(r, world, port, backend, "sharded", P, q), daemon=True) for r in range(world)]
    for p in procs:
        p.start()
    res = {}
    try:
        for _ in range(world):
            r, params = q.get(timeout=240)
            res[r] = params
        for p in procs:
            p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.terminate()
    assert all(p.exitcode == 0 for p in procs)
    if world == 2:
        assert np.array_equal(res[0], res[1])
    diff = np.abs(res[0] - ref)
    print("butd dp %s x%d sharded/%s: |params - plain step| max %.3e mean %.3e" % (backend, world, P, diff.max(), diff.mean()))
    assert np.isfinite(res[0]).all()
    assert diff.max() < 1.3e-2 and diff.mean() < 1e-5, (diff.max(), diff.mean())
