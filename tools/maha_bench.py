"""Per-batch time of the Mahalanobis scorer (rgqa_amd.scoring.maha_scores; the reference's tasks/gqa_maha.py:223-270) through the drop-in
`GQAModel_maha` / `GQAUNITER_maha` / `GQABUTD_maha` (hidden 1024, built as tools/odin_bench.py builds its BUTD model), full configuration, NC = 1842, at the reference's test batch (32, scripts/*/test/maha.sh) and at 256.  Legs
alternate in one process after a warm-up, each window bracketed by device synchronisation:

    fwd        the second forward (no_grad)
    fwd_bwd    the first forward + backward from d loss / d pooled with feats / boxes requiring grad
    scorer     the three scorer calls on a pooled vector: maha_score_rows, maha_dpooled, maha_score_rows
    fused      scoring.maha_scores
    pasted     the reference's statements (gqa_maha.py:223-270: a torch loop over the classes, twice per batch) on the same drop-in model
    pasted_loops   their two class loops and the loss statements alone, on a pooled vector (what `scorer` replaces)
    update     MahaEstimator.update on one batch (the estimator's per-batch cost next to `fwd`; reported at every batch size)

    timeout 900 python tools/maha_bench.py [--backbones lxmert,uniter,butd] [--precisions bf16x3_fwd] [--batches 32,256] [--only-leg fused]

Prints one JSON line per (backbone, precision, batch): median ms per batch of each leg over the windows.  Not part of bench.py."""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import odin_bench as OB                                               # noqa: E402
from tests.maha_reference import class_loop, ood_batch                # noqa: E402  (the reference's statements, one copy)

NC = 1842


def make_model(backbone, precision):
    os.environ["RGQA_PRECISION"] = precision
    margs = types.SimpleNamespace(llayers=9, xlayers=5, rlayers=5, from_scratch=True)
    if backbone == "lxmert":
        from rgqa_amd.tasks.gqa_model import GQAModel_maha
        return GQAModel_maha(NC, max_seq_length=20, model_args=margs).cuda().eval()
    if backbone == "uniter":
        from rgqa_amd.uniter.uniter import GQAUNITER_maha
        return GQAUNITER_maha(NC, model_args=margs).cuda().eval()
    from rgqa_amd.butd.butd import GQABUTD_maha
    from rgqa_amd.butd.preprocess import Dictionary
    d = Dictionary()
    for i in range(3000):
        d.add_word(OB.WORDS[i] if i < len(OB.WORDS) else "w%d" % i)
    return GQABUTD_maha(NC, d, dropout=False, precision=precision).cuda().train()      # the reference scores BUTD in train() (gqa_maha.py:205-206)


def make_pack(model, feats, boxes, sent, seed=0):
    """class means scattered around the model's own pooled vectors (H = 768; BUTD: joint_repr, H = 1024), a covariance of condition 1e2 with random axes"""
    from rgqa_amd import scoring
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        x = model(feats, boxes, sent)[1].cpu().numpy()
    H = x.shape[1]
    Q, _ = np.linalg.qr(rng.standard_normal((H, H)))
    lam = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), H))
    mean = (x[rng.randint(0, len(x), NC)] + 0.05 * rng.standard_normal((NC, H))).astype(np.float32)
    mean[rng.choice(NC, 40, replace=False)] = 0.0
    return scoring.maha_pack(mean, (Q / lam) @ Q.T)


def run_case(backbone, precision, B, noise, windows, iters, only):
    from rgqa_amd import scoring
    model = make_model(backbone, precision)
    feats, boxes, sent = OB.make_batch(backbone, B)
    pack = make_pack(model, feats, boxes, sent)
    with torch.no_grad():
        x = model(feats, boxes, sent)[1].clone()
    rows = scoring.maha_score_rows(x, pack)
    dp = scoring.maha_dpooled(rows, pack)
    target = torch.zeros(B, NC, device="cuda")
    target[torch.arange(B), torch.randint(0, NC, (B,), generator=torch.Generator().manual_seed(1))] = 1.0
    est = scoring.MahaEstimator(NC, x.shape[1])

    def leg_fwd():
        with torch.no_grad():
            model(feats, boxes, sent)

    def leg_fwd_bwd():
        f, b = feats.detach().requires_grad_(True), boxes.detach().requires_grad_(True)
        model(f, b, sent)[1].backward(dp)

    def leg_scorer():
        r = scoring.maha_score_rows(x, pack)
        scoring.maha_dpooled(r, pack)
        scoring.maha_score_rows(x, pack)

    def leg_fused():
        scoring.maha_scores(model, feats, boxes, sent, pack, noise)

    def leg_pasted():
        ood_batch(model, feats.detach(), boxes.detach(), sent, pack.mean, pack.precision, NC, noise)

    def leg_pasted_loops():
        g = class_loop(x, pack.mean, pack.precision, NC)
        zero_f = x - pack.mean.index_select(0, g.max(1)[1])
        torch.mean(0.5 * torch.mm(torch.mm(zero_f, pack.precision), zero_f.t()).diag())
        torch.max(class_loop(x, pack.mean, pack.precision, NC), dim=1)

    def leg_update():
        est.update(x, target)
    legs = {"fwd": leg_fwd, "fwd_bwd": leg_fwd_bwd, "scorer": leg_scorer, "fused": leg_fused, "pasted": leg_pasted, "pasted_loops": leg_pasted_loops, "update": leg_update}
    slow = ("pasted", "pasted_loops")
    if only:
        legs = {only: legs[only]}
    for k, fn in legs.items():
        for _ in range(1 if k in slow else 3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            n = max(1, iters // 5) if k in slow else iters
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / n)
    out = dict(backbone=backbone, precision=precision, batch=B, classes=NC, rank=int(pack.W.shape[1]), noise=noise, windows=windows, iters=iters)
    for k, v in times.items():
        out["%s_ms" % k] = round(float(np.median(v)), 4)
        out["%s_ms_min_max" % k] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    if "fused" in times and "pasted" in times:
        out["pasted_over_fused"] = round(out["pasted_ms"] / out["fused_ms"], 2)
    if "scorer" in times and "fwd" in times:
        out["scorer_over_fwd"] = round(out["scorer_ms"] / out["fwd_ms"], 4)
    print(json.dumps(out), flush=True)
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbones", default="lxmert")
    ap.add_argument("--precisions", default="bf16x3_fwd")
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--noise", type=float, default=1e-4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-leg", default="", choices=["", "fwd", "fwd_bwd", "scorer", "fused", "pasted", "pasted_loops", "update"], help="one leg alone (what runs under a kernel trace)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="rgqa_maha_bench_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        os.environ["RGQA_BERT_VOCAB"] = OB.write_vocab(tmp)
        for bb in a.backbones.split(","):
            for prec in a.precisions.split(","):
                for B in (int(x) for x in a.batches.split(",")):
                    run_case(bb, prec, B, a.noise, a.windows, a.iters, a.only_leg)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
