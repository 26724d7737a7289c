"""Per-batch time of the ODIN scorer (rgqa_amd.scoring.odin_scores; the reference's tasks/gqa_odin.py:97-131) through the drop-in classes of
the three backbones, at the reference's test batch (32, scripts/*/test/odin.sh) and at 256.  Three legs alternate in one process after a
warm-up, each window bracketed by device synchronisation:

    (a) forward + backward, no input gradients       model(feats, boxes, sent); logit.backward(dl)
    (b) the same with feats / boxes requiring grad   (+ the dgrad GEMM and the finishing kernel / the pos_linear dgrad)
    (c) scoring.odin_scores                          (b) + score_rows, odin_dlogits, two sign_steps, the second forward, score_rows

    timeout 600 python tools/odin_bench.py [--backbones butd,lxmert,uniter] [--precisions bf16x3_fwd,bf16] [--batches 32,256] [--only-leg c]

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

WORDS = ["what", "is", "the", "color", "of", "dog", "man", "woman", "left", "right", "to", "on", "in", "front", "behind", "table", "holding", "bottle",
         "red", "blue", "green", "who", "wearing", "shirt", "are", "there", "any", "cars", "photo", "side", "which", "kind", "animal", "standing", "near", "tree"]


def write_vocab(tmp):
    vocab = ["[unused%d]" % i for i in range(30522)]
    vocab[0], vocab[100], vocab[101], vocab[102], vocab[103] = "[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"
    vocab[1029] = "?"
    for i, w in enumerate(WORDS):
        vocab[2000 + i] = w
    path = os.path.join(tmp, "vocab.txt")
    with open(path, "w") as f:
        f.write("\n".join(vocab) + "\n")
    return path


def make_model(backbone, precision, NA=1842):
    os.environ["RGQA_PRECISION"] = precision
    margs = types.SimpleNamespace(llayers=9, xlayers=5, rlayers=5, from_scratch=True)
    if backbone == "lxmert":
        from rgqa_amd.tasks.gqa_model import GQAModel
        return GQAModel(NA, max_seq_length=20, model_args=margs).cuda().eval()
    if backbone == "uniter":
        from rgqa_amd.uniter.uniter import GQAUNITER
        return GQAUNITER(NA, model_args=margs).cuda().eval()
    from rgqa_amd.butd.butd import GQABUTD
    from rgqa_amd.butd.preprocess import Dictionary
    d = Dictionary()
    for i in range(3000):
        d.add_word(WORDS[i] if i < len(WORDS) else "w%d" % i)
    return GQABUTD(NA, d, dropout=False, precision=precision).cuda().train()      # the reference scores BUTD in train() (gqa_odin.py:87-88)


def make_batch(backbone, B, seed=5):
    rng = np.random.RandomState(seed)
    feats = torch.from_numpy(np.maximum(rng.standard_normal((B, 36, 2048)), 0).astype(np.float32)).cuda()
    xy = np.sort(rng.uniform(0, 1, (B, 36, 2, 2)), axis=3)
    box = np.stack([xy[:, :, 0, 0], xy[:, :, 1, 0], xy[:, :, 0, 1], xy[:, :, 1, 1]], -1).astype(np.float32)
    if backbone == "uniter":
        w, h = box[..., 2] - box[..., 0], box[..., 3] - box[..., 1]
        box = np.concatenate([box, np.stack([w, h, w * h], -1)], -1).astype(np.float32)
    sent = [" ".join(WORDS[int(rng.randint(0, len(WORDS)))] for _ in range(3 + int(rng.randint(0, 14)))) + " ?" for _ in range(B)]
    return feats, torch.from_numpy(box).cuda(), sent


def run_case(backbone, precision, B, temperature, noise, windows, iters, only):
    from rgqa_amd import scoring
    model = make_model(backbone, precision)
    feats, boxes, sent = make_batch(backbone, B)
    with torch.no_grad():
        lg = model(feats, boxes, sent)
    s = scoring.score_rows(lg, temperature)
    dl, _ = scoring.odin_dlogits(lg, s.label, s.max_score)

    def leg_a():
        model(feats, boxes, sent).backward(dl)

    def leg_b():
        f, b = feats.detach().requires_grad_(True), boxes.detach().requires_grad_(True)
        model(f, b, sent).backward(dl)

    def leg_c():
        scoring.odin_scores(model, feats, boxes, sent, temperature, noise)
    legs = {"a": leg_a, "b": leg_b, "c": leg_c}
    if only:
        legs = {only: legs[only]}
    for fn in legs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / iters)
    out = dict(backbone=backbone, precision=precision, batch=B, temperature=temperature, noise=noise, windows=windows, iters=iters)
    for k, v in times.items():
        out["leg_%s_ms" % k] = round(float(np.median(v)), 4)
        out["leg_%s_ms_min_max" % k] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    print(json.dumps(out), flush=True)
    del model
    torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--backbones", default="butd,lxmert,uniter")
    ap.add_argument("--precisions", default="bf16x3_fwd,bf16")
    ap.add_argument("--batches", default="32,256")
    ap.add_argument("--temperature", type=float, default=1e5)
    ap.add_argument("--noise", type=float, default=1e-4)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--only-leg", default="", choices=["", "a", "b", "c"], help="one leg alone (what runs under a kernel trace)")
    a = ap.parse_args()
    tmp = tempfile.mkdtemp(prefix="rgqa_odin_bench_", dir=os.environ.get("TMPDIR", "/tmp"))
    try:
        os.environ["RGQA_BERT_VOCAB"] = write_vocab(tmp)
        for bb in a.backbones.split(","):
            for prec in a.precisions.split(","):
                for B in (int(x) for x in a.batches.split(",")):
                    run_case(bb, prec, B, a.temperature, a.noise, a.windows, a.iters, a.only_leg)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


if __name__ == "__main__":
    main()
