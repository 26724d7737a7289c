"""Generator of tests/golden/g13_maha.npz - runs ONLY where the reference checkout exists (like oracle/gen_golden.py, whose import path and
stand-in modules it reuses) and sklearn is installed; only the .npz is committed.

The reference's own LXMERT (the G1 small config) and UNITER (small) modules, with the word table widened to the 80 entries of
tests/golden/g4_vocab.txt so that the drop-in classes can be fed the same questions as strings, filled with the deterministic weights of
rgqa_amd/synth.py at unit gain (synth.maha_fill: under the filler's 0.02 range the pooled vector hardly varies between samples and its covariance
has a condition number near 5e7), run the Mahalanobis method's statements on the synthetic data of synth.maha_case:

    tasks/gqa_maha.py:130-189   the estimator on 512 training samples with soft targets (23 classes, two of them empty, a fifth of the samples in
                                two classes, one in twenty in none): sklearn.covariance.EmpiricalCovariance(assume_centered=False)
    tasks/gqa_maha.py:223-270   the scorer on a test batch of 8 with noise = 1e-4

Per backbone <bb> in (lxmert, uniter) the file holds

    <bb>.mean [23, 64] f32, <bb>.precision [64, 64] f64            sample_class_mean, group_lasso.precision_
    <bb>.train_pooled [512, 64] f32, <bb>.train_target [512, 23]   the estimator's inputs (what the model returned; the targets)
    <bb>.pooled [8, 64], <bb>.gaussian_score [8, 23], <bb>.sample_pred [8], <bb>.loss      first pass
    <bb>.dfeats [8, 6, 32], <bb>.dboxes [8, 6, 4 | 7]                                      feats.grad, boxes.grad
    <bb>.pooled2 [8, 64], <bb>.noised_gaussian_score [8, 23], <bb>.score2 [8], <bb>.label2 [8]   second pass on the perturbed inputs
    <bb>.score_f64, <bb>.score2_f64 [8, 23]                        -0.5 (x - mean)^T precision (x - mean) in f64 on the stored pooled / pooled2
    <bb>.ref_f32_err                                               max |reference f32 score - f64 evaluation| over both passes

and the generator asserts, and prints, the conditions the tests rely on: memberships - classes present >= 4 H; covariance condition number <= 1e4;
an empty class and >= 10 % multi-class samples; in both passes every row's top-2 gap > 1e-3 |top score|; the sign mask of tests/test_gpu_odin.py
(|ref| > 0.01 max|ref|) keeps >= 90 % of the dfeats and of the dboxes elements.  Its output on the committed file:

    g13 lxmert: memberships 594 classes present 21 (need >= 277) cond 5.056e+03 multi-class 20.5 % ref_f32_err 9.274e-04 loss 33.5982
    g13 lxmert: min top-2 gap / |top| pass 1 2.19e-03 pass 2 2.28e-03; sign mask keeps dfeats 94.1 % dboxes 93.8 %
    g13 uniter: memberships 609 classes present 21 (need >= 277) cond 9.730e+03 multi-class 23.2 % ref_f32_err 2.678e-03 loss 33.3300
    g13 uniter: min top-2 gap / |top| pass 1 2.09e-03 pass 2 2.14e-03; sign mask keeps dfeats 94.6 % dboxes 94.6 %

    python tools/gen_g13_maha.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG                                   # noqa: E402
from oracle import lxmert_ref as R                                    # noqa: E402
from rgqa_amd import synth                                            # noqa: E402
from tests.maha_reference import sample_estimator, ood_batch         # noqa: E402  (the reference's statements, one copy)


def lxmert_model(M):
    m = GG.build_reference(M, synth.MAHA_CFG["lxmert"])               # forward(feat, pos, ids, seg, mask) -> (logit, pooled)
    filled = synth.maha_fill({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return m


def uniter_model():
    import uniter.modeling as UM
    cfgd = synth.MAHA_CFG["uniter"]
    UM.VISUAL_CONFIG.set_visual_dims(cfgd["feat_dim"], 4)
    bc = UM.BertConfig(cfgd["vocab_size"], hidden_size=cfgd["hidden"], num_hidden_layers=cfgd["l_layers"], num_attention_heads=cfgd["heads"],
                       intermediate_size=cfgd["inter"], max_position_embeddings=cfgd["max_pos"], type_vocab_size=cfgd["type_vocab"])
    H = cfgd["hidden"]

    class Wrap(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder = torch.nn.Module()
            self.encoder.model = UM.UniterFeatureExtraction(bc)
            self.logit_fc = torch.nn.Sequential(torch.nn.Linear(H, 2 * H), UM.GeLU(), UM.BertLayerNorm(2 * H, eps=1e-12), torch.nn.Linear(2 * H, cfgd["num_answers"]))

        def forward(self, feat, pos7, ids, seg, mask):
            B, O = feat.shape[0], feat.shape[1]
            x = self.encoder.model(input_ids=ids, token_type_ids=seg, attention_mask=mask, visual_feats=feat,
                                   visual_token_type_ids=torch.ones(B, O, dtype=torch.long), visual_attention_mask=torch.ones(B, O, dtype=torch.long),
                                   img_pos_feat=pos7)
            return self.logit_fc(x), x
    m = Wrap()
    filled = synth.maha_fill({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return m


def score_f64(x, mean, precision):
    d = x.astype(np.float64)[:, None, :] - mean.astype(np.float64)[None, :, :]
    return -0.5 * np.einsum("bch,hk,bck->bc", d, precision.astype(np.float64), d)


def top2_gap(s):
    t = np.sort(s, 1)
    return float(((t[:, -1] - t[:, -2]) / np.abs(t[:, -1])).min())


def gen(z, bb, model, vocab):
    cfgd = synth.MAHA_CFG[bb]
    H, NC, T = cfgd["hidden"], synth.MAHA_NC, synth.MAHA_T

    class OnSentences(torch.nn.Module):
        """the reference's `model(feats, boxes, sent)` signature over the wrapped modules"""
        def __init__(self):
            super().__init__()
            self.m = model

        def forward(self, feats, boxes, sent):
            ids, mask, seg = R.sents_to_features(sent, T, vocab)
            return self.m(feats, boxes, torch.tensor(ids), torch.tensor(seg), torch.tensor(mask))
    m = OnSentences()
    tr = synth.maha_case(bb, "train")
    nb = synth.MAHA_BATCH
    loader = [(torch.from_numpy(tr["feats"][i:i + nb]), torch.from_numpy(tr["boxes"][i:i + nb]), tr["sents"][i:i + nb], torch.from_numpy(tr["target"][i:i + nb]))
              for i in range(0, synth.MAHA_TRAIN, nb)]
    mean, precision, per_class, rows, cov = sample_estimator(m, loader, NC)
    te = synth.maha_case(bb, "test")
    m.eval()
    out = ood_batch(m, torch.from_numpy(te["feats"]), torch.from_numpy(te["boxes"]), te["sents"], mean.float(), torch.from_numpy(precision).float(), NC, synth.MAHA_NOISE)
    mean = mean.numpy()
    s1, s2 = score_f64(out["pooled"].numpy(), mean, precision), score_f64(out["pooled2"].numpy(), mean, precision)
    err = max(float(np.abs(out["gaussian_score"].numpy() - s1).max()), float(np.abs(out["noised_gaussian_score"].numpy() - s2).max()))
    z[bb + ".mean"], z[bb + ".precision"] = mean, precision
    z[bb + ".train_pooled"], z[bb + ".train_target"] = rows, tr["target"]
    for k, v in out.items():
        z[bb + "." + k] = v.numpy()
    z[bb + ".score_f64"], z[bb + ".score2_f64"], z[bb + ".ref_f32_err"] = s1, s2, np.float64(err)
    # the conditions the tests rely on
    members, present = int(per_class.sum()), int((per_class > 0).sum())
    lam = np.linalg.eigvalsh(cov)
    cond = float(lam.max() / lam.min())
    multi = float(((tr["target"] != 0).sum(1) > 1).mean())
    g1, g2 = top2_gap(out["gaussian_score"].numpy()), top2_gap(out["noised_gaussian_score"].numpy())
    keep = [float((np.abs(g) > 0.01 * np.abs(g).max()).mean()) for g in (out["dfeats"].numpy(), out["dboxes"].numpy())]
    print("g13 %s: memberships %d classes present %d (need >= %d) cond %.3e multi-class %.1f %% ref_f32_err %.3e loss %.4f" % (
        bb, members, present, 4 * H + present, cond, 100 * multi, err, float(out["loss"])))
    print("g13 %s: min top-2 gap / |top| pass 1 %.2e pass 2 %.2e; sign mask keeps dfeats %.1f %% dboxes %.1f %%" % (bb, g1, g2, 100 * keep[0], 100 * keep[1]))
    assert members - present >= 4 * H
    assert cond <= 1e4
    assert present < NC and multi >= 0.10
    assert g1 > 1e-3 and g2 > 1e-3
    assert min(keep) >= 0.90
    assert all(per_class[c] == 0 for c in synth.MAHA_EMPTY)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    M = GG.import_reference()[0]
    vocab = {w.rstrip("\n"): i for i, w in enumerate(open(os.path.join(GG.OUT, "g4_vocab.txt"), encoding="utf-8"))}
    z = {}
    gen(z, "lxmert", lxmert_model(M), vocab)
    gen(z, "uniter", uniter_model(), vocab)
    out = os.path.join(GG.OUT, "g13_maha.npz")
    np.savez_compressed(out, **z)
    print("g13_maha.npz written: %d bytes" % os.path.getsize(out))


if __name__ == "__main__":
    main()
