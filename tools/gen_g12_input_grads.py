"""Generator of tests/golden/g12_input_grads.npz - runs ONLY where the reference checkout exists (like oracle/gen_golden.py, whose import
path and stand-in modules it reuses); only the .npz is committed.

The reference's own GQABUTD (butd/butd.py) and UNITER modules (uniter/modeling.py + the answer head of uniter/uniter.py:22-31), filled with
the deterministic weights of the G7 / G11 fixtures, run the ODIN scorer's statements (tasks/gqa_odin.py:97-112) at temperature 1e5 on the
G7 and G11-small / G11-full inputs with `feats` / `boxes` requiring a gradient.  Per case the file holds

    <case>.logits            the logits
    <case>.col, <case>.y     the column `torch.max(preds, 1)[1]` and the target `preds >= 0.5` at it, as the reference's statements choose them
    <case>.loss              the scalar loss
    <case>.dboxes            dL/dboxes (BUTD: [B, 36, 4]; UNITER: dL/dpos [B, O, 7]) in full
    <case>.dfeats            dL/dfeats in full (the small cases), or
    <case>.dfeats_samp/_norm its entries at synth.sample_idx("g12.<case>.dfeats", numel, 4096) and its 2-norm (f64)

    python tools/gen_g12_input_grads.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG                                   # noqa: E402
from rgqa_amd import synth                                            # noqa: E402
from rgqa_amd.synth import BUTD_WORDS, BUTD_SENTS, U_SMALL, U_FULL, uniter_batch, sample_idx   # noqa: E402

TEMPERATURE = 1e5
NSAMP = 4096


def odin_backward(logit):
    """tasks/gqa_odin.py:101-112 on the host"""
    bceloss = torch.nn.BCEWithLogitsLoss(reduction="none")
    preds = torch.sigmoid(logit / TEMPERATURE)
    labels = (torch.ones(preds.shape) * (preds >= 0.5)).float()
    loss = bceloss(logit, labels)
    idx = torch.max(preds, dim=1)[1].unsqueeze(-1)
    loss = torch.mean(torch.gather(loss, 1, idx))
    loss.backward()
    return idx.squeeze(-1), torch.gather(labels, 1, idx).squeeze(-1), loss


def record(z, case, logit, feats, boxes, full):
    col, y, loss = odin_backward(logit)
    z[case + ".logits"] = logit.detach().numpy()
    z[case + ".col"], z[case + ".y"], z[case + ".loss"] = col.numpy(), y.numpy(), np.float32(loss.item())
    z[case + ".dboxes"] = boxes.grad.numpy().copy()
    df = feats.grad.numpy()
    if full:
        z[case + ".dfeats"] = df.copy()
    else:
        z[case + ".dfeats_samp"] = df.reshape(-1)[sample_idx("g12.%s.dfeats" % case, df.size, NSAMP)]
        z[case + ".dfeats_norm"] = np.float64(np.sqrt((df.astype(np.float64) ** 2).sum()))
    print("g12 %s: col %s y %s loss %.6f max|dfeats| %.3e max|dboxes| %.3e" % (case, col.tolist(), y.tolist(), loss.item(), np.abs(df).max(),
                                                                             np.abs(z[case + ".dboxes"]).max()))


def gen_butd(z):
    from butd.butd import GQABUTD
    from butd.preprocess import Dictionary
    from tests.test_oracle_golden import butd_fill
    from oracle import butd_ref as BR
    d = Dictionary()
    for w in BUTD_WORDS:
        d.add_word(w)
    m = GQABUTD(23, d, dropout=False)
    filled = butd_fill(BR.ButdConfig(ntoken=len(BUTD_WORDS), num_answers=23))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in filled.items()})
    m.train()                                    # tasks/gqa_odin.py:87-88 (dropout=False: nothing is dropped)
    b = synth.synth_batch(len(BUTD_SENTS), 8, O=36, F=2048, NA=23, vocab=64, seed=606, uq_frac=0.2)
    feat, pos = torch.from_numpy(b["feats"]).requires_grad_(True), torch.from_numpy(b["boxes"]).requires_grad_(True)
    toks = m.tokenize(BUTD_SENTS)
    # GQABUTD.forward without the hard-coded .cuda() of butd.py:197 (as gen_golden.gen_butd)
    q_enc = m.q_enc(m.w_emb(toks))
    image_features = torch.cat([feat, pos], dim=2)
    att = m.att(image_features, q_enc)
    img_enc = (image_features * att).sum(dim=1)
    logit = m.ans_classifier(m.q_project(q_enc) * m.img_project(img_enc))
    record(z, "butd_g7", logit, feat, pos, full=False)


def gen_uniter(z):
    import uniter.modeling as UM
    for tag, cfgd, cases in (("small", U_SMALL, [(5, 3, 6, 91), (8, 3, 6, 92)]), ("full", U_FULL, [(20, 4, 36, 93)])):
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
                return self.logit_fc(x)
        m = Wrap()
        filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
        m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
        m.eval()                                 # tasks/gqa_odin.py:85-86
        for (T, B, O, seed) in cases:
            b = uniter_batch(cfgd, T, B, O, seed)
            t = {k: torch.from_numpy(v) for k, v in b.items() if k != "lengths"}
            feats, pos7 = t["feats"].clone().requires_grad_(True), t["pos7"].clone().requires_grad_(True)
            logit = m(feats, pos7, t["input_ids"], t["segment_ids"], t["input_mask"])
            record(z, "uniter_%s_T%d" % (tag, T), logit, feats, pos7, full=(tag == "small"))


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    GG.import_reference()
    z = {}
    gen_butd(z)
    gen_uniter(z)
    out = os.path.join(GG.OUT, "g12_input_grads.npz")
    np.savez_compressed(out, **z)
    print("g12_input_grads.npz written: %d bytes" % os.path.getsize(out))


if __name__ == "__main__":
    main()
