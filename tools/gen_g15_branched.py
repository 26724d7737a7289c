"""Generator of tests/golden/g15_branched.npz - runs ONLY where the reference checkout exists (like oracle/gen_golden.py, whose import path and stand-in
modules it reuses); only the .npz is committed.

The reference's own GQAModel_branched (tasks/gqa_model_branched.py:14-51) at the G1 small config, its LXRTEncoder replaced by a stand-in that builds the
reference's LXRTFeatureExtraction without the network download and takes token ids where the reference takes strings (the fixture's batch is ids), filled
with the deterministic weights of rgqa_amd/synth.py, in eval mode on synth.small_batch(8) under synth.branched_target() (B = 3, row 1 unanswerable), through
the trainer's statements tasks/gqa_branched.py:126-143 (tests/branched_reference.py: one copy) in the BCE and the --mce_loss form.  The file holds

    logits [3, 11], conf [3, 1], pooled [3, 64], target_with_uq [3, 12]
    bce.loss / .loss_ce / .loss_conf,  mce.loss / .loss_ce / .loss_conf
    bce.grad.<state_dict key>          every live parameter's gradient (dead parameters - the last cross layer's vision side - are listed in `dead`): whole for
                                       logit_fc.*, conf_fc.* and every tensor of up to 4096 elements, the 1024 elements tests.branched_reference.fixture_index names
                                       of the larger ones (the feed-forward weights) - the file stays under 1 MiB
    mce.grad.<state_dict key>          the same for --mce_loss at the elements synth.sample_idx(key, numel) names (the whole tensor up to 64 elements)

    python tools/gen_g15_branched.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG                                   # noqa: E402
from rgqa_amd import synth                                            # noqa: E402
from tests.branched_reference import trainer_statements, fixture_index               # noqa: E402


def build(M, ENT, cfgd):
    M.VISUAL_CONFIG.l_layers, M.VISUAL_CONFIG.x_layers, M.VISUAL_CONFIG.r_layers = cfgd["l_layers"], cfgd["x_layers"], cfgd["r_layers"]
    M.VISUAL_CONFIG.set_visual_dims(cfgd["feat_dim"], cfgd["pos_dim"])
    bc = M.BertConfig(cfgd["vocab_size"], hidden_size=cfgd["hidden"], num_attention_heads=cfgd["heads"], intermediate_size=cfgd["inter"],
                      max_position_embeddings=cfgd["max_pos"], type_vocab_size=cfgd["type_vocab"])

    class Encoder(torch.nn.Module):
        """stands where lxrt.entry.LXRTEncoder stands: no download, `sent` = (ids, seg, mask)"""
        def __init__(self, args, max_seq_length, mode="x"):
            super().__init__()
            self.model = M.LXRTFeatureExtraction(bc, mode=mode)

        @property
        def dim(self):
            return cfgd["hidden"]

        def forward(self, sents, feats, visual_attention_mask=None):
            ids, seg, mask = sents
            return self.model(ids, seg, mask, visual_feats=feats, visual_attention_mask=visual_attention_mask)
    ENT.LXRTEncoder = Encoder
    sys.argv = sys.argv[:1]
    import tasks.gqa_model_branched as GB                            # the reference's own class; it binds LXRTEncoder at import
    m = GB.GQAModel_branched(cfgd["num_answers"])
    filled = synth.fill_state_dict({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return m


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    M, _, _, ENT = GG.import_reference()
    m = build(M, ENT, synth.SMALL)
    m.eval()
    b = {k: torch.from_numpy(v) for k, v in synth.small_batch(8).items() if k != "lengths"}
    t = torch.from_numpy(synth.branched_target())
    z = dict(target_with_uq=t.numpy())
    dead = None
    for form, mce in (("bce", False), ("mce", True)):
        for p in m.parameters():
            p.grad = None
        logit, conf = m(b["feats"], b["boxes"], (b["input_ids"], b["segment_ids"], b["input_mask"]))
        loss, ce, cf, _, _ = trainer_statements(logit, conf, t, mce)
        loss.backward()
        z["logits"], z["conf"] = logit.detach().numpy(), conf.detach().numpy()
        z[form + ".loss"], z[form + ".loss_ce"], z[form + ".loss_conf"] = np.float32(loss.item()), np.float32(ce.item()), np.float32(cf.item())
        dead = sorted(k for k, p in m.named_parameters() if p.grad is None)
        for k, p in m.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.detach().numpy()
            idx = fixture_index(form, k, g.size)
            z[form + ".grad." + k] = g if idx is None else g.reshape(-1)[idx]
        print("g15 %s: loss %.6f = %.6f + %.6f; conf logits %s" % (form, loss.item(), ce.item(), cf.item(), conf.detach().reshape(-1).numpy()))
    with torch.no_grad():
        z["pooled"] = m.lxrt_encoder((b["input_ids"], b["segment_ids"], b["input_mask"]), (b["feats"], b["boxes"])).numpy()
    z["dead"] = np.array(dead)
    assert all(k.startswith("lxrt_encoder.model.bert.encoder.x_layers.1.visn_") for k in dead), dead
    out = os.path.join(GG.OUT, "g15_branched.npz")
    np.savez_compressed(out, **z)
    print("g15_branched.npz written: %d bytes" % os.path.getsize(out))
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
