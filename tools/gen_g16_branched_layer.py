"""Generator of tests/golden/g16_branched_layer.npz - runs ONLY where the reference checkout exists (like oracle/gen_golden.py, whose import path and stand-in
modules it reuses); only the .npz is committed.

The reference's own layer-wise GQAModel_branched (tasks/gqa_branched_layer.py:280-320) at synth.LAYER_SMALL (the G1 small config with three cross-modality
layers) and project_size = synth.LAYER_PROJECT_SIZE = 16.  Its LXRTEntry is replaced by a stand-in that builds the file's own LXRTFeatureExtraction(mode='lxr')
without the network download and takes token ids where the reference takes strings; weights are synth.layer_branched_fill (the deterministic filler: it meets
both conditions below as it is, so nothing is scaled), eval mode, synth.small_batch(8) under synth.branched_target() (B = 3, row 1 unanswerable), through the
trainer's statements (:396-413 = tasks/gqa_branched.py:126-143; tests/branched_reference.py: one copy) in the BCE and the --mceLoss form.  The file holds

    logits [3, 11], conf [3, 1], projcat [3, 48], pooled [3, 64], target_with_uq [3, 12]
    bce.loss / .loss_ce / .loss_conf,  mce.loss / .loss_ce / .loss_conf
    keys                               the model's state_dict keys in order
    dead                               parameters without a gradient (the last cross layer's vision side)
    bce.grad.<key>                     every live parameter's gradient, sampled as g15 samples them (tests.layer_branched_reference.fixture_index): whole for
                                       logit_fc.*, projs.*, conf_fc.* and every tensor of up to 1024 elements, 512 elements of the larger ones
    mce.grad.<key>                     the same for --mceLoss at the elements synth.sample_idx(key, numel) names
    noconf.grad.<key>                  the BCE form's gradients of loss_ce ALONE at the elements of bce.grad.<key> (parameters of the branch have none)

and the generator asserts what keeps the tests from being blind: (a) max |projcat| < 0.95 - no tanh is saturated; (b) full and noconf gradients differ by at
least 50 times the f32 gate of the GPU tests on at least one stored tensor of each of encoder.layer.*, r_layers.*, x_layers.0.* and x_layers.1.*, so a missing
gradient injection at any tap fails the fixture test.

    python tools/gen_g16_branched_layer.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG                                   # noqa: E402
from rgqa_amd import synth                                            # noqa: E402
from tests import layer_branched_reference as LR                      # noqa: E402


def build(M, cfgd, project_size):
    M.VISUAL_CONFIG.l_layers, M.VISUAL_CONFIG.x_layers, M.VISUAL_CONFIG.r_layers = cfgd["l_layers"], cfgd["x_layers"], cfgd["r_layers"]
    M.VISUAL_CONFIG.set_visual_dims(cfgd["feat_dim"], cfgd["pos_dim"])
    bc = M.BertConfig(cfgd["vocab_size"], hidden_size=cfgd["hidden"], num_attention_heads=cfgd["heads"], intermediate_size=cfgd["inter"],
                      max_position_embeddings=cfgd["max_pos"], type_vocab_size=cfgd["type_vocab"])
    sys.argv = sys.argv[:1]
    # the file's trainer half imports the dataset classes (image transforms, answer tables) that the model classes never touch: empty stand-ins, as
    # oracle/gen_golden.py does for the download helpers
    import types
    for name, attrs in (("tasks.gqa_data", ("GQADataset", "GQATorchDataset", "GQAEvaluator")), ("pretrain.qa_answer_table", ("load_lxmert_qa",)), ("tqdm", ("tqdm",))):
        if name not in sys.modules:
            try:
                __import__(name)
            except Exception:
                mod = types.ModuleType(name)
                for a in attrs:
                    setattr(mod, a, None)
                sys.modules[name] = mod
    import tasks.gqa_branched_layer as GL                            # the reference's own classes

    class Entry(torch.nn.Module):
        """stands where the file's LXRTEntry stands: no download, `sent` = (ids, seg, mask)"""
        def __init__(self, args, max_seq_length):
            super().__init__()
            self.model = GL.LXRTFeatureExtraction(bc, mode="lxr")

        @property
        def dim(self):
            return cfgd["hidden"]

        def forward(self, sents, feats, visual_attention_mask=None):
            ids, seg, mask = sents
            return self.model(ids, seg, mask, visual_feats=feats, visual_attention_mask=visual_attention_mask)
    GL.LXRTEntry = Entry
    GL.args.project_size = project_size
    m = GL.GQAModel_branched(cfgd["num_answers"])
    filled = synth.layer_branched_fill({k: tuple(v.shape) for k, v in m.state_dict().items()})
    m.load_state_dict({k: torch.from_numpy(v) for k, v in filled.items()})
    return m


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    M, _, _, _ = GG.import_reference()
    cfgd, P = synth.LAYER_SMALL, synth.LAYER_PROJECT_SIZE
    m = build(M, cfgd, P)
    m.eval()
    b = {k: torch.from_numpy(v) for k, v in synth.small_batch(8).items() if k != "lengths"}
    t = torch.from_numpy(synth.branched_target())
    z = dict(target_with_uq=t.numpy(), keys=np.array(list(m.state_dict().keys())))
    sent = (b["input_ids"], b["segment_ids"], b["input_mask"])
    dead = None
    for form, mce, what in (("bce", False, "loss"), ("mce", True, "loss"), ("noconf", False, "loss_ce")):
        for p in m.parameters():
            p.grad = None
        logit, conf = m(b["feats"], b["boxes"], sent)
        loss, ce, cf, _, _ = LR.trainer_statements(logit, conf, t, mce)
        (loss if what == "loss" else ce).backward()
        if form != "noconf":
            z["logits"], z["conf"] = logit.detach().numpy(), conf.detach().numpy()
            z[form + ".loss"], z[form + ".loss_ce"], z[form + ".loss_conf"] = np.float32(loss.item()), np.float32(ce.item()), np.float32(cf.item())
            dead = sorted(k for k, p in m.named_parameters() if p.grad is None)
        for k, p in m.named_parameters():
            if p.grad is None:
                continue
            g = p.grad.detach().numpy()
            idx = LR.fixture_index("bce" if form == "noconf" else form, k, g.size)
            z[form + ".grad." + k] = g if idx is None else g.reshape(-1)[idx]
        print("g16 %s: loss %.6f = %.6f + %.6f; conf logits %s" % (form, loss.item(), ce.item(), cf.item(), conf.detach().reshape(-1).numpy()))
    with torch.no_grad():
        all_feats, pooled = m.lxrt_encoder(sent, (b["feats"], b["boxes"]))
        z["pooled"] = pooled.numpy()
        z["projcat"] = torch.cat([proj(f) for proj, f in zip(m.projs, all_feats)], 1).numpy()
    z["dead"] = np.array(dead)
    assert all(k.startswith("lxrt_encoder.model.bert.encoder.x_layers.%d.visn_" % (cfgd["x_layers"] - 1)) for k in dead), dead
    assert not any(k.startswith("noconf.grad.") and LR.is_branch(k[len("noconf.grad."):]) for k in z)
    amax = float(np.abs(z["projcat"]).max())
    reach, ok = LR.branch_reach(z)
    print("g16: max |projcat| = %.4f; |full - noconf| / gate per group: %s" % (amax, {k: round(v, 1) for k, v in reach.items()}))
    assert amax < 0.95, "condition (a): a tanh is saturated - scale the projs fill down in synth.layer_branched_fill"
    assert ok, "condition (b): a group of layers does not feel the branch at 50 x the f32 gate - scale the projs / conf_fc fill up in synth.layer_branched_fill"
    out = os.path.join(GG.OUT, "g16_branched_layer.npz")
    np.savez_compressed(out, **z)
    print("g16_branched_layer.npz written: %d bytes" % os.path.getsize(out))
    assert os.path.getsize(out) < (1 << 20)


if __name__ == "__main__":
    main()
