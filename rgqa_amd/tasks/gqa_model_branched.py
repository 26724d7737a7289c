"""Mirror of the reference's tasks/gqa_model_branched.py (14-51): `GQAModel_branched(num_answers)`, `MAX_GQA_LENGTH` - GQAModel plus a second head on the
pooled vector, the learned confidence `conf_fc`.

`logit_fc` and `conf_fc` are real nn.Sequential(Linear, GeLU, LayerNorm, Linear) modules with the reference's state_dict keys; their parameters are views
of the engine's arena and their arithmetic is fused into the engine (rgqa_config.conf_branch): one forward gives both outputs, whatever combination of
their gradients arrives is one engine backward, and `conf_fc` is clipped, stepped and exchanged with the rest of the arena."""
import types

import torch.nn as nn

try:                                   # the reference's process-global flags (src/param.py:150) when run drop-in
    from param import args
except Exception:                      # stand-alone use: the launchers' defaults (run/gqa_branched_finetune.bash)
    args = types.SimpleNamespace(llayers=9, xlayers=5, rlayers=5, from_scratch=False)

from ..lxrt.entry import LXRTEncoder
from ..lxrt.modeling import BertLayerNorm, GeLU

# Max length including <bos> and <eos>
MAX_GQA_LENGTH = 20


class GQAModel_branched(nn.Module):
    def __init__(self, num_answers, max_seq_length=MAX_GQA_LENGTH, model_args=None):
        super().__init__()
        self.lxrt_encoder = LXRTEncoder(model_args if model_args is not None else args, max_seq_length=max_seq_length)
        hid_dim = self.lxrt_encoder.dim
        self.logit_fc = nn.Sequential(
            nn.Linear(hid_dim, hid_dim * 2),
            GeLU(),
            BertLayerNorm(hid_dim * 2, eps=1e-12),
            nn.Linear(hid_dim * 2, num_answers)
        )
        self.conf_fc = nn.Sequential(
            nn.Linear(hid_dim, hid_dim * 2),
            GeLU(),
            BertLayerNorm(hid_dim * 2, eps=1e-12),
            nn.Linear(hid_dim * 2, 1)
        )
        self.logit_fc.apply(self.lxrt_encoder.model.init_bert_weights)
        self.conf_fc.apply(self.lxrt_encoder.model.init_bert_weights)
        self.lxrt_encoder.model.attach_head(self.logit_fc, self.conf_fc)

    def forward(self, feat, pos, sent):
        """feat (b, o, f), pos (b, o, 4), sent list[str] of length b -> (logit (b, num_answers), conf (b, 1))."""
        return self.lxrt_encoder.forward_branched(sent, (feat, pos))
