"""Mirror of the model classes of the reference's tasks/gqa_branched_layer.py (:47-59, :280-320): `GQAModel_branched(num_answers)`, `GQAProjector`,
`MAX_GQA_LENGTH` - the layer-wise sibling of tasks.gqa_model_branched: the learned confidence reads EVERY cross-modality layer instead of the pooled vector.
The [CLS] row of layer i's language output goes through `projs[i]` = Linear(H, project_size) -> Tanh, the x_layers projections side by side through
`conf_fc` = Linear(X P, 2 X P) -> GeLU -> LayerNorm -> Linear(2 X P, 1).

`projs`, `conf_fc` and `logit_fc` are real nn modules with the reference's state_dict keys; their parameters are views of the engine's arena and their arithmetic
is fused into the engine (rgqa_config.conf_branch = 2): one forward gives both outputs, whatever combination of their gradients arrives is ONE engine backward -
the gradient of every layer's tap joins the encoder backward in front of that layer - and with everything outside `projs` / `conf_fc` frozen
(--freeze_vqa_branch, :348-352) the step runs neither the answer head's nor the encoder's backward."""
import types

import torch.nn as nn

try:                                   # the reference's process-global flags (src/param.py:150) when run drop-in
    from param import args
except Exception:                      # stand-alone use: the launchers' defaults (run/gqa_branched_layer_finetune.bash; param.py:57)
    args = types.SimpleNamespace(llayers=9, xlayers=5, rlayers=5, from_scratch=False, project_size=128)

from ..lxrt.entry import LXRTEncoder
from ..lxrt.modeling import BertLayerNorm, GeLU, VISUAL_CONFIG

# Max length including <bos> and <eos>
MAX_GQA_LENGTH = 20


class GQAProjector(nn.Module):
    """Linear(hidden_size, project_size) -> Tanh on the first token of a layer's language output (:47-59).  Inside GQAModel_branched the engine does the
    arithmetic; called on its own it is the plain torch module."""

    def __init__(self, config, args):
        super().__init__()
        self.proj = nn.Sequential(
            nn.Linear(config.hidden_size, args.project_size),
            nn.Tanh()
        )

    def forward(self, hidden_states):
        # always extract first token
        first_token_tensor = hidden_states[:, 0]
        return self.proj(first_token_tensor)


class GQAModel_branched(nn.Module):
    def __init__(self, num_answers, max_seq_length=MAX_GQA_LENGTH, model_args=None):
        super().__init__()
        a = model_args if model_args is not None else args
        self.lxrt_encoder = LXRTEncoder(a, max_seq_length=max_seq_length)
        hid_dim = self.lxrt_encoder.dim
        pa = types.SimpleNamespace(project_size=int(getattr(a, "project_size", 128)))
        self.projs = nn.ModuleList([GQAProjector(self.lxrt_encoder.model.config, pa) for _ in range(VISUAL_CONFIG.x_layers)])
        inp_size = VISUAL_CONFIG.x_layers * pa.project_size
        self.conf_fc = nn.Sequential(
            nn.Linear(inp_size, inp_size * 2),
            GeLU(),
            BertLayerNorm(inp_size * 2, eps=1e-12),
            nn.Linear(inp_size * 2, 1)
        )
        self.logit_fc = nn.Sequential(
            nn.Linear(hid_dim, hid_dim * 2),
            GeLU(),
            BertLayerNorm(hid_dim * 2, eps=1e-12),
            nn.Linear(hid_dim * 2, num_answers)
        )
        self.logit_fc.apply(self.lxrt_encoder.model.init_bert_weights)
        self.conf_fc.apply(self.lxrt_encoder.model.init_bert_weights)
        self.projs.apply(self.lxrt_encoder.model.init_bert_weights)
        self.lxrt_encoder.model.attach_head(self.logit_fc, self.conf_fc, self.projs)

    def forward(self, feat, pos, sent):
        """feat (b, o, f), pos (b, o, 4), sent list[str] of length b -> (logit (b, num_answers), conf (b, 1))."""
        return self.lxrt_encoder.forward_branched(sent, (feat, pos))
