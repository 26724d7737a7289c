"""Test-time scoring of answer logits on the device — the expressions the reference's RVQA test scripts
apply to `logit = model(feats, boxes, sent)`:

    score, label = torch.sigmoid(logit).max(1)                tasks/gqa_conf.py:344, gqa_energy.py:184, gqa_dropout.py:109
    outputs = torch.sigmoid(logit / args.temperature)         tasks/gqa_odin.py:130-131
    score = torch.log(1 + torch.exp(logit)).sum(1)            tasks/gqa_energy.py:185 (energy score; :135 in training)
    logit_k = logit.topk(k=2).values; log(1+exp(logit_k)).sum tasks/gqa_energy.py:205-206

in one fused HIP kernel (`rgqa_score_rows`, csrc/score.hip), and the ODIN method on top of it (tasks/gqa_odin.py:97-131) for all three
backbones:

    labels = preds >= 0.5; idx = preds.max(1)[1]; loss = mean(gather(bceloss(logit, labels), 1, idx))     :101-110   odin_dlogits
    featsPt = torch.add(feats.data, (torch.ge(feats.grad, 0).float() - 0.5) * 2, alpha=-noise)             :115-121   sign_step
    the whole batch step: forward, loss gradient, input gradients, perturbed inputs, second forward, score  :97-131    odin_scores

There is no CPU fallback: without the HIP library this raises."""
import collections
import ctypes as C

import torch

from . import _lib

Scores = collections.namedtuple("Scores", "max_score label energy topk_values topk_indices topk_energy")
OdinScores = collections.namedtuple("OdinScores", "score label logits feats_pt boxes_pt")


def score_rows(logits, temperature=1.0, k=0):
    """logits: f32 CUDA tensor [B, NA] (row-major, any row stride). Returns `Scores`; the top-k fields are None for k == 0."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("score_rows: logits must be a 2-D float32 CUDA tensor")
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    lib = _lib.load()
    B, NA = logits.shape
    dev = logits.device
    ms = torch.empty(B, dtype=torch.float32, device=dev)
    lab = torch.empty(B, dtype=torch.int64, device=dev)
    en = torch.empty(B, dtype=torch.float32, device=dev)
    tv = ti = te = None
    if k > 0:
        tv = torch.empty(B, k, dtype=torch.float32, device=dev)
        ti = torch.empty(B, k, dtype=torch.int64, device=dev)
        te = torch.empty(B, dtype=torch.float32, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    _lib.check(lib.rgqa_score_rows(p(logits), logits.stride(0), B, NA, float(temperature), int(k), p(ms), p(lab), p(en), p(tv), p(ti), p(te),
                                   C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)))
    return Scores(ms, lab, en, tv, ti, te)


def sigmoid_max(logits, temperature=1.0):
    """(score, label) = torch.sigmoid(logit / temperature).max(1)"""
    s = score_rows(logits, temperature)
    return s.max_score, s.label


def energy_score(logits, k=0):
    """torch.log(1 + torch.exp(logit)).sum(1), or over the top-k logits when k > 0 (gqa_energy.py:185 / :205-206)"""
    s = score_rows(logits, 1.0, k)
    return s.topk_energy if k > 0 else s.energy


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def odin_dlogits(logits, label, max_score):
    """The gradient of ODIN's loss w.r.t. the logits (gqa_odin.py:101-110) and the loss itself.

    logits: f32 CUDA [B, NA]; label (int64 [B]) and max_score (f32 [B]) are what `score_rows(logits, temperature)` returned for these
    logits: the chosen column and the sigmoid value the target `preds >= 0.5` is taken from.  Returns (dlogits [B, NA], loss [1]):
    dlogits[b, label[b]] = (sigmoid(logit) - target) / B on the un-tempered logit, exact zeros elsewhere."""
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("odin_dlogits: logits must be a 2-D float32 CUDA tensor")
    B, NA = logits.shape
    if logits.stride(1) != 1:
        logits = logits.contiguous()
    if label.dtype != torch.int64 or max_score.dtype != torch.float32 or label.shape != (B,) or max_score.shape != (B,) \
            or label.device != logits.device or max_score.device != logits.device:
        raise ValueError("odin_dlogits: label (int64) and max_score (float32) must be [B] tensors on the logits' device")
    label, max_score = label.contiguous(), max_score.contiguous()
    dl = torch.empty(B, NA, dtype=torch.float32, device=logits.device)
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    p = _lib.ptr
    _lib.check(_lib.load().rgqa_odin_dlogits(p(logits), logits.stride(0), p(label), p(max_score), B, NA, NA, p(dl), dl.stride(0), p(loss), _stream(logits.device)))
    return dl, loss


def sign_step(x, grad, noise, out=None):
    """x - noise * sign(grad) with sign(g) = (torch.ge(g, 0).float() - 0.5) * 2 (gqa_odin.py:115-121): zero and -0.0 step by -noise, NaN by
    +noise.  x, grad: contiguous f32 CUDA tensors of one shape; out (optional) may be x itself."""
    if out is None:
        out = torch.empty_like(x)
    for t in (x, grad, out):
        if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.shape == x.shape and t.device == x.device):
            raise ValueError("sign_step: x, grad and out must be contiguous float32 CUDA tensors of one shape on one device")
    p = _lib.ptr
    _lib.check(_lib.load().rgqa_sign_step(p(x), p(grad), float(noise), p(out), x.numel(), _stream(x.device)))
    return out


def odin_scores(model, feats, boxes, sent, temperature=1.0, noise=0.0):
    """One batch of the reference's ODIN scorer (gqa_odin.py:97-131) for `GQAModel`, `GQABUTD` or `GQAUNITER` (drop-in classes):
    forward, `score_rows`, `odin_dlogits`, backward through the model's autograd boundary with input gradients, two `sign_step`s, a second
    forward under no_grad on the perturbed inputs, `score_rows` at the temperature.  Returns `OdinScores(score, label, logits, feats_pt,
    boxes_pt)`: score / label = sigmoid(logit / temperature).max(1) of the SECOND pass, its logits, and the perturbed inputs.

    `model.training` is honoured as the caller set it (the reference scores LXMERT / UNITER in eval() and BUTD in train() with dropout=False).
    The pass never runs the data-parallel gradient exchange, whatever `model.training` says.  Afterwards the parameters' `.grad` hold the
    scoring pass's gradients, as after the reference's `loss.backward()`: call `zero_grad()` before training on."""
    from .lxrt.modeling import scoring_pass
    f = feats.detach().contiguous().float().requires_grad_(True)
    b = boxes.detach().contiguous().float().requires_grad_(True)
    with scoring_pass():
        with torch.enable_grad():
            logit = model(f, b, sent)
        lg = logit.detach()
        s = score_rows(lg, temperature)
        dl, _ = odin_dlogits(lg, s.label, s.max_score)
        logit.backward(dl)
    feats_pt = sign_step(f.detach(), f.grad, noise)
    boxes_pt = sign_step(b.detach(), b.grad, noise)
    with torch.no_grad():
        logit2 = model(feats_pt, boxes_pt, sent)
    s2 = score_rows(logit2, temperature)
    return OdinScores(s2.max_score, s2.label, logit2, feats_pt, boxes_pt)
