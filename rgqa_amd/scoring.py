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

and the Mahalanobis method (tasks/gqa_maha.py) for all three backbones, on the pooled vector `GQAModel_maha` / `GQAUNITER_maha` return and on the
`joint_repr` of `GQABUTD_maha`:

    mean[j] = mean of the pooled rows of the samples with target[i][j] != 0; precision = pinvh(covariance)  :130-183   MahaEstimator, maha_sample_estimator
    gaussian_score[b, c] = -0.5 (x_b - mean_c)^T precision (x_b - mean_c); .max(1)                          :228-239   maha_score_rows
    loss = mean(-gaussian_score[b, pred_b]); loss.backward()                                                :240-244   maha_dpooled
    the whole batch step: forward, score, input step, second forward, score                                 :223-270   maha_scores

with precision = W W^T factored once on the host (csrc/maha.hip), and the loss head of the energy method's fine-tuning (tasks/gqa_energy.py:117-145,
run/gqa_energy_finetune.bash) as one fused operator (`rgqa_op_energy_loss`, csrc/energy_loss.hip):

    id_inds = target[:, -1] == 0; target = target[:, :-1]; BCE x NA (or --mceLoss: cross entropy x NA) and E_f                 :122-135   energy_loss_rows
    loss += 0.1 * (relu(-E_f[id_inds] - m_in)**2).mean() + 0.1 * (relu(m_out + E_f[~id_inds])**2).mean()                      :137-138
    the same under autograd, for `loss.backward()` through any drop-in model; label and score = E_f from the same pass        :122-145   energy_finetune_loss

and the loss head of the soft resampling of the unanswerable questions (tasks/gqa_resampling.py:176-220, lxmert / uniter order; csrc/resample.hip) on ONE
forward of the concatenated [positive ; negative] batch (the weight parameters themselves: rgqa_amd/resample.py):

    loss_pos = mean(bce(logit_pos, target_pos)) * NA;  loss_neg = (weights @ bce(logit_neg, target_neg)).sum() / Bn           :196-200   resample_loss_rows
    loss = loss_pos + loss_neg;  loss_w = -loss_neg, under autograd for the model, closed form for the weight parameters      :202-203   resample_finetune_loss

and the loss head and the scorer of the confidence-branch model (tasks/gqa_branched.py, GQAModel_branched; csrc/branched_loss.hip):

    id_inds = target[:, -1] == 0; loss_ce over logit[id_inds] (BCE x NA, or --mce_loss) + binary_cross_entropy(sigmoid(conf), id_inds)     :126-142   branched_loss_rows
    the same under autograd over (logit, conf), for `loss.backward()` through GQAModel_branched: ONE engine backward                      :126-143   branched_finetune_loss
    score1, label = sigmoid(logit).max(1); score2 = sigmoid(conf); score = score2, or score1 * score2 with --mix_branched_score            :206-214   branched_scores

There is no CPU fallback: without the HIP library this raises."""
import collections
import ctypes as C

import numpy as np
import torch

from . import _lib

Scores = collections.namedtuple("Scores", "max_score label energy topk_values topk_indices topk_energy")
OdinScores = collections.namedtuple("OdinScores", "score label logits feats_pt boxes_pt")
MahaPack = collections.namedtuple("MahaPack", "mean precision W nu")
MahaRows = collections.namedtuple("MahaRows", "score label y all_scores pooled")
MahaScores = collections.namedtuple("MahaScores", "score label pooled feats_pt boxes_pt")
EnergyLoss = collections.namedtuple("EnergyLoss", "loss base reg dlogits energy label")
ResampleLoss = collections.namedtuple("ResampleLoss", "loss loss_pos loss_neg dlogits row_loss")
BranchedLoss = collections.namedtuple("BranchedLoss", "loss loss_ce loss_conf dlogits dconf conf label score1")


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


# ------------------------------------------------------------------------------------------------ Mahalanobis (tasks/gqa_maha.py)
def maha_factor(precision):
    """precision [H, H] (symmetrised) -> (W [H, R], P) in numpy f64 with W W^T = P = V diag(lam) V^T over the eigenvalues
    lam > max(lam) * H * eps(f64): the cut of scipy.linalg.pinvh, which sklearn's EmpiricalCovariance takes its precision_ from.  For a precision
    matrix that came out of pinvh the cut only drops the null space pinvh left."""
    P = np.asarray(precision, dtype=np.float64)
    if P.ndim != 2 or P.shape[0] != P.shape[1]:
        raise ValueError("maha: precision must be a square matrix")
    lam, V = np.linalg.eigh((P + P.T) * 0.5)
    keep = lam > lam.max() * P.shape[0] * np.finfo(np.float64).eps
    lam, V = lam[keep], V[:, keep]
    return V * np.sqrt(lam), (V * lam) @ V.T


def maha_finalize(n, sums, G):
    """The host half of the estimator (gqa_maha.py:170-183) in numpy f64, from what `rgqa_maha_accumulate` gathered: n [NC] samples per class,
    sums [NC, H] their pooled rows added up, G [H, H] = sum over (sample, class) memberships of x x^T.  mean_c = sums_c / n_c (zero for a class
    without a sample); the rows `X` of the reference are x - mean_c per membership, so X^T X = G - sum_c n_c mean_c mean_c^T and the (biased)
    covariance is that over sum(n) (sklearn's own re-centring subtracts the mean of X, which is zero in exact arithmetic); precision = pinvh(cov).
    Returns (mean [NC, H], precision [H, H], W [H, R]) with precision = W W^T."""
    n, sums, G = np.asarray(n, np.float64), np.asarray(sums, np.float64), np.asarray(G, np.float64)
    total = n.sum()
    if total <= 0:
        raise ValueError("maha: no sample has joined a class")
    mean = sums / np.maximum(n, 1.0)[:, None]
    cov = (G - (mean * n[:, None]).T @ mean) / total
    lam, V = np.linalg.eigh((cov + cov.T) * 0.5)
    keep = lam > lam.max() * cov.shape[0] * np.finfo(np.float64).eps
    lam, V = lam[keep], V[:, keep]
    return mean, (V / lam) @ V.T, V / np.sqrt(lam)


def _pack(mean, precision, W, device):
    mean = np.asarray(mean, np.float64)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(device)
    return MahaPack(t(mean), t(precision), t(W), t(mean @ W))            # nu = mean W in f64, stored as f32


def maha_pack(mean, precision, device="cuda"):
    """The {"mean", "precision"} pair of a reference `sample_estimates.pkl` (tensors or arrays; gqa_maha.py:124-127) -> MahaPack of f32 tensors
    on `device`: mean [NC, H], precision [H, H], W [H, R] with precision = W W^T, nu = mean W [NC, R]."""
    mean = mean.detach().cpu().numpy() if isinstance(mean, torch.Tensor) else np.asarray(mean)
    precision = precision.detach().cpu().numpy() if isinstance(precision, torch.Tensor) else np.asarray(precision)
    if mean.ndim != 2 or precision.shape != (mean.shape[1], mean.shape[1]):
        raise ValueError("maha_pack: mean must be [NC, H] and precision [H, H]")
    W, P = maha_factor(precision)
    return _pack(mean, P, W, device)


def _f32_rows(name, t, cols=None):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and (cols is None or t.shape[1] == cols)):
        raise ValueError("%s must be a 2-D float32 CUDA tensor%s" % (name, "" if cols is None else " with %d columns" % cols))
    return t if t.stride(1) == 1 else t.contiguous()


def _maha_scratch(B, NC, dev):
    n = C.c_size_t()
    _lib.check(_lib.load().rgqa_maha_scratch_bytes(B, NC, C.byref(n)))
    return torch.empty(n.value, dtype=torch.uint8, device=dev), n.value


class MahaEstimator:
    """gqa_maha.py:130-183: `update(pooled, target)` per training batch (pooled [B, H] f32 CUDA, target [B, NC] f32 CUDA, the UQ column already
    dropped) accumulates on the device in f64 (`rgqa_maha_accumulate`); `finalize()` reads the state and finishes in numpy f64 -> MahaPack."""

    def __init__(self, num_classes, hidden, device="cuda"):
        self.num_classes, self.hidden, self.device = int(num_classes), int(hidden), torch.device(device)
        n = C.c_size_t()
        _lib.check(_lib.load().rgqa_maha_state_doubles(self.num_classes, self.hidden, C.byref(n)))
        self.state = torch.zeros(n.value, dtype=torch.float64, device=self.device)

    def update(self, pooled, target):
        pooled = _f32_rows("MahaEstimator.update: pooled", pooled, self.hidden)
        target = _f32_rows("MahaEstimator.update: target", target, self.num_classes)
        if target.shape[0] != pooled.shape[0] or pooled.device != self.state.device or target.device != self.state.device:
            raise ValueError("MahaEstimator.update: pooled and target must hold the same rows on the estimator's device")
        B = pooled.shape[0]
        scratch, nbytes = _maha_scratch(B, self.num_classes, pooled.device)
        p = _lib.ptr
        _lib.check(_lib.load().rgqa_maha_accumulate(p(pooled), pooled.stride(0), p(target), target.stride(0), B, self.hidden, self.num_classes, p(self.state),
                                                    p(scratch), nbytes, _stream(pooled.device)))

    def parts(self):
        """(n [NC], sums [NC, H], G [H, H]) as numpy f64"""
        s = self.state.cpu().numpy()
        NC, H = self.num_classes, self.hidden
        return s[:NC], s[NC:NC + NC * H].reshape(NC, H), s[NC + NC * H:].reshape(H, H)

    def finalize(self):
        mean, precision, W = maha_finalize(*self.parts())
        return _pack(mean, precision, W, self.device)


def _maha_model_check(model):
    from .butd.butd import GQABUTD, GQABUTD_maha
    if isinstance(model, GQABUTD) and not isinstance(model, GQABUTD_maha):
        raise NotImplementedError("maha: a plain BUTD GQABUTD returns no `joint_repr`, the vector the reference's Mahalanobis method scores on this backbone; "
                                  "build the model as GQABUTD_maha (same constructor and state_dict keys)")


def _maha_forward(model, feats, boxes, sent):
    out = model(feats, boxes, sent)
    if not (isinstance(out, tuple) and len(out) == 2):
        raise ValueError("maha: the model must return (logit, pooled) as GQAModel_maha / GQAUNITER_maha / GQABUTD_maha do")
    return out[1]


def maha_sample_estimator(model, batches):
    """gqa_maha.py:130-189 through a drop-in `GQAModel_maha` / `GQAUNITER_maha` / `GQABUTD_maha`: batches yields (feats, boxes, sent, target) with the UQ column of
    target already dropped (:141).  Runs under eval() and no_grad, restores the model's mode, returns the MahaPack."""
    _maha_model_check(model)
    was_training = model.training
    model.eval()
    est = None
    try:
        with torch.no_grad():
            for feats, boxes, sent, target in batches:
                x = _maha_forward(model, feats, boxes, sent)
                if est is None:
                    est = MahaEstimator(target.shape[1], x.shape[1], x.device)
                est.update(x, target.to(x.device, torch.float32))
    finally:
        model.train(was_training)
    if est is None:
        raise ValueError("maha_sample_estimator: no batches")
    return est.finalize()


def maha_score_rows(pooled, pack, all_scores=False):
    """pooled: f32 CUDA [B, H] (any row stride).  Returns MahaRows(score [B], label [B] int64, y [B, R], all_scores [B, NC] or None, pooled):
    score, label = gaussian_score.max(1) of gqa_maha.py:228-239 (ties: the lowest class), y = pooled W, pooled = the input, for `maha_dpooled`."""
    H, R = pack.W.shape
    NC = pack.nu.shape[0]
    pooled = _f32_rows("maha_score_rows: pooled", pooled, H)
    if pack.W.device != pooled.device:
        raise ValueError("maha_score_rows: the pack lives on another device")
    B, dev = pooled.shape[0], pooled.device
    y = torch.empty(B, R, dtype=torch.float32, device=dev)
    score = torch.empty(B, dtype=torch.float32, device=dev)
    label = torch.empty(B, dtype=torch.int64, device=dev)
    full = torch.empty(B, NC, dtype=torch.float32, device=dev) if all_scores else None
    scratch, nbytes = _maha_scratch(B, NC, dev)
    p = _lib.ptr
    _lib.check(_lib.load().rgqa_maha_score_rows(p(pooled), pooled.stride(0), p(pack.W), p(pack.nu), B, H, R, NC, p(y), p(score), p(label), p(full), NC if all_scores else 0,
                                                p(scratch), nbytes, _stream(dev)))
    return MahaRows(score, label, y, full, pooled)


def maha_dpooled(rows, pack):
    """d loss / d pooled [B, H] of loss = mean_b(-gaussian_score[b, label_b]) (gqa_maha.py:239-244) for the MahaRows of `maha_score_rows`:
    (1 / B) W W^T (pooled_b - mean[label_b]), the difference taken first as the reference takes it."""
    H, R = pack.W.shape
    NC = pack.nu.shape[0]
    x = _f32_rows("maha_dpooled: rows.pooled", rows.pooled, H)
    B = x.shape[0]
    if not isinstance(rows.label, torch.Tensor) or rows.label.dtype != torch.int64 or rows.label.shape != (B,) or rows.label.device != x.device or pack.W.device != x.device:
        raise ValueError("maha_dpooled: rows.label must be an int64 [B] tensor on the device of rows.pooled and the pack")
    label = rows.label.contiguous()
    d = torch.empty(B, R, dtype=torch.float32, device=x.device)
    out = torch.empty(B, H, dtype=torch.float32, device=x.device)
    p = _lib.ptr
    _lib.check(_lib.load().rgqa_maha_dpooled(p(x), x.stride(0), p(pack.mean), p(label), p(pack.W), 1.0 / B, B, H, R, NC, p(d), p(out), H,
                                             _stream(x.device)))
    return out


def maha_scores(model, feats, boxes, sent, pack, noise=0.0):
    """One batch of the reference's Mahalanobis scorer (gqa_maha.py:223-270) for `GQAModel_maha`, `GQAUNITER_maha` or `GQABUTD_maha` (drop-in classes): forward,
    `maha_score_rows`, `maha_dpooled`, backward from the pooled output with input gradients, two `sign_step`s, a second forward under no_grad on the
    perturbed inputs, `maha_score_rows`.  Returns MahaScores(score, label, pooled, feats_pt, boxes_pt): score / label = noised_gaussian_score.max(1)
    of the SECOND pass, its pooled vectors, and the perturbed inputs.  (`--temperature` is passed by the reference's script and never read.)

    `model.training` is honoured as the caller set it (the reference scores LXMERT / UNITER in eval() and BUTD in train() with dropout=False,
    gqa_maha.py:205-206); the pass never runs the data-parallel gradient exchange.  Afterwards the parameters' `.grad` hold the scoring pass's
    gradients, as after the reference's `loss.backward()` (BUTD: exact zeros for the answer classifier, which joint_repr does not pass through).  A
    plain `GQABUTD` (no `joint_repr`) raises NotImplementedError."""
    from .lxrt.modeling import scoring_pass
    _maha_model_check(model)
    f = feats.detach().contiguous().float().requires_grad_(True)
    b = boxes.detach().contiguous().float().requires_grad_(True)
    with scoring_pass():
        with torch.enable_grad():
            x = _maha_forward(model, f, b, sent)
        rows = maha_score_rows(x.detach(), pack)
        x.backward(maha_dpooled(rows, pack))
    feats_pt = sign_step(f.detach(), f.grad, noise)
    boxes_pt = sign_step(b.detach(), b.grad, noise)
    with torch.no_grad():
        x2 = _maha_forward(model, feats_pt, boxes_pt, sent)
    r2 = maha_score_rows(x2, pack)
    return MahaScores(r2.score, r2.label, x2, feats_pt, boxes_pt)


# ------------------------------------------------------------------------------------------------ energy fine-tuning (tasks/gqa_energy.py:117-145)
def _energy_loss_args(name, logits, target_with_uq, weight):
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("%s: logits must be a 2-D float32 CUDA tensor" % name)
    B, NA = logits.shape
    t = target_with_uq
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.device == logits.device and tuple(t.shape) == (B, NA + 1)):
        raise ValueError("%s: target_with_uq must be a float32 [B, NA + 1] = [%d, %d] tensor on the logits' device, the UQ column last" % (name, B, NA + 1))
    if not weight >= 0:
        raise ValueError("%s: weight must not be negative" % name)
    return (logits if logits.stride(1) == 1 else logits.contiguous()), (t if t.stride(1) == 1 else t.contiguous())


def energy_loss_rows(logits, target_with_uq, m_in=25.0, m_out=0.0, weight=0.1, mce_loss=False, grad_scale=1.0):
    """gqa_energy.py:122-138 and :144-145 on given logits, one fused pass (`rgqa_op_energy_loss`).  logits: f32 CUDA [B, NA], any row stride;
    target_with_uq: f32 [B, NA + 1], the last column the UQ flag (non-zero = unanswerable), read in place.  Returns EnergyLoss(loss, base, reg:
    0-dim views of one [3] tensor; dlogits [B, NA] = d loss / d logits * grad_scale; energy [B] = E_f; label [B] int64 = sigmoid(logit).max(1)[1]).
    An empty subset gives loss = reg = NaN and finite dlogits, as the reference's statements do."""
    z, t = _energy_loss_args("energy_loss_rows", logits, target_with_uq, weight)
    lib = _lib.load()
    B, NA = z.shape
    dev = z.device
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_energy_loss_scratch_floats(B, C.byref(n)))
    scratch = torch.empty(n.value, dtype=torch.float32, device=dev)
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    dl = torch.empty(B, NA, dtype=torch.float32, device=dev)
    en = torch.empty(B, dtype=torch.float32, device=dev)
    lab = torch.empty(B, dtype=torch.int64, device=dev)
    p = _lib.ptr
    _lib.check(lib.rgqa_op_energy_loss(p(z), z.stride(0), p(t), t.stride(0), C.c_void_p(t.data_ptr() + 4 * NA), t.stride(0), B, NA, NA, 1 if mce_loss else 0,
                                       float(weight), float(m_in), float(m_out), float(grad_scale), p(loss), p(dl), dl.stride(0), p(en), p(lab), p(scratch), _stream(dev)))
    return EnergyLoss(loss[0], loss[1], loss[2], dl, en, lab)


class _EnergyFinetuneLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target_with_uq, m_in, m_out, weight, mce_loss):
        r = energy_loss_rows(logit.detach(), target_with_uq, m_in, m_out, weight, mce_loss)
        ctx.save_for_backward(r.dlogits)
        ctx.mark_non_differentiable(r.energy, r.label)
        return r.loss.clone(), r.energy, r.label

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        dl, = ctx.saved_tensors
        return grad_loss * dl, None, None, None, None, None


def energy_finetune_loss(logit, target_with_uq, m_in, m_out, weight=0.1, mce_loss=False):
    """What a trainer puts in place of gqa_energy.py:122-138 and :144-145: `loss, score, label = energy_finetune_loss(model(feats, boxes, sent), target,
    args.m_in, args.m_out, mce_loss=args.mceLoss)` with `target` as the loader gives it (UQ column last); `loss.backward()`, `clip_grad_norm_` and
    `BertAdam.step()` stay as they are.  logit: the [B, NA] f32 CUDA output of GQAModel / GQAUNITER / GQABUTD.  Returns (loss 0-dim, E_f [B], label
    [B]): the forward runs the fused operator once and keeps dlogits, the backward hands `grad_output * dlogits` to the model's autograd boundary."""
    _energy_loss_args("energy_finetune_loss", logit, target_with_uq, weight)
    return _EnergyFinetuneLoss.apply(logit, target_with_uq, float(m_in), float(m_out), float(weight), bool(mce_loss))


# ------------------------------------------------------------------------------------------------ soft resampling (tasks/gqa_resampling.py:176-220)
def _resample_loss_args(name, logits, target_with_uq, n_pos, weights):
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("%s: logits must be a 2-D float32 CUDA tensor" % name)
    B, NA = logits.shape
    t = target_with_uq
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.device == logits.device and tuple(t.shape) == (B, NA + 1)):
        raise ValueError("%s: target_with_uq must be a float32 [B, NA + 1] = [%d, %d] tensor on the logits' device, the UQ column last" % (name, B, NA + 1))
    if not (isinstance(n_pos, int) and not isinstance(n_pos, bool) and 1 <= n_pos < B):
        raise ValueError("%s: n_pos must be an int with 1 <= n_pos < B = %d (positive rows first, at least one negative row)" % (name, B))
    w = weights
    if w is not None and not (isinstance(w, torch.Tensor) and w.dtype == torch.float32 and w.device == logits.device and tuple(w.shape) == (B - n_pos,)):
        raise ValueError("%s: weights must be a float32 [B - n_pos] = [%d] tensor on the logits' device" % (name, B - n_pos))
    return (logits if logits.stride(1) == 1 else logits.contiguous()), (t if t.stride(1) == 1 else t.contiguous())


def resample_loss_rows(logits, target_with_uq, n_pos, weights, grad_scale=1.0):
    """gqa_resampling.py:196-202 on given logits of the concatenated batch, one fused pass (`rgqa_op_resample_loss`).  logits: f32 CUDA [B, NA], any row
    stride, rows [0, n_pos) positive and the rest negative; target_with_uq: f32 [B, NA + 1] as the loader gives it (the UQ column is dropped at :176-177
    and is not read here); weights: f32 [B - n_pos] (ResampleWeights.batch_weights).  Returns ResampleLoss(loss, loss_pos, loss_neg: 0-dim views of one
    [3] tensor; dlogits [B, NA] = d loss / d logits * grad_scale; row_loss [B - n_pos] = the negative rows' BCE sums)."""
    z, t = _resample_loss_args("resample_loss_rows", logits, target_with_uq, n_pos, weights)
    if weights is None:
        raise ValueError("resample_loss_rows: weights must be a float32 [B - n_pos] tensor")
    lib = _lib.load()
    B, NA = z.shape
    dev = z.device
    w = weights.contiguous()
    n = C.c_size_t()
    _lib.check(lib.rgqa_resample_scratch_floats(1, B, C.byref(n)))
    scratch = torch.empty(n.value, dtype=torch.float32, device=dev)
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    dl = torch.empty(B, NA, dtype=torch.float32, device=dev)
    rl = torch.empty(B - n_pos, dtype=torch.float32, device=dev)
    p = _lib.ptr
    _lib.check(lib.rgqa_op_resample_loss(p(z), z.stride(0), p(t), t.stride(0), B, n_pos, NA, NA, p(w), float(grad_scale), p(loss), p(dl), dl.stride(0), p(rl), p(scratch),
                                         _stream(dev)))
    return ResampleLoss(loss[0], loss[1], loss[2], dl, rl)


class _ResampleFinetuneLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, target_with_uq, n_pos, weights):
        r = resample_loss_rows(logit.detach(), target_with_uq, n_pos, weights)
        ctx.save_for_backward(r.dlogits)
        loss_w = -r.loss_neg
        ctx.mark_non_differentiable(loss_w, r.row_loss)
        return r.loss.clone(), loss_w, r.row_loss

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        dl, = ctx.saved_tensors
        return grad_loss * dl, None, None, None


def resample_finetune_loss(logit, target_with_uq, n_pos, rw, wids):
    """What a trainer puts in place of gqa_resampling.py:183-203: `loss, loss_w = resample_finetune_loss(model(cat(feats_pos, feats_neg), cat(boxes_pos,
    boxes_neg), sent_pos + sent_neg), cat(target_pos, target_neg), len(sent_pos), rw, wids)` with the targets as the loader gives them (UQ column
    last), `rw` a rgqa_amd.resample.ResampleWeights and `wids` the weight-parameter indices of the negative rows (:183).  Then `optim.zero_grad();
    loss.backward(); clip_grad_norm_; optim.step(); rw.step()`.  logit: the [B, NA] f32 CUDA output of GQAModel / GQAUNITER / GQABUTD.  Returns (loss
    0-dim, loss_w 0-dim = -loss_neg, not differentiable: rw.step() has the gradient in closed form).  The forward computes the batch weights, runs the
    fused operator once, keeps dlogits and leaves the negative rows' losses on `rw`; the backward hands `grad_output * dlogits` to the model's autograd
    boundary."""
    _resample_loss_args("resample_finetune_loss", logit, target_with_uq, n_pos, None)
    if not (hasattr(rw, "batch_weights") and hasattr(rw, "step")):
        raise ValueError("resample_finetune_loss: rw must be a rgqa_amd.resample.ResampleWeights")
    if len(wids) != logit.shape[0] - n_pos:
        raise ValueError("resample_finetune_loss: %d indices for %d negative rows" % (len(wids), logit.shape[0] - n_pos))
    weights = rw.batch_weights(wids)
    loss, loss_w, row_loss = _ResampleFinetuneLoss.apply(logit, target_with_uq, n_pos, weights)
    rw.row_loss = row_loss
    return loss, loss_w


# ------------------------------------------------------------------------------------------------ confidence branch (tasks/gqa_branched.py)
def _branched_args(name, logits, conf, target_with_uq):
    if not (isinstance(logits, torch.Tensor) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2):
        raise ValueError("%s: logits must be a 2-D float32 CUDA tensor" % name)
    B, NA = logits.shape
    if not (isinstance(conf, torch.Tensor) and conf.dtype == torch.float32 and conf.device == logits.device and conf.numel() == B and conf.dim() in (1, 2)):
        raise ValueError("%s: conf must be a float32 [B] or [B, 1] = [%d] tensor on the logits' device" % (name, B))
    t = target_with_uq
    if not (isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.dim() == 2 and t.device == logits.device and tuple(t.shape) == (B, NA + 1)):
        raise ValueError("%s: target_with_uq must be a float32 [B, NA + 1] = [%d, %d] tensor on the logits' device, the UQ column last" % (name, B, NA + 1))
    return (logits if logits.stride(1) == 1 else logits.contiguous()), conf.reshape(-1).contiguous(), (t if t.stride(1) == 1 else t.contiguous())


def branched_loss_rows(logits, conf, target_with_uq, mce_loss=False, grad_scale=1.0):
    """gqa_branched.py:126-142, :147 and :209 on given logits and conf logits, one fused pass (`rgqa_op_branched_loss`).  logits: f32 CUDA [B, NA], any row
    stride; conf: f32 [B] or [B, 1] conf LOGITS (before the sigmoid); target_with_uq: f32 [B, NA + 1], the last column the UQ flag (non-zero =
    unanswerable), read in place.  Returns BranchedLoss(loss, loss_ce, loss_conf: 0-dim views of one [3] tensor; dlogits [B, NA] and dconf [B] = d loss / d
    logits, d loss / d conf logits, times grad_scale; conf [B] = sigmoid(conf); label [B] int64 = logit.max(1)[1]; score1 [B] = sigmoid(logit).max(1)[0]).
    No answerable row gives loss = loss_ce = NaN and finite gradients, as the reference's statements do.  loss_conf is formed in the stable form
    max(c, 0) - c y + log1p(exp(-|c|)) (each term capped at 100): it departs from torch's f32 statements where their sigmoid saturates (|c| >~ 17)."""
    z, c, t = _branched_args("branched_loss_rows", logits, conf, target_with_uq)
    lib = _lib.load()
    B, NA = z.shape
    dev = z.device
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_branched_loss_scratch_floats(B, C.byref(n)))
    scratch = torch.empty(n.value, dtype=torch.float32, device=dev)
    loss = torch.empty(3, dtype=torch.float32, device=dev)
    dl = torch.empty(B, NA, dtype=torch.float32, device=dev)
    dc, cf, s1 = (torch.empty(B, dtype=torch.float32, device=dev) for _ in range(3))
    lab = torch.empty(B, dtype=torch.int64, device=dev)
    p = _lib.ptr
    _lib.check(lib.rgqa_op_branched_loss(p(z), z.stride(0), p(c), p(t), t.stride(0), B, NA, NA, 1 if mce_loss else 0, float(grad_scale), p(loss), p(dl), dl.stride(0),
                                         p(dc), p(cf), p(lab), p(s1), p(scratch), _stream(dev)))
    return BranchedLoss(loss[0], loss[1], loss[2], dl, dc, cf, lab, s1)


class _BranchedFinetuneLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logit, conf, target_with_uq, mce_loss):
        r = branched_loss_rows(logit.detach(), conf.detach(), target_with_uq, mce_loss)
        ctx.save_for_backward(r.dlogits, r.dconf)
        ctx.conf_shape = tuple(conf.shape)
        ctx.mark_non_differentiable(r.loss_ce, r.loss_conf, r.conf, r.label)
        return r.loss.clone(), r.loss_ce, r.loss_conf, r.conf, r.label

    @staticmethod
    def backward(ctx, grad_loss, *unused):
        dl, dc = ctx.saved_tensors
        return grad_loss * dl, (grad_loss * dc).view(ctx.conf_shape), None, None


def branched_finetune_loss(logit, conf, target_with_uq, mce_loss=False):
    """What a trainer puts in place of gqa_branched.py:126-142 and :147: `loss, loss_ce, loss_conf, conf, label = branched_finetune_loss(*model(feats, boxes,
    sent), target, mce_loss=args.mce_loss)` with `target` as the loader gives it (UQ column last); `loss.backward()`, `clip_grad_norm_` and `BertAdam.step()`
    stay as they are.  logit [B, NA], conf [B, 1]: the outputs of GQAModel_branched.  Returns (loss 0-dim, loss_ce, loss_conf, sigmoid(conf) [B], label [B]):
    the forward runs the fused operator once and keeps dlogits and dconf, the backward hands both to the model's autograd boundary - ONE engine backward."""
    _branched_args("branched_finetune_loss", logit, conf, target_with_uq)
    return _BranchedFinetuneLoss.apply(logit, conf, target_with_uq, bool(mce_loss))


def branched_scores(model, feats, boxes, sent, mix=False):
    """One batch of the branched model's OOD scorer (gqa_branched.py:206-214) under no_grad: score = sigmoid(conf), or with mix=True (--mix_branched_score)
    sigmoid(conf) * max sigmoid(logit); label = sigmoid(logit).max(1)[1].  Returns (score [B], label [B] int64)."""
    with torch.no_grad():
        logit, conf = model(feats, boxes, sent)
    s = score_rows(logit)
    score2 = torch.sigmoid(conf).reshape(-1)
    return (s.max_score * score2 if mix else score2), s.label
