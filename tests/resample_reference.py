"""The reference's soft-resampling step (tasks/gqa_resampling.py:176-220, the lxmert / uniter order of :213-220) restated with torch, its closed-form
weight-parameter gradient, and the inputs the resampling tests draw.  Shared by tests/test_resample_host.py and tests/test_gpu_resample.py; runs on
the CPU in the dtype it is asked for."""
import numpy as np
import torch
import torch.nn.functional as F


def reference_statements(theta, wids, logit_pos, target_pos, logit_neg, target_neg):
    """gqa_resampling.py:176-203; the targets carry the UQ column last.  Returns (loss, loss_pos, loss_neg, loss_w, weights, row_loss)."""
    target_pos = target_pos[:, :-1]                                                 # :176
    target_neg = target_neg[:, :-1]                                                 # :177
    w = F.softplus(theta)                                                           # :184
    scale = (w ** .5).mean() / (w.mean() ** .5)                                     # :185
    weights = scale * (w[wids] / w.mean()) ** .5                                    # :186
    bce_loss = torch.nn.BCEWithLogitsLoss(reduction='none')                         # :121
    loss_pos = bce_loss(logit_pos, target_pos)                                      # :196
    loss_pos = torch.mean(loss_pos) * logit_pos.size(1)                             # :197
    loss_neg = bce_loss(logit_neg, target_neg)                                      # :199
    row_loss = loss_neg.sum(1)
    loss_neg = (weights.view(1, len(wids)) @ loss_neg).sum() / len(wids)            # :200
    loss = loss_pos + loss_neg                                                      # :202
    loss_w = -loss_neg                                                              # :203
    return loss, loss_pos, loss_neg, loss_w, weights, row_loss


def weight_loss(theta, wids, row_loss):
    """loss_w = -loss_neg (:184-186, :200, :203) as a function of theta alone, for given row sums r_b of the negative rows' BCE"""
    w = F.softplus(theta)
    scale = (w ** .5).mean() / (w.mean() ** .5)
    weights = scale * (w[wids] / w.mean()) ** .5
    return -(weights * row_loss).sum() / len(wids)


def closed_form_dtheta(theta, wids, row_loss):
    """d loss_w / d theta without autograd: with S = sum_b r_b sqrt(w[wid_b]) and s_j = sum over {b: wid_b = j} of r_b,
    d loss_w / d w_j = -(1 / Bn) [ S / (2 N m1 sqrt w_j) - mh S / (N m1^2) + (mh / (2 m1)) s_j / sqrt w_j ], times sigmoid(theta_j) (1 above 20)"""
    N, Bn = theta.numel(), len(wids)
    w = F.softplus(theta)
    m1, mh = w.mean(), w.sqrt().mean()
    S = (row_loss * w[wids].sqrt()).sum()
    s = torch.zeros_like(theta).index_add_(0, wids, row_loss)
    dw = -(S / (2 * N * m1 * w.sqrt()) - mh * S / (N * m1 ** 2) + (mh / (2 * m1)) * s / w.sqrt()) / Bn
    return dw * torch.where(theta > 20, torch.ones_like(theta), torch.sigmoid(theta))


def evaluate(theta, wids, z, target_uq, n_pos, dtype, lr_w=0.5, momentum=0.9, more_steps=()):
    """the statements on the concatenated batch (rows [0, n_pos) positive) in `dtype` on the CPU, loss.backward() to the logits, then the trainer's
    weight step (:218-220: optim_w.zero_grad(); loss_w.backward(); optim_w.step() with torch.optim.SGD), followed by one further step per
    (wids, row_loss) pair of `more_steps` (row sums given, cast to `dtype`).  Returns a dict of f64 tensors: weights, loss, loss_pos, loss_neg, dlogits,
    row_loss, dtheta (of the first step), dthetas (of every step), theta / buf (after the last step), max_buf (max |buf| after each step)."""
    th = theta.detach().to(dtype).clone().requires_grad_(True)
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    t = target_uq.to(dtype)
    optim_w = torch.optim.SGD([th], lr_w, momentum=momentum)                        # :140
    loss, loss_pos, loss_neg, loss_w, weights, row_loss = reference_statements(th, wids, zz[:n_pos], t[:n_pos], zz[n_pos:], t[n_pos:])
    loss.backward(retain_graph=True)                                                # :215
    dlogits = zz.grad.detach().clone()
    optim_w.zero_grad()                                                             # :218
    loss_w.backward()                                                               # :219
    dthetas = [th.grad.detach().double().clone()]
    optim_w.step()                                                                  # :220
    max_buf = [float(optim_w.state[th]["momentum_buffer"].abs().max())]
    for wk, rk in more_steps:
        optim_w.zero_grad()
        weight_loss(th, wk, rk.to(dtype)).backward()
        dthetas.append(th.grad.detach().double().clone())
        optim_w.step()
        max_buf.append(float(optim_w.state[th]["momentum_buffer"].abs().max()))
    d = lambda x: x.detach().double().clone()
    return dict(weights=d(weights), loss=d(loss), loss_pos=d(loss_pos), loss_neg=d(loss_neg), loss_w=d(loss_w), dlogits=d(dlogits), row_loss=d(row_loss),
                dtheta=dthetas[0], dthetas=dthetas, theta=d(th), buf=d(optim_w.state[th]["momentum_buffer"]), max_buf=max_buf)


def draw_wids(N, Bn, rng):
    """[Bn] int64: N // 2, N - 1 and 0 first (as many as fit), for Bn >= 7 one index three times, the rest uniform draws - then shuffled"""
    w = [N // 2, N - 1, 0][:Bn]
    if Bn >= 7:
        w += [int(rng.randint(N))] * 3
    w += [int(i) for i in rng.randint(N, size=Bn - len(w))]
    return torch.tensor([w[i] for i in rng.permutation(Bn)], dtype=torch.int64)


def draw(N, n_pos, Bn, NA, seed):
    """theta [N] = 2 randn with theta[N // 2] = 25 (above softplus's threshold) and theta[N - 1] = -12 for N >= 3; wids [Bn] (draw_wids); logits
    [n_pos + Bn, NA] = 3 randn - 6 (as tests/energy_reference.draw); targets [n_pos + Bn, NA + 1]: two soft entries (0.9, 0.3) per positive row,
    all-zero answers and UQ column 1 for the negative rows.  All on the CPU, f32 / int64."""
    rng = np.random.RandomState(seed)
    theta = (2.0 * rng.standard_normal(N)).astype(np.float32)
    if N >= 3:
        theta[N // 2], theta[N - 1] = 25.0, -12.0
    wids = draw_wids(N, Bn, rng)
    B = n_pos + Bn
    z = (3.0 * rng.standard_normal((B, NA)) - 6.0).astype(np.float32)
    t = np.zeros((B, NA + 1), np.float32)
    for b in range(B):
        if b < n_pos:
            c = rng.choice(NA, 2, replace=False)
            t[b, c[0]], t[b, c[1]] = 0.9, 0.3
        else:
            t[b, NA] = 1.0
    return torch.from_numpy(theta), wids, torch.from_numpy(z), torch.from_numpy(t)


def draw_steps(N, Bn, k, seed):
    """k further (wids, row_loss) pairs: fresh indices and row sums 5 + 10 U(0, 1) in f32"""
    rng = np.random.RandomState(seed)
    return [(draw_wids(N, Bn, rng), torch.from_numpy((5.0 + 10.0 * rng.random_sample(Bn)).astype(np.float32))) for _ in range(k)]
