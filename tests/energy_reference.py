"""The reference's energy fine-tuning loss (tasks/gqa_energy.py:117-145) restated with torch, and the inputs the energy-loss tests draw.  Shared
by tests/test_energy_loss_host.py and tests/test_gpu_energy_loss.py; runs on the CPU in the dtype of the logits it is given."""
import numpy as np
import torch


def reference_statements(logit, target, m_in, m_out, mce_loss=False, weight=0.1):
    """gqa_energy.py:122-138 and :144-145 (the constant 0.1 of :137-138 is `weight`).  target carries the UQ column last.
    Returns (loss, base, reg, E_f, label)."""
    id_inds = target[:, -1] == 0                                                    # :122
    target = target[:, :-1]                                                         # :123
    if mce_loss:
        _, tgt = target.max(1)                                                      # :128
        loss = torch.nn.CrossEntropyLoss(ignore_index=-1)(logit, tgt)               # :129
        loss = loss * logit.size(1)                                                 # :130
        E_f = torch.logsumexp(logit, dim=1)                                         # :131
    else:
        loss = torch.nn.BCEWithLogitsLoss()(logit, target)                          # :133
        loss = loss * logit.size(1)                                                 # :134
        E_f = torch.log(1 + torch.exp(logit)).sum(1)                                # :135
    base = loss
    reg = weight * (torch.relu(-E_f[id_inds] - m_in) ** 2).mean() + weight * (torch.relu(m_out + E_f[~id_inds]) ** 2).mean()      # :137-138
    loss = base + reg
    _, label = torch.sigmoid(logit).max(1)                                          # :144
    return loss, base, reg, E_f, label


def evaluate(z, target_uq, m_in, m_out, mce_loss, dtype, weight=0.1):
    """the statements and their backward to the logits in `dtype` on the CPU: dict(loss, base, reg, energy, dlogits, label), all f64 / int64"""
    zz = z.detach().to(dtype).clone().requires_grad_(True)
    loss, base, reg, E, label = reference_statements(zz, target_uq.to(dtype), m_in, m_out, mce_loss, weight)
    loss.backward()
    d = lambda t: t.detach().double()
    return dict(loss=d(loss), base=d(base), reg=d(reg), energy=d(E), dlogits=d(zz.grad), label=label)


def draw(B, NA, seed, ood="third"):
    """logits 3 randn - 6; OOD rows (UQ column 1, all-zero answers): every third row starting at row 1 ("third"), none ("none") or all ("all"); two
    soft target entries (0.9, 0.3) per ID row.  Returns (logits [B, NA] f32, target_with_uq [B, NA + 1] f32) on the CPU."""
    rng = np.random.RandomState(seed)
    z = (3.0 * rng.standard_normal((B, NA)) - 6.0).astype(np.float32)
    t = np.zeros((B, NA + 1), np.float32)
    for b in range(B):
        is_ood = {"third": b % 3 == 1, "none": False, "all": True}[ood]
        if is_ood:
            t[b, NA] = 1.0
        else:
            c = rng.choice(NA, 2, replace=False)
            t[b, c[0]], t[b, c[1]] = 0.9, 0.3
    return torch.from_numpy(z), torch.from_numpy(t)


def _f32_at_least(x):
    v = np.float32(x)
    return float(v if float(v) >= x else np.nextafter(v, np.float32(np.inf)))


def margins(z, target_uq, mce_loss):
    """m_in / m_out = the negated f64 medians (torch.median: the lower middle) of the ID / OOD energies as f32 numbers, the C ABI's type - rounded to the
    side that keeps the median row's hinge at or below zero, as it is at the exact median: rows below the ID median / above the OOD median are
    active, so a subset of >= 3 (ID) / >= 2 (OOD) rows has active and inactive hinges.  A subset that is empty keeps the reference's defaults 25 / 0.
    Returns (m_in, m_out, E_f in f64)."""
    with torch.no_grad():
        E = reference_statements(z.double(), target_uq.double(), 0.0, 0.0, mce_loss)[3]
    idm = target_uq[:, -1] == 0
    m_in = _f32_at_least(-float(E[idm].median())) if bool(idm.any()) else 25.0              # -E - m_in <= 0 at the median row
    m_out = -_f32_at_least(float(E[~idm].median())) if bool((~idm).any()) else 0.0          # m_out + E <= 0 at the median row
    return m_in, m_out, E
