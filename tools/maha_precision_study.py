"""f32 emulation on the host of the arithmetic of csrc/maha.hip (sequential FMA sums in f32) against an f64 evaluation, next to the error of the
reference's own f32 torch statements (tasks/gqa_maha.py:228-244) against the same f64: the ratio the 8 x bound of tests/test_gpu_maha.py is about.
Scores in the factored form sum_r (y - nu)^2, and the input step in two forms: W (y - nu_pred), the difference after the products, and
W W^T (x - mu_pred), the difference first (the form the library uses).  Fixture cases and one synthetic case (H = 768, NC = 1842, B = 32).  No GPU.

    python tools/maha_precision_study.py
"""
import os
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from rgqa_amd import scoring
f32 = np.float32

def torch_f32(x, mean, P):
    x, mean, P = torch.from_numpy(x), torch.from_numpy(mean), torch.from_numpy(P.astype(np.float32))
    cols = []
    for i in range(mean.shape[0]):
        z = x - mean[i]
        cols.append((-0.5 * torch.mm(torch.mm(z, P), z.t()).diag()).view(-1, 1))
    return torch.cat(cols, 1).numpy()

def f64_scores(x, mean, P):
    x, mean = x.astype(np.float64), mean.astype(np.float64)
    XP = x @ P
    return -0.5 * ((XP * x).sum(1)[:, None] - 2 * XP @ mean.T + ((mean @ P) * mean).sum(1)[None, :])

def emu(x, W, nu):
    B, H = x.shape; R = W.shape[1]
    y = np.zeros((B, R), f32)
    for k in range(H): y = (y.astype(np.float64) + x[:, k:k+1].astype(np.float64) * W[k].astype(np.float64)).astype(f32)   # fma
    acc = np.zeros((B, nu.shape[0]), f32)
    for r in range(R):
        d = (y[:, r][:, None] - nu[:, r][None, :]).astype(f32)
        acc = (acc.astype(np.float64) + d.astype(np.float64) * d.astype(np.float64)).astype(f32)
    return f32(-0.5) * acc, y

def case(name, x, mean, P):
    W64, Ps = scoring.maha_factor(P)
    W = W64.astype(f32); nu = (mean.astype(np.float64) @ W64).astype(f32)
    ref64 = f64_scores(x, mean, P)
    t = time.time(); r32 = torch_f32(x, mean, P); tt = time.time() - t
    e_ref = np.abs(r32 - ref64).max()
    s, y = emu(x, W, nu)
    e_dev = np.abs(s - ref64).max()
    print(name, "ref_f32_err %.3e dev-emu err %.3e ratio %.2f  (|score| max %.3e, torch loop %.1fs) labels eq %s" % (e_ref, e_dev, e_dev / e_ref, np.abs(ref64).max(), tt, np.array_equal(s.argmax(1), ref64.argmax(1))))
    # dpooled
    lab = ref64.argmax(1); B = x.shape[0]
    g64 = (x.astype(np.float64) - mean[lab].astype(np.float64)) @ P / B
    xt = torch.from_numpy(x).requires_grad_(True)
    z = xt - torch.from_numpy(mean)[torch.from_numpy(lab)]
    Pt = torch.from_numpy(P.astype(f32))
    loss = torch.mean(-(-0.5 * torch.mm(torch.mm(z, Pt), z.t()).diag())); loss.backward()
    e_ref = np.abs(xt.grad.numpy() - g64).max() / np.abs(g64).max()
    zc = (x - mean[lab]).astype(f32)
    dz = np.zeros((B, W.shape[1]), f32)
    for k in range(x.shape[1]): dz = (dz.astype(np.float64) + zc[:, k:k+1].astype(np.float64) * W[k].astype(np.float64)).astype(f32)
    for form, d in (("W (y - nu_pred)", (y - nu[lab]).astype(f32)), ("W W^T (x - mu_pred)", dz)):
        g = np.zeros_like(x)
        for r in range(W.shape[1]): g = (g.astype(np.float64) + d[:, r:r+1].astype(np.float64) * W[:, r][None, :].astype(np.float64)).astype(f32)
        g = g * f32(1.0 / B)
        e_dev = np.abs(g - g64).max() / np.abs(g64).max()
        print(name, "dpooled as %s: ref err %.3e emulated %.3e ratio %.2f" % (form, e_ref, e_dev, e_dev / e_ref))

def synth_case(B, H=768, NC=1842, seed=0):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((H, H)))
    lam = np.exp(rng.uniform(np.log(1e-4), np.log(1e-2), H))       # covariance eigenvalues: condition 1e2
    cov = (Q * lam) @ Q.T
    P = (Q / lam) @ Q.T
    mean = (0.3 * rng.standard_normal((NC, H))).astype(f32)
    mean[rng.choice(NC, 40, replace=False)] = 0.0
    lab = rng.randint(0, NC, B)
    x = (mean[lab] + (rng.standard_normal((B, H)) * np.sqrt(lam)) @ Q.T).astype(f32)
    return x, mean, P
if __name__ == "__main__":
    torch.set_num_threads(max(1, min(16, len(os.sched_getaffinity(0)))))
    g = np.load(os.path.join(ROOT, 'tests', 'golden', 'g13_maha.npz'))
    for bb in ("lxmert", "uniter"):
        case(bb, g[bb + ".pooled"], g[bb + ".mean"], g[bb + ".precision"])
    x, mean, P = synth_case(32)
    case("synth B=32", x, mean, P)
