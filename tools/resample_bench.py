"""Time of the soft-resampling step's weight side (tasks/gqa_resampling.py:183-186, :196-203, :218-220; csrc/resample.hip) at N = 1e5 and 1e6 weight
parameters with B = 32 + 32 (the reference script's batch size) and 128 + 128 rows at NA = 1842, and of the engine-direct LXMERT train step that uses it.
Legs alternate in one process after a warm-up; every call of a window is bracketed by device events and the window reports their mean:

    fused   ResampleWeights.batch_weights + scoring.resample_loss_rows + ResampleWeights.step  (six launches and one small upload)
    torch   the reference statements on the device with torch ops: softplus / means / gather, the two BCE terms, loss.backward() to the logits,
            optim_w.zero_grad(); loss_w.backward(); torch.optim.SGD(momentum=0.9).step()
    step_bce       Engine (LXMERT, full size, B = 256, T = 20, packed rows): forward(train) + loss_backward + adam_step - bench.py's step, whose kernels
                   this feature leaves untouched (the step of the commit before it)
    step_resample  the same step on 128 + 128 rows: batch_weights + forward + resample_loss_backward + adam_step + ResampleWeights.step (N = 1e6)

    timeout 600 python tools/resample_bench.py [--sizes 100000,1000000] [--batches 32,128] [--precision bf16x3_fwd] [--skip-step]

Prints one JSON line per (N, batch) and one for the step legs: median ms of each leg over the windows with min / max, the device launches per call of
both forms (counted with torch.profiler on one call outside the timed windows), and how far the two forms' results are apart.  Not part of bench.py."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FULL, init_params      # noqa: E402  (the flagship configuration and its random initialisation)

NA = FULL["num_answers"]
LR_W = 1.0                                # (the reference's default is 100; the legs repeat ONE batch hundreds of times, which that rate would drive to overflow)


def draw(N, half, seed=7):
    """theta 2 randn; `half` positive rows with two soft entries, `half` negative rows with all-zero answers; indices drawn with replacement"""
    rng = np.random.RandomState(seed)
    theta = (2.0 * rng.standard_normal(N)).astype(np.float32)
    B = 2 * half
    z = (3.0 * rng.standard_normal((B, NA)) - 6.0).astype(np.float32)
    t = np.zeros((B, NA + 1), np.float32)
    for b in range(half):
        c = rng.choice(NA, 2, replace=False)
        t[b, c[0]], t[b, c[1]] = 0.9, 0.3
    t[half:, NA] = 1.0
    wids = torch.from_numpy(rng.randint(N, size=half).astype(np.int64))
    return torch.from_numpy(theta).cuda(), wids, torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda()


class TorchStatements:
    """gqa_resampling.py:139-140, :176-177, :183-186, :196-203, :214-220 with device torch ops (the model's backward stops at the logits)"""

    def __init__(self, theta):
        self.weight_params = torch.nn.Parameter(theta.clone())
        self.optim_w = torch.optim.SGD([self.weight_params], LR_W, momentum=0.9)
        self.bce_loss = torch.nn.BCEWithLogitsLoss(reduction='none')

    def step(self, logit, target, n_pos, wids):
        logit = logit.detach().requires_grad_(True)
        logit_pos, logit_neg = logit[:n_pos], logit[n_pos:]
        target_pos, target_neg = target[:n_pos, :-1], target[n_pos:, :-1]
        w = torch.nn.functional.softplus(self.weight_params)
        scale = (w ** .5).mean() / (w.mean() ** .5)
        weights = scale * (w[wids.cuda()] / w.mean()) ** .5
        loss_pos = self.bce_loss(logit_pos, target_pos)
        loss_pos = torch.mean(loss_pos) * logit_pos.size(1)
        loss_neg = self.bce_loss(logit_neg, target_neg)
        loss_neg = (weights.view(1, len(wids)) @ loss_neg).sum() / len(wids)
        loss = loss_pos + loss_neg
        loss_w = -loss_neg
        loss.backward(retain_graph=True)
        self.optim_w.zero_grad()
        loss_w.backward()
        self.optim_w.step()
        return loss.detach(), logit.grad


def launches(fn):
    """device kernels and memory operations of one call"""
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    try:
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        return sum(1 for ev in prof.events() if str(ev.device_type).endswith("CUDA"))
    except Exception as ex:                                     # no device tracing in this build of torch: the timings do not depend on it
        return "not counted (%s)" % type(ex).__name__


def time_legs(legs, windows, iters, warm=3):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(iters)]
            torch.cuda.synchronize()
            for a, b in evs:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            times[k].append(float(np.mean([a.elapsed_time(b) for a, b in evs])))
    out = {}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    return out


def op_legs(N, half):
    from rgqa_amd import scoring
    from rgqa_amd.resample import ResampleWeights
    theta, wids, z, t = draw(N, half)
    rw = ResampleWeights(N, LR_W)
    ts = TorchStatements(theta)

    def fused():
        w = rw.batch_weights(wids)
        r = scoring.resample_loss_rows(z, t, half, w)
        rw.step(r.row_loss)
        return r

    # what is timed computes the same thing (one step of each from the same theta)
    rw.theta.copy_(theta)
    r = fused()
    loss_t, dl_t = ts.step(z, t, half, wids)
    torch.cuda.synchronize()
    dth = (rw.theta - theta).abs().max()
    agree = dict(loss_rel=abs(float(r.loss) - float(loss_t)) / abs(float(loss_t)), dlogits_rel_max=float((r.dlogits - dl_t).abs().max() / dl_t.abs().max()),
                 theta_update_rel_max=float((rw.theta - ts.weight_params.detach()).abs().max() / dth))
    legs = {"fused": fused, "torch": lambda: ts.step(z, t, half, wids)}
    counts = dict(fused_launches=launches(fused), torch_launches=launches(legs["torch"]))
    return legs, {k: round(v, 10) for k, v in agree.items()}, counts


def step_legs(precision, N):
    from rgqa_amd import synth
    from rgqa_amd.engine import Engine
    from rgqa_amd.resample import ResampleWeights
    B, T, O = 256, 20, 36
    e = Engine(precision=precision, **FULL).allocate("cuda")
    init_params(e, seed=0)
    b = synth.synth_batch(B, T, seed=1234)
    dev = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}
    lengths = np.ascontiguousarray(b["lengths"], dtype=np.int32)
    n_pos = B // 2
    tuq = torch.zeros(B, NA + 1, device="cuda")
    tuq[:n_pos, :NA] = dev["target"][:n_pos]
    tuq[n_pos:, NA] = 1.0                                       # the second half: negative rows, no answers
    rw = ResampleWeights(N, LR_W)
    rw.theta.copy_(torch.from_numpy((2.0 * np.random.RandomState(3).standard_normal(N)).astype(np.float32)))
    wids = torch.from_numpy(np.random.RandomState(4).randint(N, size=B - n_pos).astype(np.int64))
    e.ensure_shape(B, T, O)
    e.sync_weights()
    e.enable_segment_sumsq(True)
    state = dict(i=0)

    def step(resample):
        i = state["i"]
        if resample:
            w = rw.batch_weights(wids)
        e.forward(dev["feats"], dev["boxes"], dev["input_ids"], dev["input_mask"], dev["segment_ids"], train=True, seed=4321 + 1000003 * i, lengths=lengths)
        if resample:
            _, row_loss = e.resample_loss_backward(tuq, n_pos, w)
        else:
            e.loss_backward(dev["target"])
        e.adam_step(1e-5, max_norm=5.0)
        if resample:
            rw.step(row_loss)
        state["i"] = i + 1
    return {"step_bce": lambda: step(False), "step_resample": lambda: step(True)}, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000")
    ap.add_argument("--batches", default="32,128", help="rows per half: B = 32 + 32 and 128 + 128")
    ap.add_argument("--precision", default="bf16x3_fwd")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="operator legs: calls per window")
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-ops", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("resample_bench: needs an MI355X (no GPU found; there is no CPU path)")
    if not a.skip_ops:
        for N in (int(x) for x in a.sizes.split(",")):
            for half in (int(x) for x in a.batches.split(",")):
                legs, agree, counts = op_legs(N, half)
                out = dict(weight_params=N, batch="%d+%d" % (half, half), num_answers=NA, windows=a.windows, iters=a.iters, agreement_with_torch=agree)
                out.update(counts)
                out.update(time_legs(legs, a.windows, a.iters))
                print(json.dumps(out), flush=True)
    if not a.skip_step:
        N = max(int(x) for x in a.sizes.split(","))
        sl, e = step_legs(a.precision, N)
        out = dict(leg="step", weight_params=N, batch="128+128", precision=a.precision, step_iters=a.step_iters, windows=a.windows)
        out.update(step_bce_launches=launches(sl["step_bce"]), step_resample_launches=launches(sl["step_resample"]))
        out.update(time_legs(sl, a.windows, a.step_iters, warm=5))
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
