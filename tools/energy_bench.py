"""Time of the energy fine-tuning's loss head (tasks/gqa_energy.py:122-138, :144-145; rgqa_op_energy_loss) at NA = 1842, B = 256 and 64, and of the
engine-direct LXMERT train step that uses it.  Legs alternate in one process after a warm-up, each window bracketed by device synchronisation:

    op      rgqa_op_energy_loss into preallocated buffers: loss, dlogits, energy, label (two launches)
    rows    scoring.energy_loss_rows: the same plus its six allocations and the scratch query
    torch   the reference statements :122-138 and :144-145 on the device with their backward to the logits (torch eager)
    step_bce     Engine (LXMERT, full size, T = 20, packed rows): forward(train) + loss_backward + adam_step - bench.py's step, whose loss kernels
                 are untouched by the energy loss (the step of the commit before it)
    step_energy  the same step with energy_loss_backward on the target with its UQ column

    timeout 600 python tools/energy_bench.py [--batches 256,64] [--precision bf16x3_fwd] [--mce] [--skip-step]

Prints one JSON line per batch size: median ms of each leg over the windows, with min / max.  Not part of bench.py."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FULL, init_params      # noqa: E402  (the flagship configuration and its random initialisation)

NA = FULL["num_answers"]


def draw(B, seed=7):
    """logits 3 randn - 6, every third row OOD, two soft target entries per ID row (as tests/energy_reference.py)"""
    rng = np.random.RandomState(seed)
    z = (3.0 * rng.standard_normal((B, NA)) - 6.0).astype(np.float32)
    t = np.zeros((B, NA + 1), np.float32)
    for b in range(B):
        if b % 3 == 1:
            t[b, NA] = 1.0
        else:
            c = rng.choice(NA, 2, replace=False)
            t[b, c[0]], t[b, c[1]] = 0.9, 0.3
    return torch.from_numpy(z).cuda(), torch.from_numpy(t).cuda()


def torch_statements(logit, target, m_in, m_out, mce):
    """gqa_energy.py:122-138, :144-145 and loss.backward() down to the logits"""
    logit = logit.detach().requires_grad_(True)
    id_inds = target[:, -1] == 0
    target = target[:, :-1]
    if mce:
        _, tgt = target.max(1)
        loss = torch.nn.CrossEntropyLoss(ignore_index=-1)(logit, tgt) * logit.size(1)
        E_f = torch.logsumexp(logit, dim=1)
    else:
        loss = torch.nn.BCEWithLogitsLoss()(logit, target) * logit.size(1)
        E_f = torch.log(1 + torch.exp(logit)).sum(1)
    loss = loss + 0.1 * (torch.relu(-E_f[id_inds] - m_in) ** 2).mean() + 0.1 * (torch.relu(m_out + E_f[~id_inds]) ** 2).mean()
    loss.backward()
    _, label = torch.sigmoid(logit).max(1)
    return loss, logit.grad, E_f, label


def time_legs(legs, windows, iters, warm=3):
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(windows):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(iters):
                fn()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3 / iters)
    out = {}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    return out


def head_legs(B, mce):
    from rgqa_amd import _lib, scoring
    lib = _lib.load()
    z, t = draw(B)
    E = scoring.energy_loss_rows(z, t, weight=0.0, mce_loss=mce).energy
    idm = t[:, -1] == 0
    m_in, m_out = -float(E[idm].median()), -float(E[~idm].median())          # half of each subset's hinges active
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_energy_loss_scratch_floats(B, C.byref(n)))
    scratch, loss, dl = torch.empty(n.value, device="cuda"), torch.empty(3, device="cuda"), torch.empty(B, NA, device="cuda")
    en, lab = torch.empty(B, device="cuda"), torch.empty(B, dtype=torch.int64, device="cuda")
    p = _lib.ptr
    flag = C.c_void_p(t.data_ptr() + 4 * NA)

    def op():
        _lib.check(lib.rgqa_op_energy_loss(p(z), z.stride(0), p(t), t.stride(0), flag, t.stride(0), B, NA, NA, 1 if mce else 0, 0.1, m_in, m_out, 1.0, p(loss), p(dl),
                                           dl.stride(0), p(en), p(lab), p(scratch), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    legs = {"op": op, "rows": lambda: scoring.energy_loss_rows(z, t, m_in, m_out, 0.1, mce), "torch": lambda: torch_statements(z, t, m_in, m_out, mce)}
    # what is timed computes the same thing (measuring-on-mi355x §6)
    ref = torch_statements(z, t, m_in, m_out, mce)
    op()
    torch.cuda.synchronize()
    agree = dict(loss_rel=abs(float(loss[0]) - float(ref[0])) / abs(float(ref[0])), dlogits_rel_max=float((dl - ref[1]).abs().max() / ref[1].abs().max()),
                 energy_abs=float((en - ref[2]).abs().max()), labels_equal=bool(torch.equal(lab, ref[3])))
    return legs, {k: (round(v, 10) if isinstance(v, float) else v) for k, v in agree.items()}, (m_in, m_out)


def step_legs(B, precision, mce, margins):
    from rgqa_amd import synth
    from rgqa_amd.engine import Engine
    e = Engine(precision=precision, **FULL).allocate("cuda")
    init_params(e, seed=0)
    T, O = 20, 36
    b = synth.synth_batch(B, T, seed=1234)
    dev = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}
    lengths = np.ascontiguousarray(b["lengths"], dtype=np.int32)
    tuq = torch.zeros(B, NA + 1, device="cuda")
    tuq[:, :NA] = dev["target"]
    tuq[:, NA] = (dev["target"].sum(1) == 0).float()          # the batch's pseudo-UQ rows (all-zero targets) carry the flag
    e.ensure_shape(B, T, O)
    e.sync_weights()
    e.enable_segment_sumsq(True)
    state = dict(i=0)

    def step(energy):
        i = state["i"]
        e.forward(dev["feats"], dev["boxes"], dev["input_ids"], dev["input_mask"], dev["segment_ids"], train=True, seed=4321 + 1000003 * i, lengths=lengths)
        if energy:
            e.energy_loss_backward(tuq, margins[0], margins[1], 0.1, mce)
        else:
            e.loss_backward(dev["target"])
        e.adam_step(1e-5, max_norm=5.0)
        state["i"] = i + 1
    return {"step_bce": lambda: step(False), "step_energy": lambda: step(True)}, e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,64")
    ap.add_argument("--precision", default="bf16x3_fwd")
    ap.add_argument("--mce", action="store_true", help="the --mceLoss form (cross entropy, E = logsumexp)")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200, help="head legs: calls per window (a call is tens of microseconds)")
    ap.add_argument("--step-iters", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("energy_bench: needs an MI355X (no GPU found; there is no CPU path)")
    for B in (int(x) for x in a.batches.split(",")):
        legs, agree, margins = head_legs(B, a.mce)
        out = dict(batch=B, num_answers=NA, form="mce" if a.mce else "bce", windows=a.windows, iters=a.iters, agreement_with_torch=agree)
        out.update(time_legs(legs, a.windows, a.iters))
        if not a.skip_step:
            sl, e = step_legs(B, a.precision, a.mce, margins)
            out.update(precision=a.precision, step_iters=a.step_iters)
            out.update(time_legs(sl, a.windows, a.step_iters, warm=5))
            del e, sl
            torch.cuda.empty_cache()
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
