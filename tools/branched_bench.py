"""Time of the engine-direct LXMERT train step with the confidence branch (rgqa_config.conf_branch; reference tasks/gqa_branched.py:126-145) at the full 9/5/5
model, B = 256, T = 20, packed rows.  Legs alternate in one process after a warm-up, each window bracketed by device synchronisation:

    plain      Engine: forward(train) + loss_backward + adam_step - bench.py's step
    branched   Engine(conf_branch=True): forward(train) + branched_loss_backward + adam_step - ONE encoder backward, conf_fc in the arena
    conf_only  the same engine with branched_loss_backward(conf_only=True) (--freeze_vqa_branch): no answer-head or encoder backward
    torch_head what a user had before: the plain engine + a torch conf_fc on the pooled output - forward(train), the branched trainer's statements under
               torch autograd on (logits, pooled), backward(dlogits) + backward_pooled(dpooled, accumulate=True) (two encoder backward passes), adam_step on
               the arena and torch.optim.Adam on the foreign conf_fc

    timeout 900 python tools/branched_bench.py [--precisions bf16x3_fwd,bf16] [--batch 256]

Prints one JSON line per precision: median ms of each leg over the windows, with min / max.  Not part of bench.py."""
import argparse
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


def time_legs(legs, windows, iters, warm=5):
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


def legs_for(B, precision):
    from rgqa_amd import synth
    from rgqa_amd.engine import Engine
    from rgqa_amd.lxrt.modeling import GeLU
    T, O, H = 20, 36, FULL["hidden"]
    b = synth.synth_batch(B, T, seed=1234)
    dev = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}
    lengths = np.ascontiguousarray(b["lengths"], dtype=np.int32)
    tuq = torch.zeros(B, NA + 1, device="cuda")
    tuq[:, :NA] = dev["target"]
    tuq[:, NA] = (dev["target"].sum(1) == 0).float()          # the batch's pseudo-UQ rows (all-zero targets) carry the flag
    engines = {}
    for name, cb in (("plain", False), ("branched", True)):
        e = Engine(precision=precision, conf_branch=cb, **FULL).allocate("cuda")
        init_params(e, seed=0)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        e.enable_segment_sumsq(True)
        engines[name] = e
    conf_fc = torch.nn.Sequential(torch.nn.Linear(H, 2 * H), GeLU(), torch.nn.LayerNorm(2 * H, eps=1e-12), torch.nn.Linear(2 * H, 1)).cuda()
    opt = torch.optim.Adam(conf_fc.parameters(), lr=1e-5)
    state = dict(i=0)

    def fwd(e):
        i = state["i"]
        state["i"] = i + 1
        return e.forward(dev["feats"], dev["boxes"], dev["input_ids"], dev["input_mask"], dev["segment_ids"], train=True, seed=4321 + 1000003 * i, lengths=lengths)

    def plain():
        e = engines["plain"]
        fwd(e)
        e.loss_backward(dev["target"])
        e.adam_step(1e-5, max_norm=5.0)

    def branched(conf_only=False):
        e = engines["branched"]
        fwd(e)
        e.branched_loss_backward(tuq, conf_only=conf_only)
        e.adam_step(1e-5, max_norm=5.0)

    def torch_head():
        e = engines["plain"]
        lg, pl = fwd(e)
        logit, pooled = lg.detach().requires_grad_(True), pl.detach().requires_grad_(True)
        opt.zero_grad()
        id_inds = tuq[:, -1] == 0
        loss_ce = torch.nn.functional.binary_cross_entropy_with_logits(logit[id_inds], tuq[:, :-1][id_inds]) * NA
        loss_conf = torch.nn.functional.binary_cross_entropy(torch.sigmoid(conf_fc(pooled)).squeeze(), id_inds.float())
        (loss_ce + loss_conf).backward()
        e.backward(logit.grad)
        e.backward_pooled(pooled.grad, accumulate=True)
        e.adam_step(1e-5, max_norm=5.0)
        opt.step()
    return {"plain": plain, "branched": branched, "conf_only": lambda: branched(True), "torch_head": torch_head}, engines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precisions", default="bf16x3_fwd,bf16")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("branched_bench: needs an MI355X (no GPU found; there is no CPU path)")
    for prec in a.precisions.split(","):
        legs, engines = legs_for(a.batch, prec)
        out = dict(batch=a.batch, precision=prec, windows=a.windows, iters=a.iters)
        out.update(time_legs(legs, a.windows, a.iters))
        out["branched_minus_plain_ms"] = round(out["branched_ms"] - out["plain_ms"], 4)
        out["torch_head_minus_branched_ms"] = round(out["torch_head_ms"] - out["branched_ms"], 4)
        print(json.dumps(out), flush=True)
        del legs, engines
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
