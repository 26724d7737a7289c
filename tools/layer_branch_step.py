"""Cost of the layer-wise confidence branch (rgqa_config.conf_branch = 2; reference tasks/gqa_branched_layer.py) against the pooled-vector branch (conf_branch = 1)
on the engine-direct train step - forward(train) + branched_loss_backward + adam_step - at the full 9/5/5 model, B = 256, T = 20, packed rows, bf16x3_fwd.

The two engines alternate in one process: after a warm-up, windows of `--iters` steps each, bracketed by device events on the launch stream, `--windows` windows
per engine (>= 100 steps each by default); the whole comparison runs `--rounds` times (2) so that the spread between rounds shows beside the difference.  Then one
profiled step of each engine (per-launch device events; the weight-gradient launches then run on the launch stream) is dumped through RGQA_PROF_DUMP and the
launches the layer-wise branch adds in the pooler / head / loss block are listed by kind and shape tag.

    timeout 900 python tools/layer_branch_step.py [--precision bf16x3_fwd] [--batch 256] [--project-size 128]

Prints one JSON line per round and one for the launch lists.  Not part of bench.py."""
import argparse
import collections
import json
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import FULL, init_params      # noqa: E402  (the flagship configuration and its random initialisation)

NA = FULL["num_answers"]
CATS = ("gemm_nt", "gemm_tn", "attn_fwd", "attn_bwd", "layernorm", "other", "gemm_nt_dgrad")
HEAD_BLOCK = 3                           # csrc/engine.h ProfBlock: pooler + head + loss


def build(B, precision, project_size):
    from rgqa_amd import synth
    from rgqa_amd.engine import Engine
    T, O = 20, 36
    b = synth.synth_batch(B, T, seed=1234)
    dev = {k: torch.from_numpy(v).cuda() for k, v in b.items() if k != "lengths"}
    lengths = np.ascontiguousarray(b["lengths"], dtype=np.int32)
    tuq = torch.zeros(B, NA + 1, device="cuda")
    tuq[:, :NA] = dev["target"]
    tuq[:, NA] = (dev["target"].sum(1) == 0).float()          # the batch's pseudo-UQ rows (all-zero targets) carry the flag
    engines = {}
    for name, cb in (("pooled", True), ("layer", "layer")):
        e = Engine(precision=precision, conf_branch=cb, project_size=project_size, **FULL).allocate("cuda")
        init_params(e, seed=0)
        e.ensure_shape(B, T, O)
        e.sync_weights()
        e.enable_segment_sumsq(True)
        engines[name] = e
    state = dict(i=0)

    def step(e):
        i = state["i"]
        state["i"] = i + 1
        e.forward(dev["feats"], dev["boxes"], dev["input_ids"], dev["input_mask"], dev["segment_ids"], train=True, seed=4321 + 1000003 * i, lengths=lengths)
        e.branched_loss_backward(tuq)
        e.adam_step(1e-5, max_norm=5.0)
    return engines, step


def one_round(engines, step, windows, iters):
    times = {k: [] for k in engines}
    for _ in range(windows):
        for k, e in engines.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                step(e)
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) / iters)
    out = {}
    for k, v in times.items():
        out[k + "_ms"] = round(float(np.median(v)), 4)
        out[k + "_ms_min_max"] = [round(float(min(v)), 4), round(float(max(v)), 4)]
    out["layer_minus_pooled_ms"] = round(out["layer_ms"] - out["pooled_ms"], 4)
    return out


def launch_list(e, step):
    """{(category, block, tag): [count, ms]} of one profiled step"""
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "prof.txt")
        os.environ["RGQA_PROF_DUMP"] = path
        try:
            e.profile(True)
            step(e)
            e.profile_read()
            e.profile(False)
        finally:
            del os.environ["RGQA_PROF_DUMP"]
        acc = collections.OrderedDict()
        for line in open(path):
            cat, blk, _, _, ms, tag = line.split()
            c = acc.setdefault((CATS[int(cat)], int(blk), tag), [0, 0.0])
            c[0] += 1
            c[1] += float(ms)
    return acc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--precision", default="bf16x3_fwd")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--project-size", type=int, default=128)
    ap.add_argument("--windows", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("layer_branch_step: needs an MI355X (no GPU found; there is no CPU path)")
    engines, step = build(a.batch, a.precision, a.project_size)
    for e in engines.values():
        for _ in range(a.warm):
            step(e)
    torch.cuda.synchronize()
    rounds = []
    for r in range(a.rounds):
        out = dict(round=r, batch=a.batch, precision=a.precision, project_size=a.project_size, steps_each=a.windows * a.iters)
        out.update(one_round(engines, step, a.windows, a.iters))
        rounds.append(out)
        print(json.dumps(out), flush=True)
    if len(rounds) > 1:
        d = [r["layer_minus_pooled_ms"] for r in rounds]
        spread = max(max(r[k + "_ms"] for r in rounds) - min(r[k + "_ms"] for r in rounds) for k in engines)
        print(json.dumps(dict(layer_minus_pooled_ms=d, spread_between_rounds_ms=round(spread, 4))), flush=True)
    lists = {k: launch_list(e, step) for k, e in engines.items()}
    total = {k: [sum(c for c, _ in v.values()), round(sum(m for _, m in v.values()), 4)] for k, v in lists.items()}
    head = {k: [sum(c for (_, blk, _), (c, _) in v.items() if blk == HEAD_BLOCK), round(sum(m for (_, blk, _), (_, m) in v.items() if blk == HEAD_BLOCK), 4)] for k, v in lists.items()}
    added, gone = [], []
    for key in list(lists["layer"]) + [k for k in lists["pooled"] if k not in lists["layer"]]:
        cl, cp = lists["layer"].get(key, [0, 0.0]), lists["pooled"].get(key, [0, 0.0])
        if cl[0] != cp[0]:
            (added if cl[0] > cp[0] else gone).append(dict(kind=key[0], block=key[1], tag=key[2], launches=cl[0] - cp[0], ms=round(cl[1] - cp[1], 4)))
    print(json.dumps(dict(profiled_step_launches_and_kernel_ms=total, head_block=head, added=added, gone=gone)), flush=True)


if __name__ == "__main__":
    main()
