"""The layer-wise confidence-branch model, host side (no GPU): the restatement of the reference's model (tests/layer_branched_reference.py) reproduces the
fixture of the reference's own class (tests/golden/g16_branched_layer.npz, tools/gen_g16_branched_layer.py); the two conditions that keep the fixture from
being blind, re-checked from the file; the engine's parameter table with conf_branch 0, 1 and 2; and the tap gather / inject kernels and the conf tail at row
widths that are not 2 * hidden, compiled for the host under the workgroup emulation as a stand-alone program (tests/host_emu/), against numpy."""
import os
import subprocess

import numpy as np
import pytest
import torch

from rgqa_amd import synth
from tests import branched_reference as BR
from tests import host_emu
from tests import layer_branched_reference as LR

CFG, P = synth.LAYER_SMALL, synth.LAYER_PROJECT_SIZE


@pytest.fixture(scope="module")
def g16(golden_dir):
    return np.load(os.path.join(golden_dir, "g16_branched_layer.npz"))


@pytest.fixture(scope="module")
def restated():
    """ONE f64 forward of the restatement, shared (and left unchanged) by the tests below"""
    W = LR.weights(CFG, P, torch.float64)
    b = {k: torch.from_numpy(v) for k, v in synth.small_batch(8).items() if k != "lengths"}
    return W, LR.forward(W, CFG, b)


@pytest.mark.parametrize("form", ["bce", "mce", "noconf"])
def test_restatement_reproduces_the_fixture(g16, restated, form):
    g = g16
    W, (lg, cf, pc, pl) = restated
    for got, k in ((lg, "logits"), (cf, "conf"), (pc, "projcat"), (pl, "pooled")):
        np.testing.assert_allclose(got.detach().numpy(), g[k], rtol=0, atol=2e-5, err_msg=k)
    assert g["projcat"].shape == (3, CFG["x_layers"] * P) and g["conf"].shape == (3, 1)
    t = torch.from_numpy(g["target_with_uq"]).double()
    assert np.array_equal(g["target_with_uq"], synth.branched_target())
    loss, ce, cfl, _, _ = LR.trainer_statements(lg, cf, t, form == "mce")
    if form != "noconf":
        for k, v in (("loss", loss), ("loss_ce", ce), ("loss_conf", cfl)):
            np.testing.assert_allclose(float(v.detach()), g[form + "." + k], rtol=2e-6, err_msg=k)
    keys = [k for k in W]
    grads = dict(zip(keys, torch.autograd.grad(ce if form == "noconf" else loss, [W[k] for k in keys], retain_graph=True, allow_unused=True)))
    dead = set(g["dead"].tolist())
    assert dead and all(".x_layers.%d.visn_" % (CFG["x_layers"] - 1) in k for k in dead)
    for k in keys:
        if k in dead or (form == "noconf" and LR.is_branch(k)):
            assert grads[k] is None or float(grads[k].abs().max()) == 0, k
            assert "%s.grad.%s" % (form, k) not in g.files
            continue
        ref = g["%s.grad.%s" % (form, k)]
        got = grads[k].numpy()
        idx = LR.fixture_index("bce" if form == "noconf" else form, k, got.size)
        if idx is not None:
            got = got.reshape(-1)[idx]
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-7 + 2e-5 * np.abs(ref).max(), err_msg=k)


def test_fixture_is_not_blind(g16):
    """(a) no tanh is saturated; (b) on one stored tensor of every group of layers the full gradient and the answer loss's alone differ by at least 50 times the
    f32 gate of the GPU tests: a gradient injection missing at any tap fails the fixture tests"""
    assert float(np.abs(g16["projcat"]).max()) < 0.95
    reach, ok = LR.branch_reach(g16)
    assert ok and set(reach) == set(LR.GROUPS), reach
    keys = g16["keys"].tolist()
    assert [k for k in keys if LR.is_branch(k)] == list(LR.branch_keys(CFG["x_layers"])) and len(keys) == len(LR.param_shapes(CFG, P))


def test_parameter_table_with_conf_branch_0_1_2():
    from rgqa_amd.engine import Engine
    ep, e0, e1 = Engine(precision="bf16", **CFG), Engine(precision="bf16", conf_branch=False, **CFG), Engine(precision="bf16", conf_branch=True, **CFG)
    e2 = Engine(precision="bf16", conf_branch="layer", project_size=P, **CFG)
    key = lambda e: [(sp.name, sp.offset, sp.shape, sp.linear, sp.dead, sp.f32_read) for sp in e.specs]
    H, X = CFG["hidden"], CFG["x_layers"]
    # 0 and 1: what they were (project_size is not read)
    assert key(e0) == key(ep) and e0.arena_elems == ep.arena_elems and ep.specs[-1].name == "logit_fc.3.bias"
    assert key(Engine(precision="bf16", conf_branch=True, project_size=8, **CFG)) == key(e1)
    assert key(e1)[:len(ep.specs)] == key(ep) and [sp.name for sp in e1.specs[len(ep.specs):]] == list(BR.CONF_KEYS)
    assert [sp.shape for sp in e1.specs[len(ep.specs):]] == [(2 * H, H), (2 * H,), (2 * H,), (2 * H,), (1, 2 * H), (1,)]
    # 2: the projectors, then conf_fc, behind logit_fc.3
    new = e2.specs[len(ep.specs):]
    shapes = LR.branch_shapes(H, X, P)
    assert key(e2)[:len(ep.specs)] == key(ep)
    assert [sp.name for sp in new] == list(LR.branch_keys(X)) and all(sp.shape == shapes[sp.name] for sp in new)
    assert [sp.name for sp in new if sp.linear and sp.f32_read] == ["conf_fc.3.weight"] and not any(sp.dead for sp in new)
    assert [sp.name for sp in new if sp.linear] == [k for k in LR.branch_keys(X) if k.endswith(".weight") and not k.startswith("conf_fc.2.")]
    # ... covering the arena with no gap: every tensor starts where the slot of the one in front of it ends (slots are 64-element aligned; a linear weight's
    # slot also holds its transposed copy's padding: in_features * round_up(out_features, 64))
    up = lambda n: (n + 63) // 64 * 64
    end = up(ep.arena_elems)
    assert new[0].offset == end
    for sp in new:
        assert sp.offset == end, sp.name
        n = sp.numel
        if sp.linear and sp.name != "conf_fc.3.weight":
            n = max(n, sp.shape[1] * up(sp.shape[0]))
        if sp.name.endswith(".bias"):
            n = up(n)
        end = up(sp.offset + n)
    assert end == e2.arena_elems
    segs = e2.grad_segments()
    assert segs[0][1] == e2.arena_elems and segs[0][0] < new[0].offset      # the head + pooler segment holds the branch: clip, BertAdam and the exchange cover it
    # what engine_create refuses
    for kw, msg in ((dict(project_size=12), "project_size"), (dict(project_size=0), "project_size"), (dict(project_size=512), "2048"),
                    (dict(project_size=16, precision="bf16x3"), "project_size"), (dict(project_size=16, x_layers=0), "cross-modality")):
        args = dict(CFG, precision="bf16", conf_branch="layer")
        args.update(kw)
        if args["precision"] == "bf16x3":
            args.update(heads=1)           # head size 64, as the split-f32 precisions need
        with pytest.raises(RuntimeError, match=msg):
            Engine(**args)
    with pytest.raises(RuntimeError, match="conf"):
        Engine(precision="bf16", conf_branch="layer", arch=2, **synth.U_SMALL)
    Engine(precision="bf16x3_fwd", conf_branch="layer", project_size=32, **dict(CFG, heads=1))
    with pytest.raises(RuntimeError, match="layer-wise"):
        e1.layer_proj
    # the C ABI's own value names the layer-wise branch too; anything else is refused instead of read as a boolean
    assert key(Engine(precision="bf16", conf_branch=2, project_size=P, **CFG)) == key(e2) and key(Engine(precision="bf16", conf_branch=1, **CFG)) == key(e1)
    for bad in (3, "layers", "pooled"):
        with pytest.raises(ValueError, match="conf_branch"):
            Engine(precision="bf16", conf_branch=bad, **CFG)


# ------------------------------------------------------------------------------------------------ the kernels under a host workgroup emulation
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """csrc/layer_taps.hip and csrc/conf_head.hip built by the host compiler over tests/host_emu/kernels.h as a stand-alone program, with the host sanitizers
    where the toolchain has their runtimes"""
    return host_emu.build(tmp_path_factory.mktemp("layer_branched_emu"), ["layer_taps", "conf_head"], "layer_branched.cpp", headers=("rgqa_amd/csrc/layer_taps.h",))


def _run(exe, tmp_path, args, files):
    for k, v in files.items():
        np.ascontiguousarray(v).tofile(str(tmp_path / (k + ".bin")))
    r = subprocess.run([exe, str(tmp_path)] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TOTAL bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    return lambda k, dt=np.float32: np.fromfile(str(tmp_path / (k + ".out")), dtype=dt)


@pytest.mark.parametrize("tail", [1, 0], ids=["cls_tail", "all_rows"])
@pytest.mark.parametrize("varlen", [0, 1], ids=["padded", "cu"])
@pytest.mark.parametrize("B", [3, 70])
def test_tap_gather_and_inject_under_the_host_emulation(emu, tmp_path, B, varlen, tail):
    """every layer's [CLS] rows out of the padded / packed rows (the last layer's out of its B compact rows under the [CLS]-tail) bit for bit, the bf16 image
    of the same rows read as split-f32 lines, and the tap gradients added to exactly those rows"""
    T, X, H = 5, 3, 64
    lens = 1 + (synth.hash_u32("emu.lens%d" % B, B) % np.uint64(T)).astype(np.int32)
    lens[0], lens[-1] = 1, T
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = int(cu[-1]) if varlen else B * T
    first = cu[:-1] if varlen else np.arange(B) * T
    files, src, dy = dict(lens=lens), [], []
    for i in range(X):
        n = B if (tail and i == X - 1) else rows
        src.append(synth.uniform("emu.src%d.%d" % (i, B), (n, H), -2.0, 2.0))
        dy.append(synth.uniform("emu.dy%d.%d" % (i, B), (n, H), -1.0, 1.0))
        files["src%d" % i], files["dy%d" % i] = src[i], dy[i]
    dtap = synth.uniform("emu.dtap%d" % B, (X, B, H), -1.0, 1.0)
    files["dtap"] = dtap
    rd = _run(emu, tmp_path, ["taps", B, T, X, H, varlen, tail], files)
    taps = rd("taps").reshape(X, B, H)
    for i in range(X):
        r = np.arange(B) if (tail and i == X - 1) else first
        assert np.array_equal(taps[i], src[i][r]), i
        want = dy[i].copy()
        want[r] += dtap[i]
        assert np.array_equal(rd("dy%d" % i).reshape(want.shape), want), i        # one f32 addition per element: the same bits; every other row untouched
    img = rd("img", np.uint8).reshape(X * B, H * 2)
    lines = taps.reshape(X * B, H).view(np.uint8).reshape(X * B, -1, 128)[:, :, :64]      # the hi half of every 128-byte line
    assert np.array_equal(img, lines.reshape(X * B, -1))


@pytest.mark.parametrize("B,N", [(3, 96), (5, 1280)])      # 2 * x_layers * project_size at the fixture's and the reference's sizes; neither is 2 * hidden
def test_conf_tail_at_layer_widths_under_the_host_emulation(emu, tmp_path, B, N):
    x = synth.uniform("emu.lx%d" % N, (B, N), -1.0, 2.0)
    dg = synth.uniform("emu.ldg%d" % N, (B, N), -0.2, 1.1)
    dconf = synth.uniform("emu.ldc%d" % N, (B,), -1.0, 1.0)
    w = (1.0 + synth.uniform("emu.lg", (N,), -0.1, 0.1), synth.uniform("emu.lb", (N,), -0.1, 0.1), synth.uniform("emu.lw3", (N,), -0.05, 0.05), synth.uniform("emu.lb3", (1,), -0.05, 0.05))
    rd = _run(emu, tmp_path, ["tail", B, N], dict(x=x, dg=dg, dconf=dconf, gamma=w[0], beta=w[1], w3=w[2], b3=w[3]))
    X = torch.from_numpy(x).double().requires_grad_(True)
    G, Bt, W3, B3 = (torch.from_numpy(v).double().requires_grad_(True) for v in w)
    cl = torch.nn.functional.layer_norm(X, (N,), G, Bt, 1e-12) @ W3 + B3
    (cl * torch.from_numpy(dconf).double()).sum().backward()
    np.testing.assert_allclose(rd("cl"), cl.detach().numpy(), rtol=0, atol=1e-5)
    gc = (X.grad * torch.from_numpy(dg).double()).numpy()
    for k, ref in (("gc", gc), ("dgamma", G.grad.numpy()), ("dbeta", Bt.grad.numpy()), ("dw3", W3.grad.numpy()), ("db3", B3.grad.numpy())):
        np.testing.assert_allclose(rd(k).reshape(ref.shape), ref, rtol=0, atol=1e-5 * np.abs(ref).max(), err_msg=k)
