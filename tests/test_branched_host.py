"""The confidence-branch model, host side (no GPU): the restatement of the reference's model and trainer statements (tests/branched_reference.py) reproduces
the fixture of the reference's own GQAModel_branched (tests/golden/g15_branched.npz, tools/gen_g15_branched.py); the closed-form dlogits / dconf the kernel
computes equal f64 autograd of the statements; the engine's parameter table with and without the branch; and the loss and conf-tail kernels, compiled for the
host under a workgroup emulation as a stand-alone program (tests/host_emu/), against the same statements."""
import os
import subprocess

import numpy as np
import pytest
import torch

from rgqa_amd import synth
from tests import branched_reference as BR
from tests import host_emu


def _oracle_small(dtype):
    from oracle import lxmert_ref as R
    cfg = R.RefConfig(**synth.SMALL)
    shapes = dict(R.param_shapes(cfg))
    H = synth.SMALL["hidden"]
    shapes.update(zip(BR.CONF_KEYS, [(2 * H, H), (2 * H,), (2 * H,), (2 * H,), (1, 2 * H), (1,)]))
    P = {k: torch.from_numpy(synth.fill_value(k, tuple(s))).to(dtype).requires_grad_(True) for k, s in shapes.items()}
    b = {k: torch.from_numpy(v) for k, v in synth.small_batch(8).items() if k != "lengths"}
    lg, pl = R.gqa_forward({k: v for k, v in P.items() if not k.startswith("conf_fc.")}, cfg, b["feats"].to(dtype), b["boxes"].to(dtype), b["input_ids"],
                           b["input_mask"], b["segment_ids"])
    return P, lg, pl


@pytest.mark.parametrize("form", ["bce", "mce"])
def test_restatement_reproduces_the_fixture(golden_dir, form):
    g = np.load(os.path.join(golden_dir, "g15_branched.npz"))
    P, lg, pl = _oracle_small(torch.float64)
    cf = BR.conf_head(pl, P)
    np.testing.assert_allclose(lg.detach().numpy(), g["logits"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(pl.detach().numpy(), g["pooled"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(cf.detach().numpy(), g["conf"], rtol=0, atol=2e-5)
    t = torch.from_numpy(g["target_with_uq"]).double()
    assert np.array_equal(g["target_with_uq"], synth.branched_target()) and t[1, -1] == 1 and t[0, -1] == 0 and t[2, -1] == 0
    loss, ce, cfl, _, _ = BR.trainer_statements(lg, cf, t, form == "mce")
    for k, v in (("loss", loss), ("loss_ce", ce), ("loss_conf", cfl)):
        np.testing.assert_allclose(float(v.detach()), g[form + "." + k], rtol=2e-6, err_msg=k)
    loss.backward()
    dead = set(g["dead"].tolist())
    for k, p in P.items():
        if k in dead:
            assert p.grad is None or float(p.grad.abs().max()) == 0
            continue
        ref = g["%s.grad.%s" % (form, k)]
        got = p.grad.numpy()
        idx = BR.fixture_index(form, k, got.size)
        if idx is not None:
            got = got.reshape(-1)[idx]
        np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-7 + 2e-5 * np.abs(ref).max(), err_msg=k)


@pytest.mark.parametrize("uq", ["third", "all"])
@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA", [(5, 67), (32, 300)])
def test_closed_form_gradients_equal_f64_autograd(B, NA, mce, uq):
    z, c, t = BR.draw(B, NA, 77 + B + NA, uq=uq)
    r = BR.evaluate(z, c, t, mce, torch.float64)
    dz, dc = BR.closed_form(z, c, t, mce)
    np.testing.assert_allclose(dz.numpy(), r["dlogits"].numpy(), rtol=1e-10, atol=1e-15)
    np.testing.assert_allclose(dc.numpy(), r["dconf"].numpy(), rtol=1e-10, atol=1e-15)
    assert bool((dz[t[:, -1] != 0] == 0).all())
    if uq == "all":
        assert torch.isnan(r["loss_ce"]) and torch.isfinite(r["dconf"]).all()


def test_parameter_table_with_and_without_the_branch():
    from rgqa_amd.engine import Engine
    ep, e0, eb = Engine(precision="bf16", **synth.SMALL), Engine(precision="bf16", conf_branch=False, **synth.SMALL), Engine(precision="bf16", conf_branch=True, **synth.SMALL)
    key = lambda e: [(sp.name, sp.offset, sp.shape, sp.linear, sp.dead, sp.f32_read) for sp in e.specs]
    assert key(e0) == key(ep) and e0.arena_elems == ep.arena_elems
    assert key(eb)[:len(ep.specs)] == key(ep) and [sp.name for sp in eb.specs[len(ep.specs):]] == list(BR.CONF_KEYS)
    assert ep.specs[-1].name == "logit_fc.3.bias" and eb.arena_elems > ep.arena_elems
    with pytest.raises(RuntimeError, match="conf"):
        Engine(precision="bf16", conf_branch=True, arch=2, **synth.U_SMALL)


# ------------------------------------------------------------------------------------------------ the kernels under a host workgroup emulation
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """the two units built by the host compiler over tests/host_emu/kernels.h as a stand-alone program, with the host sanitizers where the
    toolchain has their runtimes"""
    return host_emu.build(tmp_path_factory.mktemp("branched_emu"), ["branched_loss", "conf_head"], "branched.cpp")


def _run_emu(exe, tmp_path, z, c, t, mce, NAp, w=None, x=None, dg=None, dconf=None):
    """inputs as raw little-endian f32 files -> outputs read back the same way"""
    names = dict(z=z, c=c, t=t)
    if w is not None:
        names.update(x=x, dg=dg, dconf=dconf, gamma=w[0], beta=w[1], w3=w[2], b3=w[3])
    for k, v in names.items():
        np.ascontiguousarray(v, dtype=np.float32).tofile(str(tmp_path / (k + ".bin")))
    B, NA = z.shape
    N = 0 if w is None else x.shape[1]
    r = subprocess.run([exe, str(tmp_path), str(B), str(NA), str(NAp), str(1 if mce else 0), str(N)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TOTAL bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    rd = lambda k, dt=np.float32: np.fromfile(str(tmp_path / (k + ".out")), dtype=dt)
    out = dict(loss=rd("loss"), dl=rd("dl").reshape(B, NAp), dconf=rd("dconf_out"), conf=rd("conf"), score1=rd("score1"), label=rd("label", np.int64))
    if w is not None:
        out.update(cl=rd("cl"), gc=rd("gc").reshape(B, N), dgamma=rd("dgamma"), dbeta=rd("dbeta"), dw3=rd("dw3"), db3=rd("db3"))
    return out


@pytest.mark.parametrize("mce", [False, True], ids=["bce", "mce"])
@pytest.mark.parametrize("B,NA,uq", [(5, 67, "third"), (7, 300, "third"), (4, 67, "all")])
def test_loss_kernel_under_the_host_emulation(emu, tmp_path, B, NA, mce, uq):
    z, c, t = BR.draw(B, NA, 500 + B + NA, uq=uq)
    NAp = (NA + 63) // 64 * 64
    o = _run_emu(emu, tmp_path, z.numpy(), c.numpy(), t.numpy(), mce, NAp)
    r = BR.evaluate(z, c, t, mce, torch.float64)
    np.testing.assert_allclose(o["dl"][:, :NA], r["dlogits"].numpy(), rtol=0, atol=2e-6 * max(float(r["dlogits"].abs().max()), 1e-30))
    assert not o["dl"][:, NA:].any() and not np.signbit(o["dl"][:, NA:]).any() and not o["dl"][(t[:, -1] != 0).numpy()].any()
    np.testing.assert_allclose(o["dconf"], r["dconf"].numpy(), rtol=0, atol=2e-6 * float(r["dconf"].abs().max()))
    np.testing.assert_allclose(o["conf"], r["conf"].numpy(), rtol=0, atol=2e-7)
    np.testing.assert_allclose(o["score1"], r["score1"].numpy(), rtol=0, atol=2e-7)
    assert np.array_equal(o["label"], z.max(1)[1].numpy())
    np.testing.assert_allclose(o["loss"][2], float(r["loss_conf"]), rtol=1e-6)
    if uq == "all":
        assert np.isnan(o["loss"][0]) and np.isnan(o["loss"][1])
    else:
        np.testing.assert_allclose(o["loss"][:2], [float(r["loss"]), float(r["loss_ce"])], rtol=2e-6)


@pytest.mark.parametrize("B,N", [(3, 128), (6, 1536)])      # (a workgroup costs 256 host threads: the row counts stay small; B = 70 and 300 run on the GPU)
def test_conf_tail_kernels_under_the_host_emulation(emu, tmp_path, B, N):
    """forward conf logit, the gradient entering conf_fc.0's output and the four column sums against f64 autograd of LayerNorm + the 2H -> 1 projection"""
    x = synth.uniform("emu.x%d" % N, (B, N), -1.0, 2.0)
    dg = synth.uniform("emu.dg%d" % N, (B, N), -0.2, 1.1)
    dconf = synth.uniform("emu.dc%d" % N, (B,), -1.0, 1.0)
    w = (1.0 + synth.uniform("emu.g", (N,), -0.1, 0.1), synth.uniform("emu.b", (N,), -0.1, 0.1), synth.uniform("emu.w3", (N,), -0.05, 0.05), synth.uniform("emu.b3", (1,), -0.05, 0.05))
    z, c, t = BR.draw(B, 67, 9)
    o = _run_emu(emu, tmp_path, z.numpy(), c.numpy(), t.numpy(), False, 128, w=w, x=x, dg=dg, dconf=dconf)
    X = torch.from_numpy(x).double().requires_grad_(True)
    G, Bt, W3, B3 = (torch.from_numpy(v).double().requires_grad_(True) for v in w)
    cl = torch.nn.functional.layer_norm(X, (N,), G, Bt, 1e-12) @ W3 + B3
    (cl * torch.from_numpy(dconf).double()).sum().backward()
    np.testing.assert_allclose(o["cl"], cl.detach().numpy(), rtol=0, atol=1e-5)
    gc = (X.grad * torch.from_numpy(dg).double()).numpy()
    for k, ref in (("gc", gc), ("dgamma", G.grad.numpy()), ("dbeta", Bt.grad.numpy()), ("dw3", W3.grad.numpy()), ("db3", B3.grad.numpy())):
        np.testing.assert_allclose(o[k], ref, rtol=0, atol=1e-5 * np.abs(ref).max(), err_msg=k)
