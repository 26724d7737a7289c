"""The host half of the Mahalanobis test method (tasks/gqa_maha.py:120-189; rgqa_amd/scoring.py): `maha_finalize` and `maha_pack` against the
reference's own estimator output stored in tests/golden/g13_maha.npz (tools/gen_g13_maha.py: sklearn's EmpiricalCovariance on the reference
modules' pooled rows), and the C ABI's declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BACKBONES = ["lxmert", "uniter"]
MAHA_ENTRY_POINTS = ["rgqa_maha_scratch_bytes", "rgqa_maha_score_rows", "rgqa_maha_dpooled", "rgqa_maha_state_doubles", "rgqa_maha_accumulate"]


@pytest.fixture(scope="module")
def g13():
    return np.load(os.path.join(ROOT, "tests", "golden", "g13_maha.npz"))


def accumulate_numpy(x, target):
    """the formulas of rgqa_maha_accumulate in numpy f64: n [NC], sums [NC, H], G [H, H]"""
    x = x.astype(np.float64)
    m = (target != 0).astype(np.float64)                  # sample b joins class c whenever target[b, c] != 0 (gqa_maha.py:158-168)
    k = m.sum(1)
    return m.sum(0), m.T @ x, (x * k[:, None]).T @ x


def score_f64(x, mean, precision):
    d = x.astype(np.float64)[:, None, :] - mean.astype(np.float64)[None, :, :]
    return -0.5 * np.einsum("bch,hk,bck->bc", d, precision.astype(np.float64), d)


@pytest.mark.parametrize("bb", BACKBONES)
def test_finalize_reproduces_the_reference_estimator(g13, bb):
    """mean within 1e-6, precision within 1e-5 max|P| of sklearn's (observed on three synthetic cases: 4e-9 .. 1e-7)"""
    from rgqa_amd import scoring, synth
    x, t = g13[bb + ".train_pooled"], g13[bb + ".train_target"]
    assert np.array_equal(t, synth.maha_case(bb, "train")["target"])
    n, sums, G = accumulate_numpy(x, t)
    assert all(n[c] == 0 for c in synth.MAHA_EMPTY) and ((t != 0).sum(1) > 1).mean() >= 0.10 and ((t != 0).sum(1) == 0).any()
    mean, precision, W = scoring.maha_finalize(n, sums, G)
    P = g13[bb + ".precision"]
    em, ep = np.abs(mean - g13[bb + ".mean"]).max(), np.abs(precision - P).max() / np.abs(P).max()
    print("maha finalize %s: mean err %.3e (bound 1e-6), precision err / max|P| %.3e (bound 1e-5), rank %d of %d" % (bb, em, ep, W.shape[1], W.shape[0]))
    assert em <= 1e-6 and ep <= 1e-5
    assert np.all(mean[list(synth.MAHA_EMPTY)] == 0.0)                       # classes without a sample keep the zero mean
    assert np.abs(W @ W.T - precision).max() <= 1e-12 * np.abs(precision).max()


@pytest.mark.parametrize("bb", BACKBONES)
def test_pack_factors_the_reference_pair(g13, bb):
    from rgqa_amd import scoring
    mean, P = g13[bb + ".mean"], g13[bb + ".precision"]
    W, Ps = scoring.maha_factor(P)
    assert W.dtype == np.float64 and W.shape[0] == P.shape[0] and 0 < W.shape[1] <= P.shape[0]
    e = np.abs(W @ W.T - P).max() / np.abs(P).max()
    print("maha_pack %s: |W W^T - P| / max|P| %.3e, rank %d" % (bb, e, W.shape[1]))
    assert e <= 1e-5
    nu = mean.astype(np.float64) @ W
    for key_x, key_s in ((".pooled", ".score_f64"), (".pooled2", ".score2_f64")):
        y = g13[bb + key_x].astype(np.float64) @ W
        s = -0.5 * ((y[:, None, :] - nu[None, :, :]) ** 2).sum(2)
        ref = g13[bb + key_s]
        np.testing.assert_allclose(ref, score_f64(g13[bb + key_x], mean, P), rtol=1e-12)         # the stored f64 evaluation is this formula
        print("maha_pack %s%s: factored f64 scores, max rel err %.3e" % (bb, key_x, (np.abs(s - ref) / np.abs(ref)).max()))
        np.testing.assert_allclose(s, ref, rtol=1e-9, atol=0)
    import torch
    pack = scoring.maha_pack(torch.from_numpy(mean), P, device="cpu")       # the pickle holds a tensor and an array (gqa_maha.py:185-188)
    assert isinstance(pack, scoring.MahaPack) and all(t.dtype == torch.float32 for t in pack)
    assert np.array_equal(pack.W.numpy(), W.astype(np.float32)) and np.array_equal(pack.nu.numpy(), nu.astype(np.float32))
    assert np.array_equal(pack.mean.numpy(), mean) and np.array_equal(pack.precision.numpy(), Ps.astype(np.float32))


def test_pack_and_finalize_reject_bad_input():
    from rgqa_amd import scoring
    with pytest.raises(ValueError):
        scoring.maha_pack(np.zeros((3, 4)), np.eye(5), device="cpu")
    with pytest.raises(ValueError):
        scoring.maha_factor(np.zeros((3, 4)))
    with pytest.raises(ValueError):
        scoring.maha_finalize(np.zeros(3), np.zeros((3, 4)), np.zeros((4, 4)))


def test_rank_deficient_covariance_takes_the_pinvh_cut():
    """rows confined to a subspace: the eigenvalues below max * H * eps are dropped (scipy pinvh's default cut), W has the subspace's rank"""
    from rgqa_amd import scoring
    rng = np.random.RandomState(3)
    H, r = 12, 7
    x = (rng.standard_normal((200, r)) @ rng.standard_normal((r, H))).astype(np.float32)
    t = np.zeros((200, 4), np.float32)
    t[np.arange(200), rng.randint(0, 3, 200)] = 1.0
    mean, precision, W = scoring.maha_finalize(*accumulate_numpy(x, t))
    assert W.shape == (H, r)
    xc = x.astype(np.float64) - mean[t.argmax(1)]
    cov = xc.T @ xc / 200
    np.testing.assert_allclose(precision, np.linalg.pinv(cov, rcond=H * np.finfo(np.float64).eps, hermitian=True), rtol=0, atol=1e-7 * np.abs(precision).max())


def test_maha_entry_points_are_declared_bound_and_exported():
    from rgqa_amd import _lib, scoring
    hdr = open(os.path.join(ROOT, "include", "rgqa.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(rgqa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    lib = _lib.load()
    for name in MAHA_ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name]), name
        assert protos[name].rstrip().endswith("void* stream") or name.endswith(("_bytes", "_doubles")), name     # stream argument last
    for name in ("MahaPack", "MahaEstimator", "maha_pack", "maha_sample_estimator", "maha_score_rows", "maha_dpooled", "maha_scores", "MahaScores"):
        assert hasattr(scoring, name), name
    assert scoring.MahaPack._fields == ("mean", "precision", "W", "nu")
    assert scoring.MahaScores._fields == ("score", "label", "pooled", "feats_pt", "boxes_pt")
    # the query functions need no device
    import ctypes as C
    n = C.c_size_t()
    _lib.check(lib.rgqa_maha_state_doubles(1842, 768, C.byref(n)))
    assert n.value == 1842 + 1842 * 768 + 768 * 768
    _lib.check(lib.rgqa_maha_scratch_bytes(256, 1842, C.byref(n)))
    assert n.value >= 256 * ((1842 + 15) // 16) * 8
    assert lib.rgqa_maha_scratch_bytes(0, 1842, C.byref(n)) != 0


def test_kernels_on_the_host(tmp_path):
    """csrc/maha.hip built by the host compiler over tests/host_emu/kernels.h (each workgroup = 256 threads with barriers) and run on small shapes
    against f64 loops (tests/host_emu/maha.cpp): both tile variants of the distance kernel, row strides, a duplicated class (first maximum), a NaN
    row, an overflowing class (-inf, never the winner), an invalid label, guard words behind scratch and state, counts exact, sums and G to 1e-12, two
    batches = the concatenated batch bit for bit."""
    import subprocess
    from tests import host_emu
    host_emu.build(tmp_path, ["maha"], "maha.cpp", headers=["include/rgqa.h"])
    r = subprocess.run(["./emu"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "TOTAL bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
