"""The soft-resampling step (tasks/gqa_resampling.py:176-220; rgqa_amd/csrc/resample.hip) without a GPU: the C ABI's declarations, the input checks of
the Python entry points, the closed-form weight gradient against autograd of the reference statements, and the kernels on the host."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.resample_reference import closed_form_dtheta, draw, evaluate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rgqa_resample_scratch_floats", "rgqa_resample_weights", "rgqa_op_resample_loss", "rgqa_resample_step", "rgqa_engine_resample_loss_backward"]


def test_entry_points_are_declared_bound_and_exported():
    from rgqa_amd import _lib, resample, scoring
    from rgqa_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "rgqa.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(rgqa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name]), name
        assert protos[name].rstrip().endswith("void* stream") or name.endswith("_scratch_floats"), name     # stream argument last
    assert scoring.ResampleLoss._fields == ("loss", "loss_pos", "loss_neg", "dlogits", "row_loss")
    assert callable(scoring.resample_loss_rows) and callable(scoring.resample_finetune_loss) and callable(Engine.resample_loss_backward)
    assert isinstance(Engine.resample_loss_parts, property)
    for m in ("batch_weights", "step", "sampler_weights", "state_dict", "load_state_dict"):
        assert callable(getattr(resample.ResampleWeights, m))


def test_scratch_query_needs_no_device():
    from rgqa_amd import _lib
    lib = _lib.load()
    n = C.c_size_t()
    sizes = {}
    for N, B in ((1, 2), (37, 64), (100000, 64), (1000000, 256), (1 << 30, 512)):
        _lib.check(lib.rgqa_resample_scratch_floats(N, B, C.byref(n)))
        sizes[N, B] = n.value
        assert 2 * B + 4 <= n.value <= 4096 + 4 * B, (N, B, n.value)            # never N-sized
    assert sizes[1000000, 256] >= sizes[37, 64]
    assert lib.rgqa_resample_scratch_floats(0, 4, C.byref(n)) != 0
    assert lib.rgqa_resample_scratch_floats(4, 0, C.byref(n)) != 0


class _Fake(torch.Tensor):
    """a CPU tensor that poses as a CUDA one: reaches the checks behind the device check where there is no GPU"""
    is_cuda = True


class _NoLibraryWeights:
    """stands where a ResampleWeights would: a call means the argument checks let a bad input through"""
    def batch_weights(self, wids):
        raise AssertionError("batch_weights reached")

    def step(self, *a):
        raise AssertionError("step reached")


def _call(fn, z, t, n_pos, w):
    from rgqa_amd import scoring
    if fn == "resample_loss_rows":
        return scoring.resample_loss_rows(z, t, n_pos, w)
    return scoring.resample_finetune_loss(z, t, n_pos, _NoLibraryWeights(), [0] * (0 if w is None else w.numel()))


@pytest.mark.parametrize("fn", ["resample_finetune_loss", "resample_loss_rows"])
def test_python_entry_points_reject_bad_input(fn):
    """every check comes before the library is touched"""
    z, t, w = torch.zeros(4, 9), torch.zeros(4, 10), torch.ones(2)
    with pytest.raises(ValueError, match="CUDA"):
        _call(fn, z, t, 2, w)                                    # CPU logits
    with pytest.raises(ValueError, match="CUDA"):
        _call(fn, z.double().as_subclass(_Fake), t, 2, w)
    with pytest.raises(ValueError, match="CUDA"):
        _call(fn, z[0].as_subclass(_Fake), t, 2, w)
    meta = torch.device("meta")
    with pytest.raises(ValueError):
        _call(fn, z.to(meta), t.to(meta), 2, w.to(meta))
    zf = z.as_subclass(_Fake)
    with pytest.raises(ValueError, match="UQ column"):
        _call(fn, zf, t[:, :9], 2, w)                            # no UQ column
    with pytest.raises(ValueError, match="UQ column"):
        _call(fn, zf, t.long(), 2, w)
    for n_pos in (0, 4, 5, -1, 2.0, True):
        with pytest.raises(ValueError, match="n_pos"):
            _call(fn, zf, t, n_pos, w)
    if fn == "resample_loss_rows":
        for bad in (torch.ones(3), torch.ones(2).double(), torch.ones(2, 1), None, [1.0, 1.0]):
            with pytest.raises(ValueError, match="weights"):
                _call(fn, zf, t, 2, bad)
    else:
        from rgqa_amd import scoring
        with pytest.raises(ValueError, match="indices"):
            scoring.resample_finetune_loss(zf, t, 2, _NoLibraryWeights(), [0, 1, 2])
        with pytest.raises(ValueError, match="ResampleWeights"):
            scoring.resample_finetune_loss(zf, t, 2, object(), [0, 1])


def test_resample_weights_checks_come_before_the_library():
    from rgqa_amd.resample import ResampleWeights, check_wids
    for bad in ([0, 5], [-1, 2], [], torch.tensor([0, 5]), torch.tensor([1.0, 2.0]), torch.zeros(2, 2, dtype=torch.int64)):
        with pytest.raises(ValueError):
            check_wids(bad, 5)
    assert check_wids([4, 0, 4], 5).tolist() == [4, 0, 4] and check_wids(torch.tensor([3, 3]), 5).dtype == torch.int64
    with pytest.raises(ValueError):
        ResampleWeights(0, 1.0, device="cpu")
    with pytest.raises(ValueError):
        ResampleWeights(4, -1.0, device="cpu")
    rw = ResampleWeights(5, 100.0, device="cpu")                 # the state lives anywhere; the kernels need the device
    assert rw.theta.shape == (5,) and rw.theta.dtype == torch.float32 and float(rw.theta.abs().max()) == 0 and rw.momentum == 0.9
    with pytest.raises(ValueError):
        rw.batch_weights([0, 5])                                 # outside [0, n): before any library call
    with pytest.raises(RuntimeError, match="batch_weights"):
        rw.step(torch.ones(2))                                   # no batch_weights yet
    torch.testing.assert_close(rw.sampler_weights(), torch.full((5,), 2.0).log().sqrt())                        # sqrt(softplus(0)) = sqrt(log 2)
    sd = rw.state_dict()
    sd["theta"] = torch.arange(5.0)
    rw.load_state_dict(sd)
    assert rw.theta.tolist() == [0, 1, 2, 3, 4] and rw.lr_w == 100.0
    with pytest.raises(ValueError):
        rw.load_state_dict(dict(theta=torch.zeros(4), momentum_buffer=torch.zeros(4)))


@pytest.mark.parametrize("N,Bn", [(2, 3), (37, 7), (4099, 32), (4099, 1)])
def test_closed_form_gradient_is_autograd_of_the_statements(N, Bn):
    """d(-loss_neg)/d theta as the kernels form it (S, s_j, m1, mh; duplicates in wid; theta above softplus's threshold) against loss_w.backward() of the
    restated trainer statements, both in f64: 1e-12 of max |gradient|"""
    theta, wids, z, t = draw(N, 2, Bn, 67, 100 + N + Bn)
    if Bn >= 7:
        assert int(torch.bincount(wids).max()) >= 3
    r = evaluate(theta, wids, z, t, 2, torch.float64)
    g = closed_form_dtheta(theta.double(), wids, r["row_loss"])
    dev = float((g - r["dtheta"]).abs().max() / r["dtheta"].abs().max())
    print("N=%d Bn=%d: closed form against autograd %.2e" % (N, Bn, dev))
    assert dev <= 1e-12
    assert bool((r["dtheta"] != 0).all())                        # dense: every entry moves
    assert float(r["loss_w"]) == -float(r["loss_neg"])


def test_kernels_on_the_host(tmp_path):
    """csrc/resample.hip built by the host compiler over tests/host_emu/kernels.h (each workgroup = 256 threads with barriers) and run against
    f64 loops of the reference statements and of the closed-form weight step (tests/host_emu/resample.cpp): N = 2, 37 and 4099 (five chunks of
    theta, the last one partial), NA = 67 and 1842, duplicated indices, indices outside [0, N) skipped, aligned and shifted operands giving the same bits,
    guard words behind every output, exact zeros in the padded columns, grad_scale 0.5 halving exactly, the argument checks.  (`./emu full` adds
    more shapes.)"""
    import subprocess
    from tests import host_emu
    host_emu.build(tmp_path, ["resample"], "resample.cpp")
    r = subprocess.run(["./emu"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "TOTAL bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
