"""The energy fine-tuning loss head (tasks/gqa_energy.py:117-145; rgqa_amd/csrc/energy_loss.hip) without a GPU: the C ABI's declarations, the input
checks of the Python entry points, and the convention of the reference statements for an empty subset that the GPU tests rely on."""
import ctypes as C
import os
import re

import pytest
import torch

from tests.energy_reference import draw, evaluate, margins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ["rgqa_op_energy_loss", "rgqa_op_energy_loss_scratch_floats", "rgqa_engine_energy_loss_backward"]


def test_entry_points_are_declared_bound_and_exported():
    from rgqa_amd import _lib, scoring
    from rgqa_amd.engine import Engine
    hdr = open(os.path.join(ROOT, "include", "rgqa.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = dict(re.findall(r"\b(rgqa_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", hdr, flags=re.S))
    lib = _lib.load()
    for name in ENTRY_POINTS:
        assert name in protos and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert len(protos[name].split(",")) == len(_lib.SIGNATURES[name]), name
        assert protos[name].rstrip().endswith("void* stream") or name.endswith("_scratch_floats"), name     # stream argument last
    assert scoring.EnergyLoss._fields == ("loss", "base", "reg", "dlogits", "energy", "label")
    assert callable(scoring.energy_loss_rows) and callable(scoring.energy_finetune_loss) and callable(Engine.energy_loss_backward)
    n = C.c_size_t()
    _lib.check(lib.rgqa_op_energy_loss_scratch_floats(256, C.byref(n)))      # the query needs no device
    assert 0 < n.value <= 16 * 256
    assert lib.rgqa_op_energy_loss_scratch_floats(0, C.byref(n)) != 0


@pytest.mark.parametrize("fn", ["energy_finetune_loss", "energy_loss_rows"])
def test_python_entry_points_reject_bad_input(fn):
    """every check comes before the library is touched: CPU tensors, a target without the UQ column, a negative weight"""
    from rgqa_amd import scoring
    f = getattr(scoring, fn)
    z, t = torch.zeros(4, 9), torch.zeros(4, 10)
    with pytest.raises(ValueError):
        f(z, t, 25.0, 0.0)                                      # CPU tensors
    with pytest.raises(ValueError):
        f(z.double(), t, 25.0, 0.0)
    with pytest.raises(ValueError):
        f(z[0], t, 25.0, 0.0)
    meta = torch.device("meta")                                  # a non-CPU device that needs no hardware: is_cuda is False there as well
    with pytest.raises(ValueError):
        f(z.to(meta), t.to(meta), 25.0, 0.0)
    if torch.cuda.is_available():
        zg, tg = z.cuda(), t.cuda()
        with pytest.raises(ValueError):
            f(zg, tg[:, :9], 25.0, 0.0)                          # no UQ column
        with pytest.raises(ValueError):
            f(zg, t, 25.0, 0.0)                                  # target on another device
        with pytest.raises(ValueError):
            f(zg, tg, 25.0, 0.0, weight=-0.1)


def test_shape_and_weight_checks_do_not_depend_on_the_device_check():
    """the target-shape and weight checks themselves, on CPU tensors that pose as CUDA ones (no GPU here)"""
    from rgqa_amd import scoring

    class Fake(torch.Tensor):
        is_cuda = True

    z = torch.zeros(4, 9).as_subclass(Fake)
    t = torch.zeros(4, 10)
    for fn in (scoring.energy_finetune_loss, scoring.energy_loss_rows):
        with pytest.raises(ValueError, match="UQ column"):
            fn(z, t[:, :9], 25.0, 0.0)
        with pytest.raises(ValueError, match="UQ column"):
            fn(z, t.long(), 25.0, 0.0)
        with pytest.raises(ValueError, match="weight"):
            fn(z, t, 25.0, 0.0, weight=-1e-3)
        with pytest.raises(ValueError, match="weight"):
            fn(z, t, 25.0, 0.0, weight=float("nan"))


@pytest.mark.parametrize("mce", [False, True])
@pytest.mark.parametrize("ood", ["none", "all"])
def test_reference_statements_with_an_empty_subset(ood, mce):
    """gqa_energy.py:137-138 with no OOD row, or no ID row: the mean over no rows is NaN, so the loss is NaN; autograd still hands every logit a
    finite gradient - the base loss and the other subset's hinge.  (What the device operator reproduces: tests/test_gpu_energy_loss.py.)"""
    z, t = draw(4, 67, 11, ood=ood)
    m_in, m_out, _ = margins(z, t, mce)
    for dtype in (torch.float64, torch.float32):
        r = evaluate(z, t, m_in, m_out, mce, dtype)
        assert torch.isnan(r["loss"]) and torch.isnan(r["reg"]) and torch.isfinite(r["base"])
        assert torch.isfinite(r["dlogits"]).all() and float(r["dlogits"].abs().max()) > 0
        assert torch.isfinite(r["energy"]).all()
    # and the gradient is more than the base loss's: the non-empty subset's hinge is active in some row
    r1, r0 = evaluate(z, t, m_in, m_out, mce, torch.float64), evaluate(z, t, m_in, m_out, mce, torch.float64, weight=0.0)
    assert float((r1["dlogits"] - r0["dlogits"]).abs().max()) > 1e-6 * float(r0["dlogits"].abs().max())


def test_kernels_on_the_host(tmp_path):
    """csrc/energy_loss.hip built by the host compiler over tests/host_emu/kernels.h (each workgroup = 256 threads with barriers) and run against
    f64 loops of the reference statements (tests/host_emu/energy.cpp): BCE and MCE form, NA = 67 and 1842, aligned and shifted operands giving the
    same bits, guard words behind every output, exact zeros in the padded columns, grad_scale 0.5 halving exactly, both empty subsets, the argument
    checks.  (`./emu full` adds the larger shapes; a minute.)"""
    import subprocess
    from tests import host_emu
    host_emu.build(tmp_path, ["energy_loss"], "energy.cpp")
    r = subprocess.run(["./emu"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    print(r.stdout)
    assert r.returncode == 0 and "TOTAL bad 0" in r.stdout, r.stdout[-3000:] + r.stderr[-1000:]
