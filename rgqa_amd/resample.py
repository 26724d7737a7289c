"""The weight parameters of the reference's soft resampling of the hard unanswerable questions (tasks/gqa_resampling.py:139-140, :162-163, :183-186,
:203, :218-220) on the device, with the fused kernels of csrc/resample.hip:

    self.weight_params = nn.Parameter(torch.zeros(len(self.neg_tset)).cuda())                                  :139    ResampleWeights(n, lr_w)
    self.optim_w = torch.optim.SGD([self.weight_params], args.lr_w, momentum=0.9)                              :140
    w = F.softplus(self.weight_params).detach().cpu(); WeightedRandomSampler(w ** .5, ...)                     :162-163  sampler_weights
    w = F.softplus(self.weight_params); scale = (w ** .5).mean() / (w.mean() ** .5)                            :184-185  batch_weights
    weights = scale * (w[wids.cuda()] / w.mean()) ** .5                                                        :186
    loss_w = -loss_neg; self.optim_w.zero_grad(); loss_w.backward(); self.optim_w.step()                       :203, :218-220  step

The gradient of loss_w has a closed form (csrc/resample.hip): no autograd graph hangs on theta.  There is no CPU fallback: without the HIP library
batch_weights and step raise."""
import ctypes as C

import torch

from . import _lib


def _stream(dev):
    return C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


def check_wids(wids, n):
    """wids (a Python sequence or a CPU int64 tensor) as a contiguous CPU int64 tensor; ValueError for an empty list or an index outside [0, n)"""
    if isinstance(wids, torch.Tensor):
        if wids.dtype != torch.int64 or wids.dim() != 1 or wids.device.type != "cpu":
            raise ValueError("wids must be a Python sequence or a 1-D int64 tensor on the CPU (they originate on the host)")
        w = wids.contiguous()
    else:
        w = torch.tensor([int(i) for i in wids], dtype=torch.int64)
    if w.numel() == 0:
        raise ValueError("wids is empty")
    lo, hi = int(w.min()), int(w.max())
    if lo < 0 or hi >= n:
        raise ValueError("wids must lie in [0, %d); got %d .. %d" % (n, lo, hi))
    return w


class ResampleWeights:
    """theta [n] (zeros, as :139) and its SGD momentum buffer, both f32 on `device`.  Per train step: `batch_weights(wids)` before the loss,
    `step(row_loss)` after the model's optimizer step."""

    def __init__(self, n, lr_w, momentum=0.9, device="cuda"):
        n = int(n)
        if n < 1:
            raise ValueError("n must be positive")
        if not lr_w >= 0 or not 0 <= momentum < 1:
            raise ValueError("lr_w must not be negative and momentum must be in [0, 1)")
        self.n, self.lr_w, self.momentum = n, float(lr_w), float(momentum)
        self.device = torch.device(device)
        self.theta = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.momentum_buffer = torch.zeros(n, dtype=torch.float32, device=self.device)
        self.stats = None            # [2] f64 on the device: mean softplus(theta), mean sqrt softplus(theta) - of the theta of the last batch_weights
        self.wids = None             # the device copy of the last batch's indices
        self.weights = None
        self.row_loss = None         # what scoring.resample_finetune_loss leaves for step()
        self._scratch = None

    def _scratch_for(self, rows):
        n = C.c_size_t()
        _lib.check(_lib.load().rgqa_resample_scratch_floats(self.n, int(rows), C.byref(n)))
        if self._scratch is None or self._scratch.numel() < n.value:
            self._scratch = torch.empty(n.value, dtype=torch.float32, device=self.device)
        return self._scratch

    def batch_weights(self, wids):
        """:183-186 for the negative rows of one batch: [Bn] f32 weights (no graph attached).  Keeps the statistics and the indices for step()."""
        w = check_wids(wids, self.n)
        lib = _lib.load()
        scratch = self._scratch_for(w.numel())
        if self.stats is None:
            self.stats = torch.empty(2, dtype=torch.float64, device=self.device)
        self.wids = w.to(self.device)
        self.weights = torch.empty(w.numel(), dtype=torch.float32, device=self.device)
        self.row_loss = None
        p = _lib.ptr
        _lib.check(lib.rgqa_resample_weights(p(self.theta), self.n, p(self.wids), w.numel(), p(self.stats), p(self.weights), p(scratch), _stream(self.device)))
        return self.weights

    def step(self, row_loss=None, grad_out=None):
        """:203, :218-220: the gradient of -loss_neg with respect to theta and torch.optim.SGD's momentum update, for the indices of the last
        batch_weights.  row_loss [Bn] f32: the negative rows' BCE sums (default: what resample_finetune_loss left here).  grad_out: an [n] f32
        tensor that receives the gradient."""
        if self.wids is None:
            raise RuntimeError("ResampleWeights.step() before batch_weights(): there are no indices and no statistics")
        if row_loss is None:
            row_loss = self.row_loss
        if row_loss is None:
            raise RuntimeError("ResampleWeights.step(): no row_loss given and none left by resample_finetune_loss")
        r = row_loss
        if not isinstance(r, torch.Tensor) or r.dtype != torch.float32 or r.device != self.theta.device or r.dim() != 1:
            raise ValueError("row_loss must be a 1-D f32 tensor on %s" % self.theta.device)
        if r.numel() != self.wids.numel():
            raise ValueError("row_loss has %d entries, the last batch_weights had %d indices" % (r.numel(), self.wids.numel()))
        r = r.contiguous()
        if grad_out is not None and not (isinstance(grad_out, torch.Tensor) and grad_out.dtype == torch.float32 and grad_out.device == self.theta.device
                                         and tuple(grad_out.shape) == (self.n,) and grad_out.is_contiguous()):
            raise ValueError("grad_out must be a contiguous f32 [%d] tensor on %s" % (self.n, self.theta.device))
        lib = _lib.load()
        scratch = self._scratch_for(r.numel())
        p = _lib.ptr
        _lib.check(lib.rgqa_resample_step(p(self.theta), p(self.momentum_buffer), self.n, p(self.wids), p(r), r.numel(), p(self.stats), self.lr_w, self.momentum,
                                          p(grad_out), p(scratch), _stream(self.device)))
        self.wids = self.weights = self.row_loss = None        # the statistics belong to the theta before this update

    def sampler_weights(self):
        """:162-163: sqrt(softplus(theta)) on the CPU, for WeightedRandomSampler / torch.multinomial (once per epoch: plain torch)"""
        return torch.nn.functional.softplus(self.theta).sqrt().cpu()

    def state_dict(self):
        return dict(theta=self.theta.detach().cpu().clone(), momentum_buffer=self.momentum_buffer.detach().cpu().clone(), lr_w=self.lr_w, momentum=self.momentum)

    def load_state_dict(self, sd):
        th, mb = sd["theta"], sd["momentum_buffer"]
        if tuple(th.shape) != (self.n,) or tuple(mb.shape) != (self.n,):
            raise ValueError("state for %d weight parameters, this object holds %d" % (th.numel(), self.n))
        self.theta.copy_(th.to(torch.float32))
        self.momentum_buffer.copy_(mb.to(torch.float32))
        self.lr_w, self.momentum = float(sd.get("lr_w", self.lr_w)), float(sd.get("momentum", self.momentum))
        self.wids = self.weights = self.row_loss = None
