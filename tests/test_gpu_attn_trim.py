"""Per-sample tile counts of the MFMA attention kernels (rgqa_debug_set key 23; attn_core.h and its units attn_mfma.hip, attn_x3.hip, kernels.h ATTN_RUN_TRIMMED).

With packed rows a wave whose sample fills one 16-row tile fewer than its launch's tile counts runs the body of the smaller count.  What it
leaves out only ever held masked keys (probabilities exactly 0) and query rows that are never stored, so every result must be BIT-identical
to the untrimmed run (key 23 = 0), at the engine level (logits and the whole gradient arena, train mode with dropout) and at the operator
level, where the kernels are also held to the reference kernels of attn.hip with the tolerances of tests/test_gpu_ops.py."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from rgqa_amd import synth                                                      # noqa: E402

MED = dict(vocab_size=512, hidden=128, heads=2, inter=256, max_pos=64, type_vocab=2, l_layers=2, x_layers=2, r_layers=1,
           feat_dim=64, pos_dim=4, num_answers=70)


@pytest.fixture(scope="module")
def lib():
    from rgqa_amd import _lib
    return _lib.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def ck(rc):
    from rgqa_amd._lib import check
    check(rc)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def make_engine(cfgd, precision, dropout):
    from rgqa_amd.engine import Engine
    e = Engine(precision=precision, hidden_dropout=dropout, attn_dropout=dropout, **cfgd).allocate("cuda")
    for sp in e.specs:
        e.view(e.params, sp).copy_(torch.from_numpy(synth.fill_value(sp.name, sp.shape)))
    return e


def batch_with_lengths(T, lens, cfgd):
    """synthetic batch whose questions have exactly the given token counts ([CLS] ... [SEP], zero padding)"""
    raw = synth.synth_batch(len(lens), T, O=36, F=cfgd["feat_dim"], NA=cfgd["num_answers"], vocab=cfgd["vocab_size"], seed=77, min_len=T)
    ids = raw["input_ids"]
    assert (ids != 0).all()
    for b, n in enumerate(lens):
        sep = ids[b, T - 1]
        ids[b, n:] = 0
        ids[b, n - 1] = sep
    raw["input_mask"] = (ids != 0).astype(np.int64)
    assert [int(v) for v in raw["input_mask"].sum(1)] == list(lens)
    return raw


# ---------------------------------------------------------------------------------------------------------------- engine level
@pytest.mark.parametrize("pair", [1, 0])
@pytest.mark.parametrize("T,lens", [(20, (1, 15, 16, 17, 20)), (30, (1, 15, 16, 17, 20, 30))])
@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "bf16x3_fwd"])
def test_trimmed_tiles_are_bit_identical_in_the_engine(lib, precision, T, lens, pair):
    """Packed rows with question lengths on both sides of the 16-row tile edge, 36 regions, two cross layers (both cross directions: <2,3> language
    queries over region keys and <3,2> region queries over language keys), train mode with dropout 0.1; the two problems of a stage as one
    launch (key 16 = 1) and as two: logits and every gradient equal the untrimmed run's bit for bit."""
    raw = batch_with_lengths(T, lens, MED)
    b = {k: torch.from_numpy(v).cuda() for k, v in raw.items() if k != "lengths"}
    outs = {}
    try:
        assert lib.rgqa_debug_set(16, pair) == 0
        for trim in (0, 1):
            assert lib.rgqa_debug_set(23, trim) == 0
            e = make_engine(MED, precision, dropout=0.1)
            e.ensure_shape(len(lens), T, 36)
            e.sync_weights()
            lg, _ = e.forward(b["feats"], b["boxes"], b["input_ids"], b["input_mask"], b["segment_ids"], train=True, seed=99, lengths=list(lens))
            lg = lg.clone()
            e.loss_backward(b["target"])
            torch.cuda.synchronize()
            outs[trim] = (lg, e.grads.clone())
    finally:
        lib.rgqa_debug_set(23, 1)
        lib.rgqa_debug_set(16, 1)
    assert torch.equal(outs[0][0], outs[1][0])
    assert torch.equal(outs[0][1], outs[1][1])
    assert bool(torch.isfinite(outs[1][0]).all()) and float(outs[1][1].abs().max()) > 0


# ---------------------------------------------------------------------------------------------------------------- operator level
def split(lib, x):
    x = x.contiguous().float()
    out = torch.empty(x.shape, dtype=torch.int32, device="cuda")
    assert x.numel() % 32 == 0 and out.data_ptr() % 128 == 0
    ck(lib.rgqa_split_f32(P(x), P(out), x.numel(), S()))
    return out


def unsplit(lib, x):
    out = torch.empty(x.shape, dtype=torch.float32, device="cuda")
    ck(lib.rgqa_unsplit_f32(P(x), P(out), x.numel(), S()))
    return out


def windows(lens):
    """(cu tensor, total rows) of a packed operand; (None, None) for a padded one"""
    if lens is None:
        return None, None
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return torch.from_numpy(cu).cuda(), int(cu[-1])


OP_CASES = [
    # Lq, Lk, query lengths (None = padded), key lengths
    (20, 20, (3, 16, 17, 20, 9, 1), "q"),             # language self-attention: <2,2> launch, <1,1> and <2,2> bodies
    (30, 30, (30, 16, 17, 5, 24), "q"),               # T = 30
    (20, 36, (16, 20, 7, 17), None),                  # language queries over regions: <2,3> -> <1,3>
    (36, 20, None, (16, 20, 7, 17)),                  # region queries over language keys: <3,2> -> <3,1>
    (20, 30, (16, 20, 2, 17), (30, 16, 17, 9)),       # both dimensions on their own: <1,2>, <2,1>, <1,1>, <2,2> in one launch
    (56, 56, (41, 48, 49, 56), "q"),                  # UNITER's [text ; regions] rows: <4,4> -> <3,3>
    (36, 36, (36, 32, 33), "q"),                      # a three-tile dimension one tile short
]


@pytest.mark.parametrize("dtype", [1, 2])
@pytest.mark.parametrize("Lq,Lk,lq,lk", OP_CASES)
def test_trimmed_tiles_forward_backward_single_problem(lib, dtype, Lq, Lk, lq, lk):
    """The single-problem kernels (what the language-only layers and the last cross layer launch) on cu_q / cu_k row windows that mix short and
    long samples, forward and backward: trimmed and untrimmed runs are bit-equal, and both are held to the reference kernels of attn.hip on the
    same windows with the tolerances of tests/test_gpu_ops.py (bf16: 2e-2 context, 1e-2 / 1e-3 log-sum-exp, 2e-2 Frobenius gradients; split f32:
    5e-5 context and gradients, 1e-4 log-sum-exp)."""
    nh, H = 4, 256
    if lk == "q":
        lk = lq
    B = len(lq if lq is not None else lk)
    cu_q, nq = windows(lq)
    cu_k, nk = windows(lk)
    nq = nq if nq is not None else B * Lq
    nk = nk if nk is not None else B * Lk
    qf, kvf, dof = rnd(nq, H, seed=7), rnd(nk, 2 * H, seed=8), rnd(nq, H, seed=9)
    if dtype == 1:
        q, kv, do = qf.bfloat16(), kvf.bfloat16(), dof.bfloat16()
        val = lambda t: t.float()                                           # noqa: E731
        new = lambda r, c: torch.full((r, c), 3.0, dtype=torch.bfloat16, device="cuda")      # noqa: E731
    else:
        q, kv, do = split(lib, qf), split(lib, kvf), split(lib, dof)
        val = lambda t: unsplit(lib, t)                                     # noqa: E731
        new = lambda r, c: split(lib, torch.full((r, c), 3.0, device="cuda"))                 # noqa: E731
    # a padded key side carries the additive mask of its lengths; packed keys need none
    mask = None
    if lk is None:
        klen = torch.tensor([max(1, Lk - 5 * i) for i in range(B)])
        mask = ((torch.arange(Lk)[None, :] >= klen[:, None]).float() * -10000.0).cuda()

    def run_once(impl):
        out, lse = new(nq, H), torch.full((B, nh, Lq), 5.0, device="cuda")
        ck(lib.rgqa_op_attention_rows(P(q), H, P(kv), 2 * H, P(cu_q), P(cu_k), P(mask), P(out), P(lse), B, nh, Lq, Lk, dtype, impl, S()))
        dq, dkv = new(nq, H), new(nk, 2 * H)
        ck(lib.rgqa_op_attention_rows_bwd(P(q), H, P(kv), 2 * H, P(cu_q), P(cu_k), P(mask), P(lse), P(do), P(dq), P(dkv), B, nh, Lq, Lk, dtype, impl, S()))
        torch.cuda.synchronize()
        return out, lse, dq, dkv

    res = {}
    try:
        for trim in (0, 1):
            assert lib.rgqa_debug_set(23, trim) == 0
            res[trim] = run_once(1)
    finally:
        lib.rgqa_debug_set(23, 1)
    for x, y in zip(res[0], res[1]):
        assert torch.equal(x, y)
    ref = run_once(0)
    # every row of q / out / dq is a real token's (packed, or padded and full); the [B, nh, Lq] log-sum-exp has slots past a packed sample's length
    lse_ok = (torch.arange(Lq)[None, :] < torch.tensor(lq if lq is not None else [Lq] * B)[:, None]).cuda()
    out, lse, dq, dkv = (val(res[1][0]), res[1][1], val(res[1][2]), val(res[1][3]))
    rout, rlse, rdq, rdkv = (val(ref[0]), ref[1], val(ref[2]), val(ref[3]))
    lse_m, rlse_m = lse.permute(0, 2, 1)[lse_ok], rlse.permute(0, 2, 1)[lse_ok]
    err_o = float((out - rout).abs().max())
    rel_q = float((dq - rdq).norm() / rdq.norm())
    rel_kv = float((dkv - rdkv).norm() / rdkv.norm())
    print("attention rows dtype %d Lq %d Lk %d: ctx max err %.2e, dq %.2e, dkv %.2e (Frobenius, relative)" % (dtype, Lq, Lk, err_o, rel_q, rel_kv))
    if dtype == 1:
        np.testing.assert_allclose(out.cpu().numpy(), rout.cpu().numpy(), rtol=2e-2, atol=2e-2)
        np.testing.assert_allclose(lse_m.cpu().numpy(), rlse_m.cpu().numpy(), rtol=1e-3, atol=1e-2)
        assert rel_q < 2e-2 and rel_kv < 2e-2
    else:
        np.testing.assert_allclose(lse_m.cpu().numpy(), rlse_m.cpu().numpy(), rtol=1e-4, atol=1e-4)
        assert err_o < 5e-5 and rel_q < 5e-5 and rel_kv < 5e-5


# ---------------------------------------------------------------------------------------------------------------- extent check
@pytest.mark.parametrize("dtype", [1, 2])
def test_row_stride_beyond_the_32_bit_lane_offsets_is_rejected(lib, dtype):
    """The kernels add a 32-bit lane offset (at most 63 rows) to a 64-bit wave base, so the tensor's total extent never matters; the row pitch
    does: at ATTN_MAX_LD = 2^22 elements 64 rows no longer fit.  The launchers reject such a stride on the host, before any launch (nothing of
    that size is allocated here), and accept the largest one below it."""
    from rgqa_amd._lib import check
    nh, H, B, L = 2, 128, 1, 1
    big = 1 << 22
    if dtype == 1:
        q = torch.zeros(H, dtype=torch.bfloat16, device="cuda"); kv = torch.zeros(2 * H, dtype=torch.bfloat16, device="cuda"); out = torch.zeros_like(q)
    else:
        q = torch.zeros(H, dtype=torch.int32, device="cuda"); kv = torch.zeros(2 * H, dtype=torch.int32, device="cuda"); out = torch.zeros_like(q)
    lse = torch.zeros(B, nh, L, device="cuda")
    for ldq, ldkv in ((big, 2 * H), (H, big)):
        rc = lib.rgqa_op_attention_rows(P(q), ldq, P(kv), ldkv, None, None, None, P(out), P(lse), B, nh, L, L, dtype, 1, S())
        assert rc != 0
        with pytest.raises(RuntimeError, match="row stride out of range"):
            check(rc)
        rc = lib.rgqa_op_attention_rows_bwd(P(q), ldq, P(kv), ldkv, None, None, None, P(lse), P(q), P(out), P(kv), B, nh, L, L, dtype, 1, S())
        assert rc != 0
    # one sample of one row: a stride just below the limit addresses nothing beyond row 0
    ck(lib.rgqa_op_attention_rows(P(q), big - 32, P(kv), big - 32, None, None, None, P(out), P(lse), B, nh, L, L, dtype, 1, S()))
    torch.cuda.synchronize()
