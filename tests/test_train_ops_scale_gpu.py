"""The row-wise training kernels (csrc/train_ops.hip, csrc/training.hip) and the deterministic cross-workgroup reductions under them
(csrc/det_reduce.h) against independent references at the sizes where their real machinery runs: capped grids that loop, many slabs per
group, two-level trees with ragged last groups, the scalar slab path of odd widths, LDS index windows -- none of which the toy shapes of
test_autograd_gpu.py reach, and which the recipe-batch tests only compare with themselves.

1. Cross-workgroup sums on small integers held in f32 (train_ops_scale_cases.py; the CPU companion proves every partial sum < 2**24):
   the int64 sum is the expected value to the last bit, whatever order the kernel adds in -- torch.equal, zero tolerance.  One dropped or
   double-counted row or slab moves a result by at least 1.  Accumulating outputs start from a non-zero pattern.
2. fp64 references at the same sizes where the terms are not integers, held to test_autograd_gpu.py's relerr <= 3e-5 (Adam: 1e-5).  The
   error torch's own f32 CPU kernels make against the same fp64 reference on the same inputs is printed next to every figure; one tensor
   (the CTC gradient) is named as legitimately further off in f32 and held to four times that error instead.  Never a bound from the
   kernel's output.
3. The element-wise kernels on both sides of their grid caps with ragged tails and canaries past the end; the counter-based dropout mask
   against an independent numpy restatement of its (seed, index) function.
4. Scratch hygiene: tickets back at zero after every reduction launch, big and small reductions interleaved, a scratch that is too small
   refused on the host, two identical launches of every reduction on real-valued data bit-identical.

Every kernel is called through its jatts_amd.hip wrapper (which passes the device's scratch as the trainers do), section 4 also through the
library directly with scratches of its own; the wrappers' allocators are
swapped for patterned / canary-guarded ones where a test needs to see what a kernel did NOT write."""
import contextlib
import ctypes as C
import math
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import train_ops_scale_cases as K
from helpers import relerr

pytestmark = pytest.mark.gpu
TOL = 3e-5          # test_autograd_gpu.py's per-tensor bound
TOL_ADAM = 1e-5     # test_autograd_gpu.py::test_adam_step_and_grad_clip_match_torch
TICKET_BYTES = 64 * 1024
CANARY, PAD = -777.25, 64


# ------------------------------------------------------------------------------------------ harness
@contextlib.contextmanager
def patterned_accumulators(hip, prebuilt=None):
    """The wrappers' zero-filled `+=` outputs start from K.pattern() instead; yields the list of tensors handed out.  prebuilt: {shape:
    pattern already on the device} -- a device-side clone then replaces the upload from pageable memory, which would block the host on
    the stream between two launches."""
    handed, orig = [], hip._zeros

    def take(shape, device):
        key = (shape,) if isinstance(shape, int) else tuple(shape)
        t = prebuilt[key].clone() if prebuilt is not None else K.pattern(shape).to(device)
        handed.append(t)
        return t

    hip._zeros = take
    try:
        yield handed
    finally:
        hip._zeros = orig


class _CanaryTorch:
    """Stands in for `torch` inside jatts_amd.hip: empty / empty_like hand out the head of a CANARY-filled buffer with PAD more elements
    behind it, so a store past the end -- or an element the kernel never wrote -- shows."""

    def __init__(self):
        self.bufs = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _alloc(self, shape, dtype, device):
        n = math.prod(shape)
        buf = torch.full((n + PAD,), CANARY, dtype=dtype, device=device)
        self.bufs.append((buf, n))
        return buf[:n].view(shape)

    def empty(self, *shape, dtype=None, device=None):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        return self._alloc(tuple(shape), dtype or torch.float32, device)

    def empty_like(self, t):
        return self._alloc(tuple(t.shape), t.dtype, t.device)

    def check(self, *outputs):
        """outputs: every tensor the test goes on to compare -- each must BE one of the guarded buffers (a wrapper that starts to allocate
        another way would otherwise lose its canary without anyone noticing)."""
        assert self.bufs, "the wrapper allocated no output"
        heads = {buf.data_ptr() for buf, _ in self.bufs}
        for t in outputs:
            assert t.data_ptr() in heads, "an output was not allocated through the canary allocator"
        for buf, n in self.bufs:
            assert bool((buf[n:] == CANARY).all()), "a kernel stored past the end of its output"


@contextlib.contextmanager
def canaries(hip):
    proxy, orig = _CanaryTorch(), hip.torch
    hip.torch = proxy
    try:
        yield proxy
    finally:
        hip.torch = orig


def tickets_clear(hip, dev):
    ws = hip._WS[str(dev)]
    t = ws[:TICKET_BYTES].view(torch.int32)
    bad = int((t != 0).sum())
    assert bad == 0, f"{bad} tickets left non-zero behind a reduction launch"


def run_int(hip, kernel, inp, dev):
    """One integer case through its wrapper -> {output name: device tensor}."""
    d = lambda t: None if t is None else t.to(dev)  # noqa: E731
    if kernel == "col_sum":
        return {"out": hip.col_sum(d(inp["x"]))}
    if kernel == "col_wsum":
        return {"out": hip.col_wsum(d(inp["x"]), d(inp["v"]))}
    if kernel == "col_stats0":
        o0, o1 = hip.col_stats(d(inp["x"]), shift=d(inp["shift"]))
        return {"o0": o0, "o1": o1}
    if kernel == "col_stats1":
        o0, o1 = hip.col_stats(d(inp["x"]), y2=d(inp["dy"]), shift=d(inp["shift"]), mul=d(inp["mul"]))
        return {"o0": o0, "o1": o1}
    if kernel == "ln_dbeta":
        _, _, db = hip.layernorm_bwd(d(inp["x"]), d(inp["dy"]), d(inp["gamma"]), 1e-5)
        return {"db": db}
    if kernel == "qkv_split_bwd":
        dqkv, du, dv = hip.qkv_split_bwd(d(inp["dqu"]), d(inp["dqv"]), d(inp["dk"]), d(inp["dvv"]))
        return {"dqkv": dqkv, "du": du, "dv": dv}
    if kernel == "seq_sum":
        return {"out": hip.seq_sum(hip.RaggedBatch(inp["lens"], dev), d(inp["x"]))}
    if kernel == "dwconv_wgrad":
        return {"dw": hip.dwconv_wgrad(hip.RaggedBatch(inp["lens"], dev), d(inp["x"]), d(inp["dy"]), inp["k"], inp["pad"])}
    if kernel == "sumsq":
        out = torch.full((), inp["start"], dtype=torch.float64, device=dev)
        return {"out": hip.sumsq(d(inp["x"]), out)}
    if kernel == "index_add_rows":
        return {"dst": hip.index_add_rows(d(inp["src"]), d(inp["idx"]), inp["n_dst"], inp["scale"], inp["skip"])}
    if kernel == "lr_segment_sum":
        rb_in, rb_out = hip.RaggedBatch(inp["lens"], dev), hip.RaggedBatch([inp["to"]] * len(inp["lens"]), dev)
        return {"dhs": hip.lr_segment_sum(rb_in, d(inp["cum"]), rb_out, d(inp["dy"]))}
    if kernel == "conv1d_wgrad":
        x, dy = d(inp["x"]), d(inp["dy"])
        dw, db = hip.conv1d_wgrad(hip.RaggedBatch(inp["lens"], dev), x, dy, x.shape[1], dy.shape[1], inp["k"], 1, inp["pad"], want_db=True)
        return {"dw": dw, "db": db}
    if kernel == "masked_loss1":
        rb = hip.RaggedBatch([inp["T"]] * inp["B"], dev)
        vl = torch.tensor(inp["valid"], dtype=torch.int32, device=dev)
        a, b = d(inp["a"]), d(inp["b"])
        loss = hip.masked_loss(rb, a, b, vl, 1, inp["scale"])
        da = hip.masked_loss_bwd(rb, a, b, vl, 1, inp["scale"], upstream=torch.tensor(inp["up"], dtype=torch.float32, device=dev))
        return {"loss": loss, "da": da}
    raise KeyError(kernel)


def check_int(hip, kernel, case, dev):
    """Run the case from patterned accumulators and compare every output with the int64 reference exactly."""
    inp = K.make(kernel, case)
    ref = K.reference(kernel, inp)
    with patterned_accumulators(hip):
        got = run_int(hip, kernel, inp, dev)
    torch.cuda.synchronize()
    if str(dev) in hip._WS:
        tickets_clear(hip, dev)
    assert set(got) == set(ref)
    for name, (want, _, acc) in ref.items():
        g = got[name].detach().double().cpu().reshape(want.shape)
        if acc:
            want = want + (inp["start"] if kernel == "sumsq" else K.pattern(want.shape).double())
        if not torch.equal(g, want):
            diff = (g - want).abs()
            raise AssertionError(f"{kernel} {K.case_id((kernel, case))} {name}: {int((diff != 0).sum())} of {diff.numel()} elements differ, "
                                 f"max |d| = {float(diff.max())}")
    if kernel == "index_add_rows":
        for j in inp["untouched"]:          # the padding row and a row no index names keep their pattern
            assert torch.equal(got["dst"][j].cpu(), K.pattern(got["dst"].shape)[j])
    return got


def hold(label, rows, tol=TOL, f32_bound=()):
    """rows: (name, kernel result, fp64 reference, the same op by torch in f32 on the CPU or None).  Prints every figure, then asserts
    relerr <= tol.  Only the tensors named in f32_bound -- where f32 arithmetic at this size is legitimately further from fp64, measured and
    written down in profiles/r09_notes.md -- are held to max(tol, 4 x the f32 CPU error) instead."""
    fails = []
    for name, got, w64, w32 in rows:
        e = relerr(got.detach().cpu(), w64.detach())
        e32 = relerr(w32.detach().double(), w64.detach()) if w32 is not None else 0.0
        bound = max(tol, 4.0 * e32) if name in f32_bound else tol
        print(f"[scale] {label} {name}: kernel relerr {e:.3e}; torch f32 on the CPU {e32:.3e}; bound {bound:.3e}")
        if not e <= bound:
            fails.append((name, e, bound))
    assert not fails, (label, fails)


def grads(fn, tensors, gy, dtype):
    """-> [y, d/d tensors...] of fn by torch autograd on the CPU in `dtype`."""
    leaves = [t.detach().to(dtype).clone().requires_grad_() for t in tensors]     # (a copy: .to() of the same dtype aliases its input)
    y = fn(*leaves)
    y.backward(gy.to(dtype))
    return [y.detach()] + [v.grad for v in leaves]


def randn(shape, seed, mean=0.0, std=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std + mean


# ------------------------------------------------------------------------------------------ 1. exact integer sums
@pytest.mark.parametrize("kc", K.ALL_INT, ids=K.case_id)
def test_cross_workgroup_sums_are_exact_on_integers(cuda, lib, kc):
    from jatts_amd import hip
    check_int(hip, kc[0], kc[1], cuda)


# ------------------------------------------------------------------------------------------ 2. fp64 references at size
LN_F64 = [(1, 81), (511, 384), (512, 384), (513, 81), (513, 384), (8176, 384), (8192, 81), (8208, 384), (24576, 81), (24576, 384),
          (513, 1536), (8208, 1536), (24576, 1536)]


@pytest.mark.parametrize("rows,dim", LN_F64)
def test_layernorm_backward_at_size(cuda, lib, rows, dim):
    from jatts_amd import hip
    x, dy = randn((rows, dim), rows + dim, 0.3, 2.0), randn((rows, dim), rows + dim + 1)
    w, b = randn((dim,), dim + 2, 0.2), randn((dim,), dim + 3)
    fn = lambda x_, w_, b_: F.layer_norm(x_, (dim,), w_, b_, 1e-12)  # noqa: E731
    r64, r32 = grads(fn, [x, w, b], dy, torch.float64), grads(fn, [x, w, b], dy, torch.float32)
    dx, dg, db = hip.layernorm_bwd(x.to(cuda), dy.to(cuda), w.to(cuda), 1e-12)
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    hold(f"layernorm_bwd {rows}x{dim}", [("dx", dx, r64[1], r32[1]), ("dgamma", dg, r64[2], r32[2]), ("dbeta", db, r64[3], r32[3])])


def test_layernorm_backward_refuses_dim_1537(cuda, lib):
    from jatts_amd import _abi, hip
    x = torch.ones(4, 1537, device=cuda)
    with pytest.raises(_abi.JattsHipError, match="dim <= 1536"):
        hip.layernorm_bwd(x, x.clone(), torch.ones(1537, device=cuda), 1e-12)


def _groupnorm_ref(lens, groups):
    def fn(x, w, b):
        outs, o = [], 0
        for n in lens:
            outs.append(F.group_norm(x[o:o + n].t().unsqueeze(0), groups, w, b, 1e-5)[0].t())
            o += n
        return torch.cat(outs)
    return fn


@pytest.mark.parametrize("dim", [256, 512])
def test_groupnorm_at_the_recipe_batch(cuda, lib, dim):
    from jatts_amd import hip
    lens, groups = K.RECIPE_FRAMES, 8
    R = sum(lens)
    x, dy = randn((R, dim), dim, 0.4, 1.3), randn((R, dim), dim + 1)
    w, b = randn((dim,), dim + 2, 0.2), randn((dim,), dim + 3)
    r64, r32 = grads(_groupnorm_ref(lens, groups), [x, w, b], dy, torch.float64), grads(_groupnorm_ref(lens, groups), [x, w, b], dy, torch.float32)
    rb = hip.RaggedBatch(lens, cuda)
    xd, wd = x.to(cuda), w.to(cuda)
    y, mean, rstd = hip.groupnorm_fwd(rb, xd, groups, wd, b.to(cuda), 1e-5)
    dx, dg, db = hip.groupnorm_bwd(rb, xd, dy.to(cuda), groups, wd, mean, rstd)
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    hold(f"groupnorm {len(lens)} seq x {dim}", [("y", y, r64[0], r32[0]), ("dx", dx, r64[1], r32[1]), ("dgamma", dg, r64[2], r32[2]),
                                                 ("dbeta", db, r64[3], r32[3])])


@pytest.mark.parametrize("rows,dim", [(257, 65), (24576, 384), (65836, 5)])
def test_snakebeta_backward_at_size(cuda, lib, rows, dim):
    from jatts_amd import hip
    x, dy = randn((rows, dim), rows, 0.2, 2.0), randn((rows, dim), rows + 1)
    al, be = randn((dim,), dim + 2, 0.1, 0.5), randn((dim,), dim + 3, 0.1, 0.5)
    fn = lambda x_, a_, b_: x_ + (1.0 / (torch.exp(b_) + 1e-9)) * torch.sin(x_ * torch.exp(a_)) ** 2  # noqa: E731
    r64, r32 = grads(fn, [x, al, be], dy, torch.float64), grads(fn, [x, al, be], dy, torch.float32)
    dx, da, db = hip.snakebeta_bwd(x.to(cuda), dy.to(cuda), al.to(cuda), be.to(cuda))
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    hold(f"snakebeta_bwd {rows}x{dim}", [("dx", dx, r64[1], r32[1]), ("dalpha", da, r64[2], r32[2]), ("dbeta", db, r64[3], r32[3])])


@pytest.mark.parametrize("rows,dim", [(24576, 384), (65836, 5)])
def test_batchnorm_backward_from_the_column_statistics_at_size(cuda, lib, rows, dim):
    """The BatchNormTrain sequence of jatts_amd/autograd.py on the raw kernels: two col_stats passes (mode 0), col_stats mode 1, bn_bwd_apply."""
    from jatts_amd import hip
    x, dy = randn((rows, dim), rows + 7, 0.7, 1.5), randn((rows, dim), rows + 8)
    w, b = randn((dim,), dim + 2, 0.2), randn((dim,), dim + 3)
    fn = lambda x_, w_, b_: F.batch_norm(x_, None, None, w_, b_, True, 0.1, 1e-5)  # noqa: E731
    r64, r32 = grads(fn, [x, w, b], dy, torch.float64), grads(fn, [x, w, b], dy, torch.float32)
    xd, dyd, wd = x.to(cuda), dy.to(cuda), w.to(cuda)
    s, _ = hip.col_stats(xd)
    mean = s / rows
    _, q = hip.col_stats(xd, shift=mean)
    var = q / rows
    rstd = torch.rsqrt(var + 1e-5)
    s_dy, s_dyx = hip.col_stats(xd, y2=dyd, shift=mean, mul=rstd)
    dx = hip.bn_bwd_apply(xd, dyd, mean, rstd, wd, s_dy, s_dyx)
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    x64 = x.double()
    hold(f"batchnorm {rows}x{dim}", [("mean", mean, x64.mean(0), x.mean(0)), ("var", var, x64.var(0, unbiased=False), x.var(0, unbiased=False)),
                                     ("dx", dx, r64[1], r32[1]), ("dgamma", s_dyx, r64[2], r32[2]), ("dbeta", s_dy, r64[3], r32[3])])


def test_adam_and_clip_norm_over_a_looping_grid(cuda, lib):
    """4 194 304 + 5 elements: adam_step's 4 096 x 1 024 grid and sumsq's 1 024 x 4 096 grid both loop, with a ragged tail."""
    from jatts_amd import hip
    n = 4194304 + 5
    p0, gs = randn((n,), 12), [randn((n,), 13 + i, 0.01, 3e-3) for i in range(3)]       # gradient norm ~ 20: the clip at 1.0 is active

    def torch_adam(dtype):
        p = p0.detach().to(dtype).clone().requires_grad_()
        opt = torch.optim.Adam([p], lr=1e-2, betas=(0.9, 0.98), eps=1e-9)
        out = []
        for g in gs:
            p.grad = g.to(dtype).clone()
            torch.nn.utils.clip_grad_norm_([p], 1.0)
            opt.step()
            out.append(p.detach().clone())
        return out

    r64, r32 = torch_adam(torch.float64), torch_adam(torch.float32)
    pd, m, v = p0.to(cuda), torch.zeros(n, device=cuda), torch.zeros(n, device=cuda)
    for step, g in enumerate(gs, 1):
        ss = torch.zeros((), dtype=torch.float64, device=cuda)
        gd = g.to(cuda)
        hip.sumsq(gd, ss)
        want_ss = float((g.double() ** 2).sum())
        # f32 squares are exact in double; the kernel's adds are at most ~300 deep (16 per thread, an 8-level tree, 256 slabs per wave): 300 x 2**-53
        assert abs(float(ss) - want_ss) <= 1e-12 * want_ss, (float(ss), want_ss)
        hip.adam_step(pd, gd, m, v, 1e-2, 0.9, 0.98, 1e-9, 0.0, step, grad_sumsq=ss, max_norm=1.0)
        torch.cuda.synchronize()
        tickets_clear(hip, cuda)
        hold(f"adam_step n={n} step {step}", [("p", pd, r64[step - 1], r32[step - 1])], tol=TOL_ADAM)
        # Beyond what the issue asks: the update itself, which relerr on p hides behind |p|.  The bound is this test's own ESTIMATE, not a
        # measured figure: ~1e-2 per step on |p| ~ 1 held in f32 (ulp 1.2e-7) is ~1e-5 of the update per step; 1e-4 leaves a decade.
        hold(f"adam_step n={n} step {step}", [("p - p0", pd.cpu().double() - p0.double(), r64[step - 1] - p0.double(), r32[step - 1].double() - p0.double())],
             tol=1e-4)


@pytest.mark.parametrize("kind,log_offset", [(0, -1.0), (1, 1.0), (0, 1.0)])
def test_masked_loss_at_size(cuda, lib, kind, log_offset):
    from jatts_amd import hip
    B, T, dim = 32, 1000, 80
    valid = K.ragged(B, T)
    a, b = randn((B * T, dim), 20 + kind, 0.3), torch.rand(B * T, dim, generator=torch.Generator().manual_seed(21)) * 4
    m = (torch.arange(T)[None, :] < torch.tensor(valid)[:, None]).reshape(-1)
    n = float(sum(valid) * dim)

    def ref(dtype):
        ar = a.detach().to(dtype).clone().requires_grad_()
        tgt = torch.log(b.to(dtype) + log_offset) if log_offset >= 0 else b.to(dtype)
        dlt = ar[m] - tgt[m]
        loss = (dlt.abs().sum() if kind == 0 else (dlt ** 2).sum()) / n
        (loss * 1.7).backward()
        return loss.detach(), ar.grad

    (l64, g64), (l32, g32) = ref(torch.float64), ref(torch.float32)
    rb = hip.RaggedBatch([T] * B, cuda)
    vl = torch.tensor(valid, dtype=torch.int32, device=cuda)
    ad, bd = a.to(cuda), b.to(cuda)
    loss = hip.masked_loss(rb, ad, bd, vl, kind, 1.0 / n, log_offset)
    da = hip.masked_loss_bwd(rb, ad, bd, vl, kind, 1.0 / n, upstream=torch.tensor(1.7, device=cuda), log_offset=log_offset)
    hold(f"masked_loss kind {kind} log_offset {log_offset}", [("loss", loss, l64, l32), ("da", da, g64, g32)])


def test_forward_sum_ctc_at_the_recipe_lengths(cuda, lib):
    from jatts_amd import hip
    B, T, N = 8, 768, 128
    ilens, olens = torch.tensor([128, 1, 100, 64, 127, 37, 128, 90]), torch.tensor([768, 5, 700, 513, 512, 300, 767, 640])
    g = torch.Generator().manual_seed(15)
    lp = torch.log_softmax(torch.randn(B, T, N, generator=g) * 2, dim=-1) + torch.randn(B, T, N, generator=g) * 0.3
    blank = -1.0

    def ref(dtype):
        lr_ = lp.detach().to(dtype).clone().requires_grad_()
        pd = F.pad(lr_, (1, 0, 0, 0, 0, 0), value=blank)
        nll = torch.stack([F.ctc_loss(pd[b, : olens[b], : ilens[b] + 1].unsqueeze(1), torch.arange(1, int(ilens[b]) + 1).unsqueeze(0),
                                      olens[b:b + 1], ilens[b:b + 1], zero_infinity=True) for b in range(B)])
        nll.sum().backward()
        return nll.detach(), lr_.grad

    (n64, g64), (n32, g32) = ref(torch.float64), ref(torch.float32)
    nll, grad = hip.ctc_forward_sum(lp.to(cuda), ilens, olens, blank, want_grad=True, grad_scale=1.0)
    # grad: 768 sequential f32 log-sum-exp steps, then exp(alpha + beta + nll - lp) turns the lattice's absolute error into a relative one;
    # torch's own f32 ctc_loss is at 3.6e-5 of fp64 on these inputs, the kernel at 3.2e-5 (profiles/r09_notes.md)
    hold("ctc_forward_sum 8x768x128", [("nll", nll, n64, n32), ("grad", grad, g64, g32)], f32_bound=("grad",))


# ------------------------------------------------------------------------------------------ 3. element-wise kernels across their grid caps
NS = [2097152 + 7, 8388608 + 7]      # blocks_for(n, 256) and blocks_for(n, 1024) stop growing at 8 192 workgroups: both crossed, ragged tails
C3 = 3                               # both n are multiples of 3: rows x 3 for the kernels that take a matrix


def _sig(t):
    return 1.0 / (1.0 + torch.exp(-t))


@pytest.mark.parametrize("n", NS)
def test_elementwise_kernels_do_not_depend_on_the_grid(cuda, lib, n):
    from jatts_amd import hip
    rows = n // C3
    assert rows * C3 == n
    x2, dy = randn((rows, 2 * C3), n, 0.1, 1.5), randn((rows, C3), n + 1)
    h, skip = randn((rows, C3), n + 2), randn((rows, C3), n + 3)
    vec = [randn((C3,), n + 4 + i, 0.5) for i in range(6)]
    v1 = randn((rows,), n + 11)
    flat = randn((n,), n + 12, 0.2, 2.0)
    A, Bm = x2[:, :C3].double(), x2[:, C3:].double()
    D = dy.double()
    x2d, dyd, hd, skd, flatd = x2.to(cuda), dy.to(cuda), h.to(cuda), skip.to(cuda), flat.to(cuda)
    vd = [t.to(cuda) for t in vec]
    approx, exact = [], []
    with canaries(hip) as guard:
        approx.append(("glu_fwd", hip.glu_fwd(x2d), A * _sig(Bm)))
        s = _sig(Bm)
        approx.append(("glu_bwd", hip.glu_bwd(x2d, dyd), torch.cat([D * s, D * A * s * (1 - s)], 1)))
        t = torch.tanh(A)
        approx.append(("gate_bwd", hip.gate_bwd(x2d, dyd), torch.cat([D * s * (1 - t * t), D * t * s * (1 - s)], 1)))
        mean, rstd, gam, sdy, sdyx = (vec[i].double() for i in range(5))
        rstd = rstd.abs() + 0.5
        xh = (h.double() - mean) * rstd
        approx.append(("bn_bwd_apply", hip.bn_bwd_apply(hd, dyd, vd[0], (vd[1].abs() + 0.5), vd[2], vd[3], vd[4]),
                       gam * rstd * (D - sdy / rows - xh * sdyx / rows)))
        ho, so = hip.split_add(x2d, hd, skd)
        exact += [("split_add h", ho, h + x2[:, :C3]), ("split_add skip", so, skip + x2[:, C3:])]
        ho, so = hip.split_add(x2d, hd, None)
        exact += [("split_add (no skip) skip", so, x2[:, C3:].clone())]
        exact.append(("concat2", hip.concat2(hd, skd, rows, C3, cuda), torch.cat([h, skip], 1)))
        exact.append(("concat2 (a only)", hip.concat2(hd, None, rows, C3, cuda), torch.cat([h, torch.zeros_like(h)], 1)))
        approx.append(("outer_rows", hip.outer_rows(v1.to(cuda), vd[0], vd[5]), v1.double()[:, None] * vec[0].double() + vec[5].double()))
        approx.append(("snakebeta_fwd", hip.snakebeta_fwd(hd, vd[0], vd[5]),
                       h.double() + torch.sin(h.double() * torch.exp(vec[0].double())) ** 2 / (torch.exp(vec[5].double()) + 1e-9)))
        f64 = flat.double()
        approx.append(("act_fwd swish", hip.act_fwd(flatd, "swish"), f64 * _sig(f64)))
        exact.append(("act_fwd relu", hip.act_fwd(flatd, "relu"), torch.relu(flat)))
        approx.append(("act_fwd tanh", hip.act_fwd(flatd, "tanh"), torch.tanh(f64)))
        gyf = randn((n,), n + 13)
        sf = _sig(f64)
        approx.append(("act_bwd swish", hip.act_bwd(flatd, gyf.to(cuda), "swish"), gyf.double() * sf * (1 + f64 * (1 - sf))))
        exact.append(("act_bwd relu", hip.act_bwd(flatd, gyf.to(cuda), "relu"), gyf * (flat > 0).float()))
        # the Q|K|V head split: B = 1, T = rows, H = 3 heads of d_k = 1 (A = 3) -- a pure gather plus one f32 add
        qkv = randn((rows, 3 * C3), n + 14)
        qu, qv, kk, vv = hip.qkv_split(qkv.to(cuda), vd[0], vd[5], 1, rows, C3)
        heads = lambda m_: m_.view(1, rows, C3, 1).permute(0, 2, 1, 3).contiguous()  # noqa: E731
        exact += [("qkv_split q+u", qu, heads(qkv[:, :C3] + vec[0])), ("qkv_split q+v", qv, heads(qkv[:, :C3] + vec[5])),
                  ("qkv_split k", kk, heads(qkv[:, C3:2 * C3])), ("qkv_split v", vv, heads(qkv[:, 2 * C3:]))]
        # the counter-based mask kernels: n = 2 097 159 loops dropout / dropout_add (256 per workgroup) but not act_dropout (1 024), n = 8 388 615 all
        seed, p, alpha = 0x5EED0000 + n, 0.1, 0.5
        keep = _keep_mask(seed, 0, n, p).double()
        inv = 1.0 / (1.0 - float(np.float32(p)))
        resid = gyf.double()
        drop = [("dropout", hip.dropout(flatd, p, seed), f64 * keep * inv),
                ("dropout_add", hip.dropout_add(flatd, gyf.to(cuda), p, alpha, seed), resid + alpha * f64 * keep * inv),
                ("dropout_add (no resid)", hip.dropout_add(flatd, None, p, alpha, seed), alpha * f64 * keep * inv),
                ("dropout_add (p = 0)", hip.dropout_add(flatd, gyf.to(cuda), 0.0, alpha, seed), resid + alpha * f64),
                ("act_dropout swish", hip.act_dropout(flatd, "swish", p, seed), f64 * sf * keep * inv),
                ("act_dropout swish bwd", hip.act_dropout(flatd, "swish", p, seed, dy=gyf.to(cuda)), gyf.double() * sf * (1 + f64 * (1 - sf)) * keep * inv)]
        approx += drop
        torch.cuda.synchronize()
        guard.check(*[got for _, got, _ in approx + exact])
    for name, got, want in exact:
        assert torch.equal(got.cpu(), want), (name, n)
    assert bool((flat != 0).all())
    for name, got, _ in (drop[0], drop[2], drop[4]):   # the mask itself, exactly: a dropped element is 0, a kept one (x, x / 2, swish(x): non-zero) is not
        assert torch.equal(got.cpu() != 0, keep.bool()), (name, n)
    hold(f"elementwise n={n}", [(name, got, want, None) for name, got, want in approx])


def _mix32(k):
    """numpy restatement of the kernels' counter-based generator (splitmix64 finaliser, high word)."""
    with np.errstate(over="ignore"):
        k = k + np.uint64(0x9E3779B97F4A7C15)
        k = (k ^ (k >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        k = (k ^ (k >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return ((k ^ (k >> np.uint64(31))) >> np.uint64(32)).astype(np.uint32)


def _keep_mask(seed, i0, n, p):
    """keep[i] for elements i0 .. i0 + n - 1: a function of (seed, i) only."""
    with np.errstate(over="ignore"):
        base = np.uint64(seed & 0xFFFFFFFFFFFFFFFF) * np.uint64(0x100000001B3)
        idx = base + np.arange(i0, i0 + n, dtype=np.uint64)
    thr = np.uint32(int(float(np.float32(p)) * 4294967296.0))
    return torch.from_numpy(_mix32(idx) >= thr)


N_DROP = 24576 * 384       # a recipe activation: 9 437 184 elements, above both grid caps


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_mask_is_a_function_of_seed_and_index_only(cuda, lib, p):
    from jatts_amd import hip
    seed, n, m = 0x1234ABCD5678, N_DROP, 100000
    x = torch.rand(n, generator=torch.Generator().manual_seed(5)) + 0.5            # never zero: y != 0 <=> kept
    xd = x.to(cuda)
    keep = _keep_mask(seed, 0, n, p)
    with canaries(hip) as guard:
        y = hip.dropout(xd, p, seed)
        y_head = hip.dropout(xd[:m].contiguous(), p, seed)
        y_tail = hip.dropout(xd[n - m:].contiguous(), p, seed)
        z = hip.dropout_add(xd, xd, p, 0.5, seed)
        ya = hip.act_dropout(xd, "relu", p, seed)
        torch.cuda.synchronize()
        guard.check()
    yc = y.cpu()
    assert torch.equal(yc != 0, keep), "dropout: the mask of element i is not mix32(seed, i) >= p"
    assert torch.equal(y_head.cpu(), yc[:m]), "the first elements of a large launch differ from a small launch with the same seed"
    # a launch over the tail slice numbers its elements from 0 again: its mask is the head's, its kept values are the tail's
    yt = y_tail.cpu()
    assert torch.equal(yt != 0, keep[:m]) and torch.equal(yc[n - m:] != 0, keep[n - m:])
    scale32 = torch.tensor(1.0, dtype=torch.float32) / (torch.tensor(1.0, dtype=torch.float32) - torch.tensor(p, dtype=torch.float32))
    assert relerr(yc, x * keep * scale32) <= 1e-6
    if p == 0.5:           # 1 / (1 - p) = 2 and alpha / (1 - p) = 1 exactly: every value is exact
        assert torch.equal(yc, x * keep * 2.0) and torch.equal(z.cpu(), x + x * keep)
    else:
        assert relerr(z.cpu(), x.double() + 0.5 * x.double() * keep / (1.0 - float(np.float32(p)))) <= 1e-6
    assert torch.equal((z.cpu() != x), keep), "dropout_add: another mask than dropout's"
    assert torch.equal(ya.cpu(), yc), "act_dropout(relu) of positive inputs is dropout"
    rate = float(keep.double().mean())
    assert abs(rate - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n), rate
    assert abs(float((yc != 0).double().mean()) - (1 - p)) <= 5 * math.sqrt(p * (1 - p) / n)


@pytest.mark.parametrize("mode", ["relu", "swish"])
def test_act_dropout_equals_act_then_dropout_at_size(cuda, lib, mode):
    from jatts_amd import hip
    n, p, seed = N_DROP + 3, 0.1, 99
    x, dy = randn((n,), 31, 0.1, 2.0).to(cuda), randn((n,), 32).to(cuda)
    with canaries(hip) as guard:
        fused, two = hip.act_dropout(x, mode, p, seed), hip.dropout(hip.act_fwd(x, mode), p, seed)
        fused_b, two_b = hip.act_dropout(x, mode, p, seed, dy=dy), hip.dropout(hip.act_bwd(x, dy, mode), p, seed)
        torch.cuda.synchronize()
        guard.check()
    assert torch.equal(fused, two) and torch.equal(fused_b, two_b)
    keep = _keep_mask(seed, 0, n, p)
    xc = x.cpu().double()
    want = (torch.relu(xc) if mode == "relu" else xc * _sig(xc)) * keep / (1.0 - float(np.float32(p)))
    assert relerr(fused.cpu(), want) <= TOL


# ------------------------------------------------------------------------------------------ 4. scratch hygiene
def test_interleaved_reductions_do_not_leak_into_each_other(cuda, lib):
    """A large reduction, then small ones of other shapes, back to back on one stream with nothing but launches (and device-side clones of
    the start patterns) between them: slabs and tickets the large launch left behind must not reach the small ones.  Each launch is
    checked as in sections 1 and 2: dbeta and the plain sums exactly, LayerNorm's dx and dgamma against fp64."""
    from jatts_amd import hip
    big, small = K.make("ln_dbeta", (24576, 384)), K.make("ln_dbeta", (37, 81))
    cs, ss = K.make("col_sum", (5, 3)), K.make("seq_sum", ([1, 1025, 64, 65], 65))
    d = lambda t: t.to(cuda)  # noqa: E731
    dev_in = {k: {n: d(t) for n, t in inp.items() if torch.is_tensor(t)} for k, inp in (("big", big), ("small", small), ("cs", cs), ("ss", ss))}
    rb = hip.RaggedBatch(ss["lens"], cuda)
    pats = {shape: K.pattern(shape).to(cuda) for shape in ((384,), (3,), (4, 65), (81,))}
    torch.cuda.synchronize()
    with patterned_accumulators(hip, prebuilt=pats):
        dx1, dg1, db1 = hip.layernorm_bwd(dev_in["big"]["x"], dev_in["big"]["dy"], dev_in["big"]["gamma"], 1e-5)
        o2 = hip.col_sum(dev_in["cs"]["x"])
        o3 = hip.seq_sum(rb, dev_in["ss"]["x"])
        dx4, dg4, db4 = hip.layernorm_bwd(dev_in["small"]["x"], dev_in["small"]["dy"], dev_in["small"]["gamma"], 1e-5)
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    for name, got, kernel, inp, out in (("layernorm 24576x384 dbeta", db1, "ln_dbeta", big, "db"), ("col_sum 5x3", o2, "col_sum", cs, "out"),
                                        ("seq_sum", o3, "seq_sum", ss, "out"), ("layernorm 37x81 dbeta", db4, "ln_dbeta", small, "db")):
        want = K.reference(kernel, inp)[out][0]
        assert torch.equal(got.double().cpu(), want + K.pattern(want.shape).double()), name
    # the non-integer outputs of the two LayerNorm launches against fp64
    for label, inp, dx, dg in (("24576x384", big, dx1, dg1), ("37x81", small, dx4, dg4)):
        dim = inp["x"].shape[1]
        fn = lambda x_, w_: F.layer_norm(x_, (dim,), w_, None, 1e-5)  # noqa: E731
        r64, r32 = grads(fn, [inp["x"], inp["gamma"]], inp["dy"], torch.float64), grads(fn, [inp["x"], inp["gamma"]], inp["dy"], torch.float32)
        hold(f"interleaved layernorm {label}", [("dx", dx, r64[1], r32[1]), ("dgamma", dg - pats[(dim,)], r64[2], r32[2])])


def test_a_scratch_that_is_too_small_is_refused_on_the_host(cuda, lib):
    """A jatts_scratch of the minimum size, then a recipe-size LayerNorm backward: JATTS_ERR_ARG naming the bytes, nothing launched, outputs
    untouched.  (An argument check in the launcher; the wrappers hand the library whatever hip._WS holds, and the normal scratch is put back.)"""
    from jatts_amd import _abi, hip
    hip.col_sum(torch.ones(4, 4, device=cuda))          # the normal scratch exists
    key = str(cuda)
    normal = hip._WS[key]
    assert normal.numel() == hip.WS_BYTES
    small = torch.zeros(TICKET_BYTES + 4096, dtype=torch.uint8, device=cuda)
    rows, dim = 24576, 384
    x, g = torch.ones(rows, dim, device=cuda), torch.ones(dim, device=cuda)
    outs = [torch.full((rows, dim), CANARY, device=cuda), torch.full((dim,), CANARY, device=cuda), torch.full((dim,), CANARY, device=cuda)]
    torch.cuda.synchronize()
    rc = lib.jatts_layernorm_bwd(x.data_ptr(), dim, x.data_ptr(), dim, g.data_ptr(), rows, dim, 1e-5, outs[0].data_ptr(), dim,
                                 outs[1].data_ptr(), outs[2].data_ptr(), C.byref(_abi.Scratch(small.data_ptr(), small.numel())),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    msg = lib.jatts_last_error().decode(errors="replace")
    assert hip._WS[key] is normal                      # a direct call leaves the wrappers' scratch alone
    hip._WS[key] = small
    try:
        with pytest.raises(_abi.JattsHipError, match="bytes of scratch"):       # and through the wrapper: the same refusal as an exception
            hip.layernorm_bwd(x, x, g, 1e-5)
    finally:
        hip._WS[key] = normal
    torch.cuda.synchronize()
    assert rc == -1, rc                                # JATTS_ERR_ARG (include/jatts_hip.h)
    named = re.search(r"(\d+) bytes of scratch", msg)
    assert named and int(named.group(1)) > small.numel() - TICKET_BYTES, msg       # a byte count, and more than was passed
    for o in outs:
        assert bool((o == CANARY).all())
    assert not bool(small.any())
    check_int(hip, "ln_dbeta", (513, 81), cuda)        # and the normal scratch works again
    assert hip._WS[key] is normal


# The same reductions through the library itself, with a jatts_scratch of the test's own (include/jatts_hip.h): what the wrappers' one scratch per
# device cannot show -- a scratch of exactly the size a launch names, and two scratches in use at once.
DIRECT = [("ln_dbeta", (513, 81)), ("col_sum", (5, 3)), ("seq_sum", ([1, 1025, 64, 65], 65)), ("sumsq", 4097)]


def direct_case(hip, kernel, case, dev):
    """-> (launch(lib, scratch or None, stream) -> rc, {output: device tensor, accumulators started from their pattern}, {output: expected float64})."""
    inp = K.make(kernel, case)
    ref = {n: w for n, (w, _, _) in K.reference(kernel, inp).items()}
    x = inp["x"].to(dev)
    p = lambda t: t.data_ptr()  # noqa: E731
    sc = lambda scratch: None if scratch is None else C.byref(scratch)  # noqa: E731
    st = lambda stream: C.c_void_p(stream.cuda_stream)  # noqa: E731
    if kernel == "ln_dbeta":
        rows, dim = case
        dy, g = inp["dy"].to(dev), inp["gamma"].to(dev)
        outs = {"dx": torch.full((rows, dim), CANARY, device=dev), "dg": K.pattern((dim,)).to(dev), "db": K.pattern((dim,)).to(dev)}
        want = {"db": ref["db"] + K.pattern((dim,)).double()}
        launch = lambda lib, scratch, stream: lib.jatts_layernorm_bwd(p(x), dim, p(dy), dim, p(g), rows, dim, 1e-5, p(outs["dx"]), dim,  # noqa: E731
                                                                      p(outs["dg"]), p(outs["db"]), sc(scratch), st(stream))
    elif kernel == "col_sum":
        rows, dim = case
        outs = {"out": K.pattern((dim,)).to(dev)}
        want = {"out": ref["out"] + K.pattern((dim,)).double()}
        launch = lambda lib, scratch, stream: lib.jatts_col_sum(p(x), dim, rows, dim, p(outs["out"]), sc(scratch), st(stream))  # noqa: E731
    elif kernel == "seq_sum":
        lens, dim = case
        rb = hip.RaggedBatch(lens, dev)
        outs = {"out": K.pattern((len(lens), dim)).to(dev)}
        want = {"out": ref["out"] + K.pattern((len(lens), dim)).double()}
        launch = lambda lib, scratch, stream: lib.jatts_seq_sum(C.byref(rb.struct()), p(x), dim, p(outs["out"]), sc(scratch), st(stream))  # noqa: E731
    else:
        assert kernel == "sumsq"
        outs = {"out": torch.full((), inp["start"], dtype=torch.float64, device=dev)}
        want = {"out": ref["out"] + inp["start"]}
        launch = lambda lib, scratch, stream: lib.jatts_sumsq(p(x), x.numel(), p(outs["out"]), sc(scratch), st(stream))  # noqa: E731
    return launch, outs, want


def assert_direct(kernel, outs, want):
    for name, w in want.items():
        assert torch.equal(outs[name].double().cpu().reshape(w.shape), w), (kernel, name)


@pytest.mark.parametrize("kernel,case", DIRECT, ids=[k for k, _ in DIRECT])
def test_a_scratch_of_exactly_the_named_size_is_enough(cuda, lib, kernel, case):
    """bytes = the tickets + the count the refusal names: accepted, exact results, nothing written behind it.  The guard half behind the
    scratch is as large as the scratch, so a size formula that is too small fails here as an assertion, not as a store outside the buffer."""
    from jatts_amd import _abi, hip
    launch, outs, want = direct_case(hip, kernel, case, cuda)
    stream = torch.cuda.current_stream()
    start = {n: t.clone() for n, t in outs.items()}
    probe = torch.zeros(16, device=cuda)
    assert launch(lib, _abi.Scratch(probe.data_ptr(), 0), stream) == -1
    named = re.search(r"(\d+) bytes of scratch", lib.jatts_last_error().decode(errors="replace"))
    assert named, lib.jatts_last_error()
    need = int(named.group(1))
    assert need > 0 and need % 4 == 0
    torch.cuda.synchronize()
    for n, t in outs.items():
        assert torch.equal(t, start[n]), (kernel, n, "a refused launch wrote an output")
    buf = torch.zeros((TICKET_BYTES + 2 * need) // 4, device=cuda)
    buf[(TICKET_BYTES + need) // 4:] = CANARY
    torch.cuda.synchronize()
    assert launch(lib, _abi.Scratch(buf.data_ptr(), TICKET_BYTES + need), stream) == 0, lib.jatts_last_error()
    torch.cuda.synchronize()
    assert_direct(kernel, outs, want)
    assert bool((buf[(TICKET_BYTES + need) // 4:] == CANARY).all()), "a launch stored behind the scratch it was given"
    assert not bool(buf[:TICKET_BYTES // 4].view(torch.int32).any()), "tickets left non-zero"


def test_two_private_scratches_on_two_streams(cuda, lib):
    """The same two integer reductions on two non-default streams, each stream with a jatts_scratch of its own and no host synchronisation in
    between: nothing orders the streams against each other, and nothing has to."""
    from jatts_amd import _abi, hip
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    bufs = [torch.zeros(TICKET_BYTES + (1 << 20), dtype=torch.uint8, device=cuda) for _ in streams]
    runs = [[(k, *direct_case(hip, k, c, cuda)) for k, c in DIRECT[:2]] for _ in streams]
    torch.cuda.synchronize()
    for i in range(2):                                   # launch i of stream 0, launch i of stream 1, ...
        for s, buf, run in zip(streams, bufs, runs):
            assert run[i][1](lib, _abi.Scratch(buf.data_ptr(), buf.numel()), s) == 0, lib.jatts_last_error()
    torch.cuda.synchronize()
    for buf, run in zip(bufs, runs):
        for kernel, _, outs, want in run:
            assert_direct(kernel, outs, want)
        assert not bool(buf[:TICKET_BYTES].view(torch.int32).any()), "tickets left non-zero"


def test_the_shared_scratch_is_handed_from_stream_to_stream(cuda, lib):
    """The small members of the interleaved sequence above through the wrappers, alternating between two non-default streams with no host
    synchronisation between the launches: the wrappers' one scratch per device changes hands at every launch, each time behind an event
    wait (hip._scratch).  The kernels never spin on a ticket, so a missing wait would show as a wrong sum, not as a hang."""
    from jatts_amd import hip
    small, cs, ss = K.make("ln_dbeta", (37, 81)), K.make("col_sum", (5, 3)), K.make("seq_sum", ([1, 1025, 64, 65], 65))
    d = lambda t: t.to(cuda)  # noqa: E731
    dev_in = {k: {n: d(t) for n, t in inp.items() if torch.is_tensor(t)} for k, inp in (("small", small), ("cs", cs), ("ss", ss))}
    rb = hip.RaggedBatch(ss["lens"], cuda)
    pats = {shape: K.pattern(shape).to(cuda) for shape in ((81,), (3,), (4, 65))}
    hip.col_sum(dev_in["cs"]["x"])                       # the scratch exists
    torch.cuda.synchronize()
    ops = [("layernorm 37x81 dbeta", "ln_dbeta", small, "db", lambda: hip.layernorm_bwd(dev_in["small"]["x"], dev_in["small"]["dy"], dev_in["small"]["gamma"], 1e-5)[2]),
           ("col_sum 5x3", "col_sum", cs, "out", lambda: hip.col_sum(dev_in["cs"]["x"])),
           ("seq_sum", "seq_sum", ss, "out", lambda: hip.seq_sum(rb, dev_in["ss"]["x"]))]
    streams = [torch.cuda.Stream(device=cuda) for _ in range(2)]
    got = []
    with patterned_accumulators(hip, prebuilt=pats):
        for i in range(2 * len(ops)):                    # six launches: every op runs once on each stream
            with torch.cuda.stream(streams[i % 2]):
                got.append((ops[i % len(ops)], ops[i % len(ops)][4]()))
    torch.cuda.synchronize()
    tickets_clear(hip, cuda)
    assert hip._WS_OWNER[str(cuda)][0] == streams[1].cuda_stream
    for (name, kernel, inp, out, _), t in got:
        want = K.reference(kernel, inp)[out][0]
        assert torch.equal(t.double().cpu(), want + K.pattern(want.shape).double()), name


def test_a_null_scratch_where_nothing_reduces(cuda, lib):
    """LayerNorm backward without the parameter gradients, the Q|K|V split without position biases: no cross-workgroup sum, scratch = NULL."""
    from jatts_amd import hip
    inp = K.make("ln_dbeta", (37, 81))
    x, dy, g = (inp[n].to(cuda) for n in ("x", "dy", "gamma"))
    dx = torch.full((37, 81), CANARY, device=cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert lib.jatts_layernorm_bwd(x.data_ptr(), 81, dy.data_ptr(), 81, g.data_ptr(), 37, 81, 1e-5, dx.data_ptr(), 81, None, None, None, stream) == 0, \
        lib.jatts_last_error()
    dx_full, _, _ = hip.layernorm_bwd(x, dy, g, 1e-5)
    torch.cuda.synchronize()
    assert torch.equal(dx, dx_full) and bool((dx != CANARY).all())
    q = K.make("qkv_split_bwd", (1, 513, 3, 27))
    dqu, dk, dvv = (q[n].to(cuda) for n in ("dqu", "dk", "dvv"))
    dqkv = torch.full((513, 3 * 81), CANARY, device=cuda)
    assert lib.jatts_qkv_split_bwd(dqu.data_ptr(), None, dk.data_ptr(), dvv.data_ptr(), 1, 513, 3, 27, dqkv.data_ptr(), None, None, None, stream) == 0, \
        lib.jatts_last_error()
    torch.cuda.synchronize()
    rows = lambda t: t.permute(0, 2, 1, 3).reshape(513, 81)  # noqa: E731
    assert torch.equal(dqkv.cpu(), torch.cat([rows(q["dqu"]), rows(q["dk"]), rows(q["dvv"])], dim=1))


def _repeat_cases(hip, dev):
    """{name: launch} of every cross-workgroup reduction at its recipe size on seeded real-valued data, where the order of the adds shows
    in the last bits (on the integer cases of section 1 every order gives the same bits, so a repeat there could not fail)."""
    R, Cc = 24576, 384
    r = lambda shape, seed, mean=0.1, std=1.0: randn(shape, seed, mean, std).to(dev)  # noqa: E731
    x, dy, v = r((R, Cc), 101, 0.3, 2.0), r((R, Cc), 102), r((R,), 103)
    vec = [r((Cc,), 104 + i, 0.2, 0.5) for i in range(3)]
    lens = K.RECIPE_FRAMES
    rb, rb_full = hip.RaggedBatch(lens, dev), hip.RaggedBatch([768] * 32, dev)
    xr, dyr = x[:sum(lens)].contiguous(), dy[:sum(lens)].contiguous()
    q = [r((32, 2, 768, 192), 110 + i) for i in range(4)]
    flat = r((4194304 + 3,), 115, 0.0, 1e-2)
    xc, dyc = r((R, 80), 116), r((R, 64), 117)
    xg = r((sum(lens), 512), 118, 0.4, 1.3)
    dyg = r((sum(lens), 512), 119)
    gam, bet = r((512,), 120, 0.2), r((512,), 121)
    _, gmean, grstd = hip.groupnorm_fwd(rb, xg, 8, gam, bet, 1e-5)
    return {
        "col_sum": lambda: (hip.col_sum(x),),
        "col_wsum": lambda: (hip.col_wsum(x, v),),
        "col_stats0": lambda: hip.col_stats(x, shift=vec[0]),
        "col_stats1": lambda: hip.col_stats(x, y2=dy, shift=vec[0], mul=vec[1].abs() + 0.5),
        "layernorm_bwd": lambda: hip.layernorm_bwd(x, dy, vec[2], 1e-12),
        "qkv_split_bwd": lambda: hip.qkv_split_bwd(*q),
        "seq_sum": lambda: (hip.seq_sum(rb, xr),),
        "dwconv_wgrad k7": lambda: (hip.dwconv_wgrad(rb, xr, dyr, 7, 3),),
        "dwconv_wgrad k31": lambda: (hip.dwconv_wgrad(rb_full, x, dy, 31, 15),),
        "dwconv_wgrad k15": lambda: (hip.dwconv_wgrad(rb, xr, dyr, 15, 7),),
        "sumsq": lambda: (hip.sumsq(flat, torch.zeros((), dtype=torch.float64, device=dev)),),
        "conv1d_wgrad k9": lambda: hip.conv1d_wgrad(rb_full, xc, dyc, 80, 64, 9, 1, 4, want_db=True),
        "groupnorm_bwd": lambda: hip.groupnorm_bwd(rb, xg, dyg, 8, gam, gmean, grstd),
        "snakebeta_bwd": lambda: hip.snakebeta_bwd(x, dy, vec[0], vec[1]),
    }


REPEAT = ["col_sum", "col_wsum", "col_stats0", "col_stats1", "layernorm_bwd", "qkv_split_bwd", "seq_sum", "dwconv_wgrad k7", "dwconv_wgrad k31",
          "dwconv_wgrad k15", "sumsq", "conv1d_wgrad k9", "groupnorm_bwd", "snakebeta_bwd"]


def test_two_identical_launches_of_each_reduction_are_bit_identical(cuda, lib):
    """The recipe-batch determinism property at kernel granularity: a failure names its kernel."""
    from jatts_amd import hip
    cases = _repeat_cases(hip, cuda)
    assert sorted(cases) == sorted(REPEAT)
    bad = []
    for name in REPEAT:
        a = [t.clone() for t in cases[name]()]
        torch.cuda.synchronize()
        tickets_clear(hip, cuda)
        b = cases[name]()
        torch.cuda.synchronize()
        tickets_clear(hip, cuda)
        assert all(bool(torch.isfinite(t).all()) and bool((t != 0).any()) for t in a), name
        if not all(torch.equal(u, w) for u, w in zip(a, b)):
            bad.append(name)
    assert not bad, bad
