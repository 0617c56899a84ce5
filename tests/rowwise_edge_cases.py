"""Case table of tests/test_rowwise_edges_{cpu,gpu}.py and tests/test_spkemb_kernels_gpu.py: the row-wise kernels of csrc/rowwise.hip and
csrc/spkemb.hip at every dispatch branch, tile boundary and grid-stride step, each at the smallest shape that reaches it.

A case is (kernel, name, parameters, seeded inputs, formula).  The formula is the operation written out plainly in torch, one sequence at a
time, never the packed form; it runs in the dtype of the tensors it is given:

  ref64  the formula on float64 copies of the inputs -- what the kernel is held to;
  r32    the same formula on the float32 inputs, on the CPU;
  err32  max over every output element of |r32 - ref64| / (1 + |ref64|): the reference side's own float32 error, in the units of the bound.

The bound is elementwise, |y - ref64| <= tol + tol * |ref64| with tol = max(T_k, 4 * err32): T_k is the tolerance test_kernels_gpu.py
already asserts for the kernel, the factor 4 covers the device's expf / tanhf / log10f being a few ulp from libm and another summation
order.  An f16 output adds 2**-10 * |ref64| (half an f16 ulp is 2**-11; double rounding through f32 is allowed).  Inputs of an f16 case are
rounded to f16 BEFORE the reference is taken.  Pure moves, gathers and integer paths are `exact`: the formula's float32 / int64 result is
the expected value to the last bit.  err32 comes from the reference side only, never from a kernel.

`branch(case)` restates the dispatch condition of the .hip file in Python; every case names the branch it was built to reach."""
import functools

import torch
import torch.nn.functional as F

F16_EXTRA = 2.0 ** -10
GRID_CAP = 4096 * 256            # the element-wise launchers cap their grids at 4096 workgroups of 256 threads (rowwise.hip: affine_launch,
                                 # jatts_snakebeta, jatts_gaussian_sample, jatts_flip_channels): one element more takes a second grid-stride step

# T_k: what tests/test_kernels_gpu.py asserts for the kernel in fp32 (test_layernorm, test_glu_dwconv_bn_swish, test_groupnorm_mish,
# test_snakebeta, test_hifigan_output_conv, test_gaussian_upsample); 1e-5 for every other kernel
T_K = {"layernorm": 1e-5, "glu_dwconv_bn_swish": 1e-5, "groupnorm_mish": 2e-5, "snakebeta": 2e-6, "hifigan_output": 2e-5,
       "gaussian_upsample": 1e-5}


def gen(seed):
    return torch.Generator().manual_seed(seed)


def r16(t):
    return t.half().float()


def cu_of(lens):
    cu = [0]
    for v in lens:
        cu.append(cu[-1] + v)
    return cu


def seqs(lens):
    """(b, first row, length) of every sequence of a packed batch."""
    cu = cu_of(lens)
    return [(b, cu[b], n) for b, n in enumerate(lens)]


class Case:
    def __init__(self, kernel, name, p, make, fn, expect, exact=False):
        self.kernel, self.name, self.p, self._make, self.fn, self.expect, self.exact = kernel, name, p, make, fn, expect, exact
        self.id = f"{kernel}/{name}"
        self.tk = T_K.get(kernel, 1e-5)

    @functools.cached_property
    def x(self):
        """Inputs: float32 (already rounded to f16 where p['in16']) and integer CPU tensors; None for an absent optional operand."""
        return self._make(self.p)

    def _run(self, dt):
        x = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in self.x.items()}
        return self.fn(x, self.p)

    @functools.cached_property
    def ref64(self):
        return self._run(torch.float64)

    @functools.cached_property
    def r32(self):
        return self._run(torch.float32)

    @functools.cached_property
    def err32(self):
        e = 0.0
        for k, r in self.ref64.items():
            if r.is_floating_point() and r.numel():
                e = max(e, float(((self.r32[k].double() - r).abs() / (1.0 + r.abs())).max()))
        return e

    @property
    def tol(self):
        return max(self.tk, 4.0 * self.err32)

    def allowed(self, key, out16=False):
        """Elementwise bound tensor for output `key`."""
        r = self.ref64[key].abs()
        return self.tol + self.tol * r + (F16_EXTRA * r if out16 else 0.0)


# ============================================================================================== GPU side: shared by the two GPU test files
ERR_ARG, ERR_UNSUPPORTED = -1, -3         # include/jatts_hip.h
SENTINEL = 7.5


def dt_of(f16):
    from jatts_amd import hip
    return hip.F16 if f16 else hip.F32


def tdt(f16):
    return torch.float16 if f16 else torch.float32


def dev(t, cuda, f16=False):
    if t is None:
        return None
    return t.to(cuda).half() if f16 else t.to(cuda)


def ragged(lens, cuda):
    from jatts_amd import hip
    return hip.RaggedBatch(lens, cuda)


def hold(c, key, y, out16=False):
    """Print the figures, then assert the elementwise bound."""
    ref = c.ref64[key]
    y = y.detach().cpu().double()
    assert y.shape == ref.shape, (c.id, key, y.shape, ref.shape)
    diff, allowed = (y - ref).abs(), c.allowed(key, out16)
    worst = float((diff / allowed).max()) if ref.numel() else 0.0
    print(f"{c.id}[{key}] out16={int(out16)}: max|d|={float(diff.max()) if ref.numel() else 0.0:.3e} worst |d|/allowed={worst:.3f} "
          f"tol={c.tol:.2e} (T_k={c.tk:.0e}, err32={c.err32:.2e})")
    assert bool(torch.isfinite(y).all()) and worst <= 1.0, (c.id, key, worst)


def same(c, key, y):
    want = c.r32[key]
    y = y.detach().cpu()
    y = y.float() if want.is_floating_point() else y
    assert y.shape == want.shape and torch.equal(y, want), (c.id, key)


def refused(rc, text):
    from jatts_amd import _abi
    import pytest
    return pytest.raises(_abi.JattsHipError, match=rf"rc={rc}\).*{text}")


CASES = {}


def add(kernel, name, p, make, fn, expect, exact=False):
    c = Case(kernel, name, p, make, fn, expect, exact)
    assert c.id not in CASES, c.id
    CASES[c.id] = c
    return c


def of(kernel):
    return [c for c in CASES.values() if c.kernel == kernel]


def ids_of(kernel):
    return [c.id for c in of(kernel)]


def _in(p, t):
    return r16(t) if p.get("in16") else t


# ============================================================================================================ branches (restated dispatch)
def glu_lds_bytes(k_w):
    return (64 + 2 * k_w - 1) * (64 + 1) * 4            # rowwise.hip jatts_glu_dwconv_bn_swish: (DW_TT + 2 k_w - 1) * (DW_CB + 1) floats


def hifigan_lds_bytes(c_in, k_w):
    vec = (c_in & 7) == 0                                # rowwise.hip jatts_hifigan_output: ((OUT_TT + k_w - 1) * (c_in + (vec ? 4 : 1)) + k_w * c_in) floats
    return ((256 + k_w - 1) * (c_in + (4 if vec else 1)) + k_w * c_in) * 4


def branch(c):
    """The path the launcher of c.kernel takes for c.p, restated from the .hip files (csrc/rowwise.hip unless noted)."""
    p, k = c.p, c.kernel
    if k == "layernorm":                                 # jatts_layernorm: `dim > 64 * LN_MAXV` (LN_MAXV = 32); layernorm_kernel masks `c < dim`
        return "refused" if p["dim"] > 64 * 32 else ("tail" if p["dim"] % 64 else "full")
    if k == "glu_dwconv_bn_swish":                       # jatts_glu_dwconv_bn_swish: `!(k_w & 1)`, `lds > 64 * 1024`, `k_w <= 8 / <= 32 / else`;
        if not p["K"] & 1:                               # glu_dw_kernel: `(C & 7) == 0`
            return "refused-even"
        if glu_lds_bytes(p["K"]) > 64 * 1024:
            return "refused-lds"
        kmax = 8 if p["K"] <= 8 else (32 if p["K"] <= 32 else 0)
        return f"{'vec' if (p['C'] & 7) == 0 else 'scalar'}-kmax{kmax}" + ("-ctail" if p["C"] % 64 else "")
    if k == "groupnorm_mish":                            # jatts_groupnorm_mish: `workspace && (gc & 7) == 0 && GN_TCH * gc <= 256 * GN_MAXU * 8`
        gc = p["C"] // p["G"]                            # (64 * gc <= 8192), then `groups <= GN_MAXG && (channels & 7) == 0` (GN_MAXG = 32)
        if not (p["time_split"] and (gc & 7) == 0 and 64 * gc <= 256 * 4 * 8):
            return "single-workgroup"
        return "split-rows" if p["G"] <= 32 and (p["C"] & 7) == 0 else "split-groups"
    if k == "snakebeta":                                 # snakebeta_kernel: `(C & 7) == 0`; jatts_snakebeta: grid = min(4096, ceil(total / 256))
        vec = (p["C"] & 7) == 0
        return ("vec" if vec else "scalar") + ("-stride2" if p["rows"] * p["C"] > GRID_CAP * (8 if vec else 1) else "")
    if k in ("affine_cast", "gaussian_sample", "flip_channels"):
        n = p["rows"] * (p.get("ldy") or p.get("C") or p["dim"])
        return "stride2" if n > GRID_CAP else "one-step"
    if k == "hifigan_output":                            # jatts_hifigan_output: `vec = (c_in & 7) == 0`, `lds > 64 * 1024`
        if hifigan_lds_bytes(p["C"], p["K"]) > 64 * 1024:
            return "refused-lds"
        tiles = max((n * p["mul"] + 255) // 256 for n in p["lens"])   # OUT_TT = 256
        return ("vec" if (p["C"] & 7) == 0 else "scalar") + ("-tiles" if tiles > 1 else "")
    if k == "gaussian_upsample":                         # jatts_gaussian_upsample: `max_len * 4 > 64 * 1024`; kernel: `t += 64` lane loops, `c += 64`
        if max(p["lens"]) * 4 > 64 * 1024:
            return "refused-text"
        return ("lanes2" if max(p["lens"]) > 64 else "lanes1") + ("-ctail" if p["dim"] % 64 else "")
    if k == "zero_pad_rows":                             # jatts_zero_pad_rows: grid.x = min(64, ceil(max_len * len_mul * dim / 1024)) workgroups of 256
        per = max(p["lens"]) * p["mul"] * p["dim"]
        gx = min(64, (per + 1023) // 1024)
        n = max((ln * p["mul"] - max(v, 0)) * p["dim"] for ln, v in zip(p["lens"], p["valid"]))
        return "stride2" if n > gx * 256 else "one-step"
    if k == "sq_err_sum":                                # jatts_sq_err_sum: blocks = min(256, ceil(n / 4096)), 256 threads each
        blocks = max(1, min(256, (p["n"] + 4095) // 4096))
        return f"blocks{blocks}" + ("-stride2" if p["n"] > blocks * 256 else "")
    if k == "lr_durations":                              # lr_durations_kernel: per = ceil(L / 256) entries per thread
        return f"per{max((n + 255) // 256 for n in p['lens'])}-rule{p['zero_rule']}"
    if k in ("variance_embed_add", "add_seq_vector", "gated_tanh_sigmoid", "embed_scale"):   # launched with 128 threads: `c += blockDim.x`
        return "cloop2" if p["dim"] > 128 else "cloop1"
    if k == "fbank_post":                                # spkemb.hip jatts_fbank_post: `n_mels < 1 || n_mels > 256`
        return "refused" if not 1 <= p["n_mels"] <= 256 else "run"
    if k == "frame_signal":                              # spkemb.hip jatts_frame_signal: grid.x = min(max_len, 1024): `t += gridDim.x`
        return "stride2" if max(p["frames"]) > 1024 else "one-step"
    return "run"


# ==================================================================================================================== layernorm / affine
def _ln_make(p):
    g = gen(100 + p["dim"] * 7 + p["rows"])
    rows, dim = p["rows"], p["dim"]
    x = torch.randn(rows, dim, generator=g)
    if p["kind"] == "randn":
        x = x * 3 + 1
    elif p["kind"] == "offset":                          # mean 100, std 1: a wrong mean subtraction shows
        x = x + 100.0
    elif p["kind"] == "const":                           # a constant row (3.0: every partial sum is exact) -> y = beta
        x = x * 3 + 1
        x[0] = 3.0
    return {"x": _in(p, x), "gamma": torch.randn(dim, generator=g), "beta": torch.randn(dim, generator=g)}


def _ln_fn(x, p):
    """F.layer_norm written out (two passes, biased variance): ATen's float32 CPU kernel folds mean and rstd into one scale and one bias per
    row, which on a constant row (rstd = eps^-1/2 = 1e6) cancels badly and would put ITS error into err32.  The CPU test checks this against
    F.layer_norm in float64."""
    v = x["x"]
    d = v - v.mean(-1, keepdim=True)
    return {"y": d * torch.rsqrt((d * d).mean(-1, keepdim=True) + p["eps"]) * x["gamma"] + x["beta"]}


for in16 in (False, True):
    for dim in (1, 63, 65, 80, 192, 2048):
        for rows in (1, 5):
            add("layernorm", f"dim{dim}-rows{rows}-{'f16' if in16 else 'f32'}", dict(dim=dim, rows=rows, kind="randn", eps=1e-12, in16=in16),
                _ln_make, _ln_fn, "tail" if dim % 64 else "full")
    for kind in ("offset", "const"):
        for dim in (80, 192, 2048):
            add("layernorm", f"{kind}-dim{dim}-{'f16' if in16 else 'f32'}", dict(dim=dim, rows=5, kind=kind, eps=1e-12, in16=in16),
                _ln_make, _ln_fn, "tail" if dim % 64 else "full")
LN_REFUSED = dict(dim=2049, rows=2)


def _aff_make(p):
    g = gen(200 + p["dim"])
    return {"x": torch.randn(p["rows"], p["ldx"], generator=g), "scale": torch.randn(p["dim"], generator=g) if p["scale"] else None,
            "shift": torch.randn(p["dim"], generator=g) if p["shift"] else None}


def _aff_fn(x, p):
    v = x["x"][:, p["col0"]:p["col0"] + p["dim"]]
    if x["scale"] is not None:
        v = v * x["scale"]
    if x["shift"] is not None:
        v = v + x["shift"]
    return {"y": F.pad(v, (0, (p.get("ldy") or p["dim"]) - p["dim"]))}     # ldy > dim zero-fills


for sc, sh in ((True, True), (True, False), (False, True), (False, False)):
    add("affine_cast", f"scale{int(sc)}-shift{int(sh)}", dict(rows=9, dim=80, ldx=80, col0=0, ldy=96, scale=sc, shift=sh), _aff_make, _aff_fn, "one-step")
add("affine_cast", "stride2", dict(rows=1025, dim=1023, ldx=1023, col0=0, ldy=1024, scale=True, shift=True), _aff_make, _aff_fn, "stride2")
add("affine_slice", "cols", dict(rows=9, dim=20, ldx=40, col0=13, out_ld=37, out_col0=5, scale=True, shift=True), _aff_make, _aff_fn, "run")


# ============================================================================================================ GLU + depthwise + BN + Swish
GLU_LENS = [1, 63, 64, 65, 129, 5]                       # DW_TT = 64: 63 / 64 / 65, 128 + 1; 1 and 5 are shorter than every K > 9 (K > L)


def _glu_make(p):
    g = gen(300 + p["C"] * 100 + p["K"])
    C, K, lens = p["C"], p["K"], p["lens"]
    x = torch.randn(sum(lens), 2 * C, generator=g)
    for b, o, n in seqs(lens):                           # every sequence at its own power of ten: a halo row leaked from a neighbour is large
        x[o:o + n] *= 10.0 ** (b - 2)
    return {"x": _in(p, x), "w": torch.randn(C, K, generator=g) * 0.3, "s": torch.rand(C, generator=g) + 0.5, "t": torch.randn(C, generator=g) * 0.1}


def _glu_fn(x, p):
    C, K = p["C"], p["K"]
    outs = []
    for _, o, n in seqs(p["lens"]):
        if n == 0:
            continue
        h = F.glu(x["x"][o:o + n], dim=-1).t().unsqueeze(0)
        y = F.conv1d(h, x["w"].unsqueeze(1), None, padding=(K - 1) // 2, groups=C)[0].t() * x["s"] + x["t"]
        outs.append(y * torch.sigmoid(y))
    return {"y": torch.cat(outs)}


def _glu_expect(C, K):
    return f"{'vec' if C % 8 == 0 else 'scalar'}-kmax{8 if K <= 8 else 32 if K <= 32 else 0}" + ("-ctail" if C % 64 else "")


for in16 in (False, True):
    sfx = "f16" if in16 else "f32"
    for C in (8, 72, 100):
        for K in (1, 7, 9, 31, 33):
            add("glu_dwconv_bn_swish", f"C{C}-K{K}-{sfx}", dict(C=C, K=K, lens=GLU_LENS, in16=in16), _glu_make, _glu_fn, _glu_expect(C, K))
    add("glu_dwconv_bn_swish", f"C8-K93-{sfx}", dict(C=8, K=93, lens=[65, 5], in16=in16), _glu_make, _glu_fn, _glu_expect(8, 93))   # the widest K the LDS takes
    add("glu_dwconv_bn_swish", f"zero-len-{sfx}", dict(C=72, K=7, lens=[5, 0, 70], in16=in16), _glu_make, _glu_fn, _glu_expect(72, 7))
GLU_REFUSED = {"refused-lds": dict(C=8, K=95), "refused-even": dict(C=8, K=8)}


# ======================================================================================================================== predictor head
def _ph_make(p):
    g = gen(400 + p["dim"])
    return {"x": _in(p, torch.randn(p["rows"], p["dim"], generator=g)), "w": torch.randn(p["dim"], generator=g) * (0.1 if p["dim"] > 1 else 1.0)}


def _ph_fn(x, p):
    return {"v": x["x"] @ x["w"] + p["b"]}


for in16 in (True, False):
    for dim in (1, 80, 256):
        add("predictor_head", f"dim{dim}-{'f16' if in16 else 'f32'}", dict(dim=dim, rows=5, b=0.7, offset=0.5, in16=in16), _ph_make, _ph_fn, "run")


def durations_of(v, offset):
    """duration_predictor.py:87-90 on log-durations v (float64) -> (durations, rows within 1e-4 of a .5 rounding boundary)."""
    lin = torch.exp(v.double()) - offset
    return torch.clamp(torch.round(lin), min=0).long(), (lin - torch.floor(lin) - 0.5).abs() < 1e-4


# =========================================================================================== 128-thread channel loops: dim above the block
VE_LENS = [11, 4, 1]                                     # 4 and 1 are shorter than the 9-tap kernel


def _ve_make(p):
    g = gen(500 + p["dim"] + p["kp"])
    R, dim = sum(p["lens"]), p["dim"]
    return {"hs": torch.randn(R, dim, generator=g), "p": torch.randn(R, generator=g), "e": torch.randn(R, generator=g),
            "wp": torch.randn(dim, p["kp"], generator=g), "we": torch.randn(dim, p["ke"], generator=g),
            "bp": torch.randn(dim, generator=g), "be": torch.randn(dim, generator=g)}


def _ve_fn(x, p):
    out = x["hs"].clone()
    for _, o, n in seqs(p["lens"]):
        for sig, w, b in ((x["p"], x["wp"], x["bp"]), (x["e"], x["we"], x["be"])):
            k = w.shape[1]
            out[o:o + n] += F.conv1d(sig[o:o + n].view(1, 1, n), w.unsqueeze(1), b, padding=(k - 1) // 2)[0].t()
    return {"hs": out}


def _asv_make(p):
    g = gen(520 + p["dim"])
    return {"hs": torch.randn(sum(p["lens"]), p["dim"], generator=g), "vec": torch.randn(len(p["lens"]), p["dim"], generator=g)}


def _asv_fn(x, p):
    out = x["hs"].clone()
    for b, o, n in seqs(p["lens"]):
        out[o:o + n] += x["vec"][b]
    return {"hs": out}


def _gate_make(p):
    g = gen(540 + p["dim"])
    C = p["dim"]
    return {"x": _in(p, torch.randn(sum(p["lens"]), 2 * C, generator=g) * 2), "gseq": torch.randn(len(p["lens"]), 2 * C, generator=g) if p["gseq"] else None}


def _gate_fn(x, p):
    C, outs = p["dim"], []
    for b, o, n in seqs(p["lens"]):
        v = x["x"][o:o + n]
        if x["gseq"] is not None:
            v = v + x["gseq"][b]
        outs.append(torch.tanh(v[:, :C]) * torch.sigmoid(v[:, C:]))
    return {"y": torch.cat(outs)}


def _emb_make(p):
    g = gen(560 + p["dim"])
    return {"table": torch.randn(20, p["dim"], generator=g), "ids": torch.randint(0, 20, (50,), generator=g)}


def _emb_fn(x, p):
    return {"y": x["table"][x["ids"]] * p["scale"]}


for dim in (130, 384):
    for kp, ke in ((1, 9), (9, 1)):
        add("variance_embed_add", f"dim{dim}-kp{kp}-ke{ke}", dict(dim=dim, kp=kp, ke=ke, lens=VE_LENS), _ve_make, _ve_fn, "cloop2")
    add("add_seq_vector", f"dim{dim}", dict(dim=dim, lens=VE_LENS), _asv_make, _asv_fn, "cloop2")
    for in16 in (False, True):
        for gs in (False, True):
            add("gated_tanh_sigmoid", f"C{dim}-gseq{int(gs)}-{'f16' if in16 else 'f32'}", dict(dim=dim, lens=VE_LENS, gseq=gs, in16=in16),
                _gate_make, _gate_fn, "cloop2")
    add("embed_scale", f"dim{dim}", dict(dim=dim, scale=8.0), _emb_make, _emb_fn, "cloop2", exact=True)


# ====================================================================================================================== GroupNorm + Mish
GN_LENS = [1, 63, 64, 65, 129]                           # GN_TCH = 64 rows per statistics chunk, GN_AROWS = 16 rows per apply workgroup


def _gn_make(p):
    g = gen(600 + p["C"] + p["G"])
    C, G, lens = p["C"], p["G"], p["lens"]
    x = torch.randn(sum(lens), C, generator=g) * 0.5 + 50.0     # mean 50, std 0.5
    gc = C // G
    b, o, n = seqs(lens)[p["const_seq"]]                 # group 1 of one whole utterance is constant (50.0: every partial sum is exact): rstd = eps^-1/2
    x[o:o + n, gc:2 * gc] = 50.0
    return {"x": _in(p, x), "gamma": torch.randn(C, generator=g), "beta": torch.randn(C, generator=g),
            "add": torch.randn(len(lens), C, generator=g) if p["addvec"] else None}


def _gn_fn(x, p):
    C, outs = p["C"], []
    for b, o, n in seqs(p["lens"]):
        if n == 0:
            continue
        v = x["x"][o:o + n].view(n, p["G"], C // p["G"])                 # F.group_norm written out, for the reason given at _ln_fn
        d = v - v.mean((0, 2), keepdim=True)
        y = (d * torch.rsqrt((d * d).mean((0, 2), keepdim=True) + p["eps"])).reshape(n, C) * x["gamma"] + x["beta"]
        y = F.mish(y)
        outs.append(y + x["add"][b] if x["add"] is not None else y)
    return {"y": torch.cat(outs)}


def gn_library_form(c):
    """The same through F.group_norm + F.mish in float64 (the CPU test compares the two)."""
    x, p, outs = c.x, c.p, []
    for b, o, n in seqs(p["lens"]):
        if n:
            y = F.mish(F.group_norm(x["x"][o:o + n].double().t().unsqueeze(0), p["G"], x["gamma"].double(), x["beta"].double(), p["eps"]))[0].t()
            outs.append(y + x["add"][b].double() if x["add"] is not None else y)
    return torch.cat(outs)


GN_SHAPES = [(64, 8, "split-rows"), (256, 8, "split-rows"), (512, 8, "split-rows"), (1024, 8, "split-rows"), (1088, 8, "single-workgroup"),
             (32, 8, "single-workgroup"), (320, 40, "split-groups")]
for C, G, exp in GN_SHAPES:
    lens = [65, 1] if C >= 1024 else GN_LENS
    for ts in (True, False):
        for in16, av in ((False, True), (True, True), (False, False)):
            add("groupnorm_mish", f"C{C}-G{G}-{'split' if ts else 'single'}-{'f16' if in16 else 'f32'}-add{int(av)}",
                dict(C=C, G=G, lens=lens, eps=1e-5, time_split=ts, in16=in16, addvec=av, const_seq=0 if C >= 1024 else 3),
                _gn_make, _gn_fn, exp if ts else "single-workgroup")
for C, G, exp in ((64, 8, "split-rows"), (32, 8, "single-workgroup"), (320, 40, "split-groups")):
    for ts in (True, False):
        add("groupnorm_mish", f"zero-len-C{C}-G{G}-{'split' if ts else 'single'}",
            dict(C=C, G=G, lens=[5, 0, 70], eps=1e-5, time_split=ts, in16=False, addvec=True, const_seq=2), _gn_make, _gn_fn,
            exp if ts else "single-workgroup")


# ======================================================================================== SnakeBeta and the other grid-capped element loops
def _snake_make(p):
    g = gen(700 + p["C"])
    C = p["C"]
    return {"x": _in(p, torch.randn(p["rows"], C, generator=g) * 3), "alpha": torch.rand(C, generator=g) * 2 + 0.1, "inv_beta": torch.rand(C, generator=g) + 0.2}


def _snake_fn(x, p):
    return {"y": x["x"] + x["inv_beta"] * torch.sin(x["x"] * x["alpha"]) ** 2}


for in16 in (False, True):
    for C, exp in ((6, "scalar"), (50, "scalar"), (48, "vec")):
        add("snakebeta", f"C{C}-{'f16' if in16 else 'f32'}", dict(C=C, rows=203, in16=in16), _snake_make, _snake_fn, exp)
add("snakebeta", "C6-stride2", dict(C=6, rows=GRID_CAP // 6 + 1, in16=False), _snake_make, _snake_fn, "scalar-stride2")
add("snakebeta", "C48-stride2", dict(C=48, rows=GRID_CAP * 8 // 48 + 1, in16=False), _snake_make, _snake_fn, "vec-stride2")


def _gs_make(p):
    g = gen(720 + p["C"])
    return {"stats": torch.randn(p["rows"], 2 * p["C"], generator=g), "noise": torch.randn(p["rows"], p["C"], generator=g)}


def _gs_fn(x, p):
    C = p["C"]
    return {"z": x["stats"][:, :C] + x["noise"] * torch.exp(x["stats"][:, C:]) * p["noise_scale"]}


add("gaussian_sample", "C7", dict(C=7, rows=33, noise_scale=0.667), _gs_make, _gs_fn, "one-step")
add("gaussian_sample", "C6-stride2", dict(C=6, rows=GRID_CAP // 6 + 1, noise_scale=0.667), _gs_make, _gs_fn, "stride2")


def _flip_make(p):
    return {"x": torch.randn(p["rows"], p["C"], generator=gen(740 + p["C"]))}


def _flip_fn(x, p):
    return {"y": torch.flip(x["x"], [1])}


add("flip_channels", "C7", dict(C=7, rows=33), _flip_make, _flip_fn, "one-step", exact=True)
add("flip_channels", "C7-stride2", dict(C=7, rows=GRID_CAP // 7 + 1), _flip_make, _flip_fn, "stride2", exact=True)


# ================================================================================================ l2_normalize, cfm_mix, sq_err_sum
def _l2_make(p):
    x = torch.randn(p["rows"], p["dim"], generator=gen(760 + p["dim"])) * 4
    x[2] = 0.0                                           # an all-zero row: zeros, not NaN
    return {"x": x}


def _l2_fn(x, p):
    return {"y": F.pad(F.normalize(x["x"], dim=1, eps=p["eps"]), (0, p["ldy"] - p["dim"]))}


for dim in (1, 80, 192):
    for ldy in (dim, dim + 8):
        add("l2_normalize", f"dim{dim}-ldy{ldy}", dict(rows=5, dim=dim, ldy=ldy, eps=1e-12), _l2_make, _l2_fn, "run")


def _cfm_make(p):
    g = gen(780)
    R = sum(p["lens"])
    return {"x1": torch.randn(R, p["dim"], generator=g), "z": torch.randn(R, p["dim"], generator=g), "t": torch.rand(len(p["lens"]), generator=g)}


def _cfm_fn(x, p):
    ys, us = [], []
    for b, o, n in seqs(p["lens"]):
        x1, z, t = x["x1"][o:o + n], x["z"][o:o + n], x["t"][b]
        ys.append((1 - (1 - p["sigma"]) * t) * z + t * x1)
        us.append(x1 - (1 - p["sigma"]) * z)
    return {"y": torch.cat(ys), "u": torch.cat(us)}


# jatts_cfm_mix: grid.x = min(256, ceil(max_len * dim / 256)): 900 * 80 > 65 536 takes the grid-stride step
add("cfm_mix", "ragged", dict(lens=[7, 1, 900, 0, 30], dim=80, sigma=1e-4), _cfm_make, _cfm_fn, "run")


def _sq_make(p):
    g = gen(800 + p["n"] % 1000)
    return {"a": torch.randn(p["n"], generator=g), "b": torch.randn(p["n"], generator=g)}


def _sq_fn(x, p):
    return {"s": (p["scale"] * ((x["a"].double() - x["b"].double()) ** 2).sum()).reshape(1)}      # the kernel itself accumulates in double


for n in (1, 4095, 4096, 4097, 256 * 4096 + 3):
    blocks = max(1, min(256, (n + 4095) // 4096))
    add("sq_err_sum", f"n{n}", dict(n=n, scale=0.5), _sq_make, _sq_fn, f"blocks{blocks}" + ("-stride2" if n > blocks * 256 else ""))


# ===================================================================================================================== length regulator
def _lr_make(p):
    g = gen(900 + p["dim"] + p["zero_rule"])
    lens = p["lens"]
    d = torch.cat([torch.randint(0, 5, (n,), generator=g) for n in lens]) if sum(lens) else torch.zeros(0, dtype=torch.int64)
    for b, o, n in seqs(lens):
        if b in p["zero_seqs"]:
            d[o:o + n] = 0
        elif n:
            d[o] = max(int(d[o]), 1)
    if p.get("d") is not None:
        d = torch.tensor(p["d"], dtype=torch.int64)
    return {"d": d, "x": torch.randn(sum(lens), p["dim"], generator=g)}


def _lr_fn(x, p):
    """length_regulator.py:85-107 per utterance: durations (alpha rounding, the all-zero rules), cumulative sums, then the gather into an
    output batch of p['extra'][b] frames more than sum(d): those are zero rows with index -1 (pad_list)."""
    d, xs = x["d"], x["x"]
    d_eff, cum, olens, fb, out, idx = [], [], [], [], [], []
    for b, o, n in seqs(p["lens"]):
        v = d[o:o + n].clone()
        if p["zero_rule"] == 1:
            v = torch.ones_like(v)
        elif p["alpha"] != 1.0:
            v = torch.round(v.float() * p["alpha"]).long()
        flag = p["zero_rule"] == 2 and n > 0 and int(v.sum()) == 0
        if flag:
            v = torch.ones_like(v)
        c = torch.cumsum(v, 0)
        total = int(c[-1]) if n else 0
        d_eff.append(v), cum.append(c), olens.append(total), fb.append(int(flag))
        i = torch.repeat_interleave(torch.arange(n), v)
        pad = p["extra"][b]
        out.append(torch.cat([xs[o:o + n][i], xs.new_zeros(pad, xs.shape[1])]))
        idx.append(torch.cat([i, torch.full((pad,), -1, dtype=torch.int64)]))
    return {"d_eff": torch.cat(d_eff), "cum": torch.cat(cum), "olens": torch.tensor(olens), "fallback": torch.tensor(fb),
            "out": torch.cat(out), "index": torch.cat(idx)}


for dim in (24, 65, 192):
    add("lr_durations", f"rule2-dim{dim}", dict(lens=[255, 256, 257, 1], zero_seqs=(1,), zero_rule=2, alpha=1.0, dim=dim, extra=[1, 0, 17, 0]),
        _lr_make, _lr_fn, "per2-rule2", exact=True)
add("lr_durations", "rule1", dict(lens=[255, 256, 257, 1], zero_seqs=(1,), zero_rule=1, alpha=1.0, dim=24, extra=[0, 17, 0, 1]),
    _lr_make, _lr_fn, "per2-rule1", exact=True)
add("lr_durations", "alpha1.5", dict(lens=[255, 256, 257, 1], zero_seqs=(), zero_rule=2, alpha=1.5, dim=24, extra=[0, 0, 0, 0]),
    _lr_make, _lr_fn, "per2-rule2", exact=True)
add("lr_durations", "zero-len", dict(lens=[7, 0, 9], zero_seqs=(), zero_rule=2, alpha=1.0, dim=24, extra=[0, 3, 0]),
    _lr_make, _lr_fn, "per1-rule2", exact=True)
# 16 output frames per lr_gather workgroup: 15 / 16 / 17 frames
add("lr_durations", "lout-15-16-17", dict(lens=[3, 3, 3], zero_seqs=(), zero_rule=0, alpha=1.0, dim=65, extra=[0, 0, 0], d=[5, 5, 5, 5, 5, 6, 5, 6, 6]),
    _lr_make, _lr_fn, "per1-rule0", exact=True)


# ========================================================================================================================= zero_pad_rows
def _zp_make(p):
    rows = sum(p["lens"]) * p["mul"]
    shape = (rows,) if p["one_d"] else (rows, p["dim"])
    return {"x": _in(p, torch.randn(*shape, generator=gen(1000 + p["dim"])) + 3.0)}      # no element is zero by accident


def _zp_fn(x, p):
    """Sequence b owns rows cu[b] * mul .. cu[b+1] * mul - 1; rows t >= valid[b] of it are zeroed (valid counts multiplied rows)."""
    out = x["x"].clone()
    for (b, o, n), v in zip(seqs(p["lens"]), p["valid"]):
        out[o * p["mul"] + max(v, 0):(o + n) * p["mul"]] = 0
    return {"x": out}


ZP_LENS = [5, 3, 4, 6]
for in16 in (False, True):
    for one_d in (False, True):
        add("zero_pad_rows", f"{'1d' if one_d else '2d'}-{'f16' if in16 else 'f32'}",
            dict(lens=ZP_LENS, valid=[0, 3, 7, -2], mul=1, dim=1 if one_d else 24, one_d=one_d, in16=in16), _zp_make, _zp_fn, "one-step", exact=True)
    add("zero_pad_rows", f"stride2-{'f16' if in16 else 'f32'}", dict(lens=[300, 2], valid=[10, 1], mul=1, dim=256, one_d=False, in16=in16),
        _zp_make, _zp_fn, "stride2", exact=True)
    add("zero_pad_rows", f"len-mul2-{'f16' if in16 else 'f32'}", dict(lens=[5, 3, 4], valid=[3, 6, 0], mul=2, dim=24, one_d=False, in16=in16),
        _zp_make, _zp_fn, "one-step", exact=True)


# ===================================================================================================================== gaussian upsample
GU_LENS = [1, 64, 65, 130]


def _gu_make(p):
    g = gen(1100 + p["dim"])
    lens = p["lens"]
    d = torch.cat([torch.randint(0, 4, (n,), generator=g) for n in lens])               # zeros included
    for b, o, n in seqs(lens):
        if n > 1:
            d[o + n // 2] = 40                           # one long token
        d[o + n - 1] = 0
        d[o + n - 1] = 4 - int(d[o:o + n].sum()) % 4 + 1     # Lout % 4 == 1: the last workgroup of every utterance has idle waves
    return {"d": d, "hs": torch.randn(sum(lens), p["dim"], generator=g)}


def _gu_fn(x, p):
    outs = []
    dt = x["hs"].dtype
    for _, o, n in seqs(p["lens"]):
        ds = x["d"][o:o + n].to(dt)
        t = torch.arange(int(x["d"][o:o + n].sum())).to(dt)
        c = ds.cumsum(0) - ds / 2                        # length_regulator.py:143
        outs.append(torch.softmax(-p["delta"] * (t[:, None] - c[None]) ** 2, dim=1) @ x["hs"][o:o + n])
    return {"y": torch.cat(outs)}


def gu_olens(c):
    return [int(c.x["d"][o:o + n].sum()) for _, o, n in seqs(c.p["lens"])]


for dim in (16, 80, 192):
    add("gaussian_upsample", f"dim{dim}", dict(lens=GU_LENS, dim=dim, delta=0.1), _gu_make, _gu_fn, "lanes2" + ("-ctail" if dim % 64 else ""))
add("gaussian_upsample", "short-dim80", dict(lens=[1, 64], dim=80, delta=0.1), _gu_make, _gu_fn, "lanes1-ctail")
GU_REFUSED = dict(lens=[16385], dim=16)


# ================================================================================================================= HiFi-GAN output conv
def _ho_make(p):
    g = gen(1200 + p["C"] * 10 + p["K"] + p["n_in"])
    R = sum(p["lens"]) * p["mul"]
    x = {f"x{i}": _in(p, torch.randn(R, p["C"], generator=g)) for i in range(p["n_in"])}
    x["w"] = torch.randn(p["K"], p["C"], generator=g) * 0.1
    return x


def _ho_fn(x, p):
    outs = []
    bias = torch.tensor([p["bias"]], dtype=x["w"].dtype)
    for _, o, n in seqs(p["lens"]):
        o, n = o * p["mul"], n * p["mul"]
        if n == 0:
            continue
        s = sum(x[f"x{i}"][o:o + n] for i in range(p["n_in"]))
        a = F.leaky_relu(s * p["in_scale"], p["slope"]).t().unsqueeze(0)
        outs.append(torch.tanh(F.conv1d(a, x["w"].t().unsqueeze(0), bias, padding=(p["K"] - 1) // 2)).reshape(-1))
    return {"y": torch.cat(outs)}


for in16 in (False, True):
    for C in (32, 12):
        for n_in, K in ((1, 3), (2, 7), (3, 3), (3, 7)):
            for mul, lens in ((16, [16, 1, 17]), (1, [255, 257])):       # 256 / 16 / 272 samples; 255 / 257: around OUT_TT = 256
                add("hifigan_output", f"C{C}-n{n_in}-K{K}-mul{mul}-{'f16' if in16 else 'f32'}",
                    dict(C=C, K=K, n_in=n_in, mul=mul, lens=lens, in_scale=1.0 / n_in, slope=0.01, bias=0.3, in16=in16), _ho_make, _ho_fn,
                    ("vec" if C % 8 == 0 else "scalar") + "-tiles")
        add("hifigan_output", f"zero-len-C{C}-{'f16' if in16 else 'f32'}",
            dict(C=C, K=7, n_in=2, mul=16, lens=[3, 0, 2], in_scale=0.5, slope=0.01, bias=0.3, in16=in16), _ho_make, _ho_fn,
            "vec" if C % 8 == 0 else "scalar")
HO_REFUSED = dict(C=64, K=7)


# ========================================================================================================================== spkemb.hip
def _fs_make(p):
    g = gen(1300)
    return {"x": torch.randn(sum(p["samples"]), generator=g), "window": torch.hann_window(p["n_fft"], periodic=True) + 0.25}


def _fs_fn(x, p):
    """frames[t][i] = window[i] * x[t * hop + i - n_fft / 2], zero outside the signal and in the columns i >= n_fft (indexed, one value at a time)."""
    n_fft, hop = p["n_fft"], p["hop"]
    outs = []
    for (_, s0, n), T in zip(seqs(p["samples"]), p["frames"]):
        sig = x["x"][s0:s0 + n]
        pos = torch.arange(T)[:, None] * hop + torch.arange(n_fft)[None] - n_fft // 2
        ok = (pos >= 0) & (pos < n)
        fr = torch.where(ok, sig[pos.clamp(0, n - 1)] * x["window"][None], torch.zeros((), dtype=sig.dtype))
        outs.append(F.pad(fr, (0, p["ldo"] - n_fft)))
    return {"y": torch.cat(outs)}


FS_SAMPLES = [3, 16, 4200]
add("frame_signal", "n16-hop4", dict(n_fft=16, hop=4, ldo=24, samples=FS_SAMPLES, frames=[n // 4 + 1 for n in FS_SAMPLES]), _fs_make, _fs_fn,
    "stride2", exact=True)


def _ps_make(p):
    return {"x": torch.randn(p["rows"], p["ldx"], generator=gen(1320)) * 3}


def _ps_fn(x, p):
    nb = p["n_bins"]
    return {"y": F.pad(x["x"][:, :nb] ** 2 + x["x"][:, nb:2 * nb] ** 2, (0, p["ldo"] - nb))}


add("power_spectrum", "bins9", dict(rows=37, n_bins=9, ldx=21, ldo=12), _ps_make, _ps_fn, "run")


def _fb_make(p):
    g = gen(1340 + p["n_mels"])
    lens, ldp = p["lens"], p["n_mels"] + 3
    pw = torch.rand(sum(lens), ldp, generator=g) * 1.5 + 0.5                             # within 6 dB: the top_db floor does not bind
    b, o, n = seqs(lens)[0]
    pw[o:o + n] = 10.0 ** (torch.rand(n, ldp, generator=g) * 15 - 12)                    # 150 dB of range, some below amin: the floor binds
    return {"p": pw}


def _fb_fn(x, p):
    outs = []
    for _, o, n in seqs(p["lens"]):
        db = 10.0 * torch.log10(torch.clamp(x["p"][o:o + n, :p["n_mels"]], min=p["amin"]))
        db = torch.maximum(db, db.max() - p["top_db"])                                   # per utterance
        outs.append(F.pad(db - db.mean(0, keepdim=True), (0, p["ldo"] - p["n_mels"])))
    return {"y": torch.cat(outs)}


def fb_floor_binds(c):
    """Per utterance: does max(dB) - top_db exceed the smallest dB?"""
    out = []
    for _, o, n in seqs(c.p["lens"]):
        db = 10.0 * torch.log10(torch.clamp(c.x["p"][o:o + n, :c.p["n_mels"]].double(), min=c.p["amin"]))
        out.append(bool(db.min() < db.max() - c.p["top_db"]))
    return out


for n_mels in (1, 80, 256):
    add("fbank_post", f"mels{n_mels}", dict(n_mels=n_mels, ldo=n_mels + 8, lens=[300, 1, 300], amin=1e-10, top_db=80.0), _fb_make, _fb_fn, "run")
FB_REFUSED = dict(n_mels=257)


def _sms_make(p):
    g = gen(1360 + p["dim"])
    R, ld = sum(p["lens"]), p["dim"] + 5
    lg = None
    if p["logits"]:
        lg = (torch.randn(R, ld, generator=g) * 40).clamp(-80, 80)
        lg[::7] = 80.0
        lg[3::7] = -80.0
    return {"x": torch.randn(R, ld, generator=g) * 2 + 1, "logits": lg}


def _sms_fn(x, p):
    dim, ms, ss = p["dim"], [], []
    for _, o, n in seqs(p["lens"]):
        v = x["x"][o:o + n, :dim]
        w = torch.softmax(x["logits"][o:o + n, :dim], 0) if x["logits"] is not None else torch.full_like(v, 1.0 / n)
        m = (w * v).sum(0)
        ms.append(m)
        ss.append(torch.sqrt(torch.clamp((w * (v - m) ** 2).sum(0), min=p["eps"])))
    return {"mean": torch.stack(ms), "std": torch.stack(ss)}


for dim in (1, 65, 192):
    for lg in (False, True):
        add("seq_mean_std", f"dim{dim}-logits{int(lg)}", dict(dim=dim, lens=[1, 37, 130], logits=lg, eps=1e-12), _sms_make, _sms_fn, "run")


def _saa_make(p):
    g = gen(1380 + p["pre"] * 2 + p["post"])
    dim, R = p["dim"], sum(p["lens"])
    return {"x": torch.randn(R, dim + 5, generator=g) * 2, "vec": torch.randn(len(p["lens"]), dim, generator=g) if p["vec"] else None,
            "scale": torch.randn(dim, generator=g) if p["scale"] else None, "shift": torch.randn(dim, generator=g) if p["shift"] else None}


def _saa_fn(x, p):
    dim, outs = p["dim"], []
    for b, o, n in seqs(p["lens"]):
        v = x["x"][o:o + n, :dim]
        if x["vec"] is not None:
            v = v + x["vec"][b]
        if p["pre"]:
            v = torch.relu(v)
        if x["scale"] is not None:
            v = v * x["scale"]
        if x["shift"] is not None:
            v = v + x["shift"]
        if p["post"]:
            v = torch.tanh(v)
        outs.append(F.pad(v, (0, p["ldy"] - dim)))
    return {"y": torch.cat(outs)}


for pre in (0, 1):
    for post in (0, 1):
        add("seq_affine_act", f"pre{pre}-post{post}", dict(dim=65, ldy=72, lens=[5, 0, 37], pre=pre, post=post, vec=True, scale=True, shift=True),
            _saa_make, _saa_fn, "run")
for i, (v, sc, sh) in enumerate(((False, True, True), (True, False, True), (True, True, False), (False, False, False))):
    add("seq_affine_act", f"vec{int(v)}-scale{int(sc)}-shift{int(sh)}", dict(dim=65, ldy=65, lens=[5, 0, 37], pre=i & 1, post=1, vec=v, scale=sc, shift=sh),
        _saa_make, _saa_fn, "run")


def _se_make(p):
    g = gen(1400 + int(p["resid"]))
    R, dim = sum(p["lens"]), p["dim"]
    return {"x": torch.randn(R, dim, generator=g), "s": torch.randn(len(p["lens"]), dim, generator=g) * 3,
            "resid": torch.randn(R, dim, generator=g) if p["resid"] else None}


def _se_fn(x, p):
    outs = []
    for b, o, n in seqs(p["lens"]):
        y = x["x"][o:o + n] * torch.sigmoid(x["s"][b])
        outs.append(y + x["resid"][o:o + n] if x["resid"] is not None else y)
    return {"y": torch.cat(outs)}


for rs in (False, True):
    add("se_scale_add", f"resid{int(rs)}", dict(dim=65, lens=[3, 40, 0, 1], resid=rs), _se_make, _se_fn, "run")
