"""Case table, CPU reference and epilogue-selection model of tests/test_conv_store_{cpu,gpu}.py: the OUTPUT side of jatts_conv1d -- where a result row
goes (tight, a window of a wider row, transposed into a V^T layout, two outputs from one launch), which residual it takes (none, tight, a window, in place,
the half-row in-place window of the VITS flow), which activation / alpha the epilogue applies -- on the small INTEGERS of tests/conv_geometry_cases.py.

Operands as there (|u| <= 8, |w| <= 4 at about half density, integer bias), plus an integer residual |r| <= 8 and alpha in {1, 0.5, 2}: the pre-activation
z = b + sum W u is an integer below 2**24 in every summation order, and act(z) * alpha + r for act in {none, relu} is an integer or a half-integer that an
FMA and a separate multiply / add both give exactly, in f32 and -- below 2048 / 1024 -- in f16.  The float64 value of the definition

    y[t, n] = act(b[n] + sum W u) * alpha + resid[t, resid_col0 + n]

is therefore the expected output bit for bit in every arithmetic and through every store path; tanh / swish / mish / SnakeBeta are applied to the same exact
z and held to the elementwise rule of tests/rowwise_edge_cases.py.  Every output buffer is prefilled (NaN, or the residual data of an in-place update) and
compared WHOLE: a store outside the window, a stale slack column of a V^T layout or an unwritten element inside the window fails like a wrong value.

`store_path` restates, with the predicate TEXT of the sources (SOURCE_PREDICATES, compared with csrc/ by the CPU test), which epilogue a launch takes;
the CPU test proves that the table reaches every path of every kernel and flips every predicate alone.

Pure data and CPU functions: nothing here touches the GPU or the library (profiles/r35_notes.md lists kernel -> case -> path)."""
import collections
import functools
import os
import re
import types

import torch
import torch.nn.functional as F

from conv_geometry_cases import F16_EXACT, F24, _gen, _one_thread, int_weight, reference_conv

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jatts_amd", "csrc")
NAN = float("nan")
ARITHS = ["F32", "F16", "F32S", "F32E", "F32E6"]
T_K = 2e-5                     # TOL["fp32"] of tests/test_kernels_gpu.py: z is exact in EVERY arithmetic, so the f16 kernels' activations are held to it too
F16_EXTRA = 2.0 ** -10         # the f16-store term of tests/rowwise_edge_cases.py
LENS = [200, 1, 65, 2, 64, 63]                 # lens_of at tile 64 (the halo of k 3 is below 2 rows): short utterances between long ones
REFLECT_LENS = [200, 9, 65, 10, 64, 63]        # every length >= halo + 1 of (5, 2, 4)
LENS_T128 = [300, 1, 129, 2, 128, 127]         # the same around the 128-row tiles ...
LENS_T256 = [300, 1, 257, 2, 256, 255]         # ... and the 256-row tiles of the n_out <= 64 kernels
NONLINEAR = ("tanh", "swish", "mish", "snake")


def round_up(v, m):
    return (v + m - 1) // m * m


# One launch: channel shape, (k, dil, pad), lengths, len_mul, and the store side:
#   y      None (tight) | (out_ld, out_col0): a window of a wider row-major buffer
#   r      None | ("sep", ldr, resid_col0): a residual buffer of its own | ("inplace",): resid is out, tight | ("vits",): out_col0 = resid_col0 = n_out of ONE
#          (rows, 2 n_out) buffer
#   tr     None | "rows" (no y_seq_col0: column = global row, out_ld = rows) | "vt" (RaggedBatch.vt_layout) | "seq" (a hand-built y_seq_col0)
#   split  None | n_split: two outputs, the first under `y`, the second in the vt layout
Case = collections.namedtuple("StoreCase", "name axis c_in n_out geom lens len_mul y r act alpha tr split reflect density n_in")


def _case(name, axis, n_out=136, c_in=64, geom=(3, 1, 1), lens=None, len_mul=1, y=None, r=None, act=None, alpha=1.0, tr=None, split=None, reflect=False,
          density=0.5, n_in=1):
    return Case(name, axis, c_in, n_out, geom, tuple(lens or (REFLECT_LENS if reflect else LENS)), len_mul, y, r, act, alpha, tr, split, reflect, density, n_in)


TIGHT_R = ("sep", 136, 0)
AXES = ["n_out", "placement", "residual", "transposed", "split", "act_exact", "act_nonlinear", "geometry", "inputs"]
CASES = [
    # ---- n_out: 136 two 128-wide slabs, the second partial; 132 % 8 == 4; 131 / 13 / 1 ragged last quad, scalar bias tail; 8 / 64 the narrow tiles; 392 wide
    _case("n136", "n_out"), _case("n132", "n_out", n_out=132), _case("n131", "n_out", n_out=131), _case("n13", "n_out", n_out=13),
    _case("n1", "n_out", n_out=1), _case("n8", "n_out", n_out=8), _case("n64", "n_out", n_out=64), _case("n392", "n_out", n_out=392),
    _case("n136c256", "n_out", c_in=256, density=0.25),                                   # the f16 kernel's 128-channel chunks, the async f32 pipeline
    _case("n136t128", "n_out", lens=LENS_T128), _case("n64t256", "n_out", n_out=64, lens=LENS_T256),      # the 128- and 256-row time tiles at their edges
    # ---- y placement (the baseline is n136: tight, base and rows on 16 bytes)
    _case("win16", "placement", y=(160, 8)),                 # window on 16 bytes
    _case("col2", "placement", y=(160, 2)),                  # 8 B in f32, 4 B in f16
    _case("col1odd", "placement", y=(139, 1)),               # odd out_ld
    _case("ld138", "placement", y=(138, 0)),                 # out_ld % 4 != 0, aligned base
    _case("ld140", "placement", y=(140, 0)),                 # f16: out_ld % 8 == 4
    _case("n8win16", "placement", n_out=8, y=(32, 8)),
    _case("n131win16", "placement", n_out=131, y=(160, 8)),  # the ragged quad inside a window: its neighbours are canaries
    # ---- residual
    _case("r_none", "residual", alpha=0.5),
    _case("r_tight", "residual", r=TIGHT_R, alpha=0.5),
    _case("r_win", "residual", r=("sep", 160, 8), alpha=0.5),
    _case("r_col2", "residual", r=("sep", 160, 2), alpha=0.5),
    _case("r_ld138", "residual", r=("sep", 138, 0), alpha=0.5),
    _case("r_inplace", "residual", r=("inplace",), alpha=2.0),
    _case("r_vits", "residual", r=("vits",), alpha=0.5),
    _case("r_n131", "residual", n_out=131, r=("sep", 131, 0), alpha=2.0),               # the scalar tail adds its residual
    _case("r_n132", "residual", n_out=132, r=("sep", 132, 0), alpha=0.5),
    _case("r_n64", "residual", n_out=64, r=("sep", 64, 0), alpha=0.5),
    _case("r_n64vits", "residual", n_out=64, r=("vits",), alpha=2.0),
    _case("r_win_ywin", "residual", y=(160, 8), r=("sep", 168, 8), alpha=0.5),          # both windows, different leading dimensions
    _case("r_win_ycol2", "residual", y=(160, 2), r=("sep", 160, 8), alpha=2.0),
    _case("r_n392", "residual", n_out=392, r=("sep", 392, 0), alpha=0.5),
    _case("r_win_t128", "residual", y=(160, 8), r=("sep", 168, 8), alpha=0.5, lens=LENS_T128),
    _case("r_n64vits_t256", "residual", n_out=64, r=("vits",), alpha=0.5, lens=LENS_T256),
    _case("r_win_mul2", "residual", y=(160, 8), r=("sep", 168, 8), alpha=0.5, len_mul=2, lens=[100, 1, 33, 2, 32, 31]),
    # ---- transposed
    _case("t_rows", "transposed", tr="rows"),
    _case("t_vt", "transposed", tr="vt"),
    _case("t_vt131", "transposed", n_out=131, tr="vt", act="relu", alpha=0.5),
    _case("t_seq2", "transposed", tr="seq", len_mul=2, lens=[100, 1, 33, 2, 32, 31]),    # column = y_seq_col0[b] * len_mul + pos
    _case("t_resid", "transposed", tr="rows", r=TIGHT_R, alpha=0.5),                     # transposed y, row-major residual
    _case("t_vt_resid", "transposed", tr="vt", r=("sep", 160, 8), alpha=2.0),
    _case("t_n8", "transposed", n_out=8, tr="vt"),
    # ---- two outputs: n_split = 256, the second in the vt layout
    _case("s264", "split", n_out=264, split=256), _case("s388", "split", n_out=388, split=256), _case("s259", "split", n_out=259, split=256),
    _case("s392", "split", n_out=392, split=256),
    _case("s392win", "split", n_out=392, split=256, y=(416, 8)), _case("s259win", "split", n_out=259, split=256, y=(280, 8)),
    _case("s264col2", "split", n_out=264, split=256, y=(280, 2), act="relu", alpha=0.5),
    _case("s259odd", "split", n_out=259, split=256, y=(261, 1)),
    # ---- epilogue activation, exact: none / relu x alpha 1 / 0.5 / 2, with a residual (so that the order of alpha and the residual shows)
    *[_case(f"{a or 'none'}_a{al:g}", "act_exact", r=TIGHT_R, act=a, alpha=al) for a in (None, "relu") for al in (1.0, 0.5, 2.0)],
    _case("relu_a0.5_n131_noresid", "act_exact", n_out=131, act="relu", alpha=0.5),
    # ---- epilogue activation, elementwise bound on the exact z
    *[_case(f"{a}", "act_nonlinear", act=a) for a in NONLINEAR],
    *[_case(f"{a}_resid", "act_nonlinear", act=a, r=TIGHT_R, alpha=0.5) for a in NONLINEAR],
    *[_case(f"{a}_n132", "act_nonlinear", n_out=132, act=a, alpha=2.0) for a in NONLINEAR],
    _case("tanh_n131", "act_nonlinear", n_out=131, act="tanh"), _case("mish_vt", "act_nonlinear", act="mish", tr="vt"),
    _case("snake_n64", "act_nonlinear", n_out=64, act="snake"),
    # ---- geometries new to the exact table
    _case("k1", "geometry", geom=(1, 1, 0)), _case("k1resid", "geometry", geom=(1, 1, 0), r=("inplace",), alpha=0.5),
    _case("reflect311", "geometry", geom=(3, 1, 1), reflect=True), _case("reflect524", "geometry", geom=(5, 2, 4), reflect=True),
    _case("reflect524win", "geometry", geom=(5, 2, 4), reflect=True, y=(160, 8), r=TIGHT_R, alpha=0.5),
    # (reflect padding keeps the F32 launch off the register-streamed kernel: the LDS-staged kernel's fragment-order stores under variant 0 / 3 / 4 / 5)
    _case("reflect_col2", "geometry", reflect=True, y=(160, 2)), _case("reflect_ld138", "geometry", reflect=True, y=(138, 0), r=TIGHT_R, alpha=2.0),
    _case("reflect_vt", "geometry", reflect=True, tr="vt"), _case("reflect_n131win", "geometry", reflect=True, n_out=131, y=(160, 8)),
    _case("halo34", "geometry", geom=(3, 17, 17)), _case("halo36", "geometry", geom=(5, 9, 4)),
    _case("halo36win", "geometry", geom=(5, 9, 4), y=(160, 8), r=TIGHT_R, alpha=0.5),
    # ---- summed inputs: the multi-input instantiations of every family (their own tiles: the 16 x 16 kernel's 4 x 4-fragment waves), never register-streamed
    _case("in2", "inputs", n_in=2), _case("in3_n131", "inputs", n_in=3, n_out=131), _case("in2_n64", "inputs", n_in=2, n_out=64, r=("vits",), alpha=0.5),
    _case("in2_resid", "inputs", n_in=2, y=(160, 8), r=("sep", 168, 8), alpha=0.5, lens=LENS_T128), _case("in2_col2", "inputs", n_in=2, y=(160, 2)),
    _case("in3_ld138", "inputs", n_in=3, r=("sep", 138, 0), alpha=2.0), _case("in2_vt", "inputs", n_in=2, tr="vt"),
    _case("in2_s264", "inputs", n_in=2, n_out=264, split=256), _case("in2_s264col2", "inputs", n_in=2, n_out=264, split=256, y=(280, 2)),
    _case("in2_s259odd", "inputs", n_in=2, n_out=259, split=256, y=(261, 1)),
_case("in2_relu_inplace", "inputs", n_in=2, act="relu", alpha=0.5, r=("inplace",)),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def of_axis(axis):
    return [c for c in CASES if c.axis == axis]


def halo_of(case):
    return (case.geom[0] - 1) * case.geom[1]


def wide_halo(case):
    return halo_of(case) > 32              # hip.conv_halo_fits: beyond the split / emulated kernels' staging


# ------------------------------------------------------------------------------------------ geometry of the buffers
def seq_col0(case):
    """-> (first column of every sequence in BASE units, ld) of a transposed output, or (None, rows)."""
    mul = case.len_mul
    if case.tr == "vt" or case.split:                         # RaggedBatch.vt_layout: every sequence on a multiple of 8 columns, 8 columns of slack
        col, c = [], 0
        for v in case.lens:
            col.append(c)
            c += round_up(v, 8)
        return col, (c + 8) * mul
    if case.tr == "seq":                                      # hand-built: 3 base columns of slack after every sequence, 5 in front
        col, c = [], 5
        for v in case.lens:
            col.append(c)
            c += v + 3
        return col, c * mul + 4
    return None, sum(case.lens) * mul


Layout = collections.namedtuple("Layout", "rows out_shape out_ld out_col0 resid_shape ldr resid_col0 alias out2_shape")


def layout(case):
    rows, n = sum(case.lens) * case.len_mul, case.n_out
    kind = case.r[0] if case.r else None
    if kind == "vits":
        return Layout(rows, (rows, 2 * n), 2 * n, n, (rows, 2 * n), 2 * n, n, True, None)
    if kind == "inplace":
        return Layout(rows, (rows, n), n, 0, (rows, n), n, 0, True, None)
    rs, ldr, rc = ((rows, case.r[1]), case.r[1], case.r[2]) if kind else (None, 0, 0)
    if case.tr:
        ld = seq_col0(case)[1]
        return Layout(rows, (n, ld), ld, 0, rs, ldr, rc, False, None)
    width = case.split or n
    ld, c0 = case.y or (width, 0)
    return Layout(rows, (rows, ld), ld, c0, rs, ldr, rc, False, (n - case.split, seq_col0(case)[1]) if case.split else None)


# ------------------------------------------------------------------------------------------ operands and the reference, from the definition
Data = collections.namedtuple("Data", "x xs w b rbuf snake z row_lens")


@_one_thread
def reference_z(x, w, b, row_lens, geom, reflect):
    """The integer pre-activation, float64: zero halo through conv_geometry_cases.reference_conv, reflect halo by F.pad(mode="reflect") per utterance."""
    k, dil, pad = geom
    if not reflect:
        return reference_conv(x, w, b, row_lens, k, dil, pad)
    outs, o = [], 0
    for L in row_lens:
        xs = F.pad(x[o:o + L].double().t().unsqueeze(0), (pad, (k - 1) * dil - pad), mode="reflect")
        outs.append(F.conv1d(xs, w.double(), b.double(), dilation=dil)[0].t())
        o += L
    return torch.cat(outs)


@functools.lru_cache(maxsize=None)
def data(name):
    """Inputs of a case and its exact pre-activation z; computed once per process.  The residual BUFFER is integer data in every column, so a read from
    a neighbouring column gives a wrong finite value, never a conspicuous NaN."""
    case = BY_NAME[name]
    # (cases that differ on the store side only share their operands: the store-side axes flip ONE thing against the same numbers)
    g = _gen("store", case.c_in, case.n_out, case.geom, case.lens, case.len_mul, case.reflect)
    row_lens = [v * case.len_mul for v in case.lens]
    x = torch.randint(-8, 9, (sum(row_lens), case.c_in), generator=g).float()
    w, b = int_weight(case.n_out, case.c_in, case.geom[0], g, case.density)
    L = layout(case)
    gr = _gen("store-resid", name)
    rbuf = torch.randint(-8, 9, L.resid_shape, generator=gr).double() if L.resid_shape else None
    snake = None
    if case.act == "snake":        # small per-channel a, b: (exp(alpha), 1 / (exp(beta) + 1e-9)) as the models hand them over, f32
        snake = (torch.exp(torch.rand(case.n_out, generator=gr) * 2.5 - 5.0), 1.0 / (torch.exp(torch.rand(case.n_out, generator=gr) * 2 - 1) + 1e-9))
    xs = [x]
    if case.n_in > 1:              # summed inputs (in_scale 1): integers |x_i| <= 16 whose sum is the staged operand x
        gi = _gen("store-inputs", name)
        rest = [torch.randint(-8, 9, x.shape, generator=gi).float() for _ in range(case.n_in - 1)]
        xs = [x - sum(rest)] + rest
    return Data(x, xs, w, b, rbuf, snake, reference_z(x, w, b, row_lens, case.geom, case.reflect), row_lens)


def activation(case, z, snake=None):
    """act(z) in the dtype of z (float64: the reference; float32: the reference side's own error)."""
    a = case.act
    if a is None:
        return z
    if a == "relu":
        return torch.relu(z)
    if a == "tanh":
        return torch.tanh(z)
    if a == "swish":
        return z * torch.sigmoid(z)
    if a == "mish":
        return z * torch.tanh(F.softplus(z, threshold=1e4))
    if a == "snake":
        return z + snake[1].to(z.dtype) * torch.sin(z * snake[0].to(z.dtype)) ** 2
    raise ValueError(a)


def value(case, fault=None, dtype=torch.float64):
    """(rows, n_out): act(z) * alpha + resid[:, resid_col0 : resid_col0 + n_out].  Faults (the sensitivity tests): "resid_col_minus4" reads the residual
    four columns to the left, "alpha_after_resid" scales the sum.  -> None where a fault does not apply to the case."""
    d, L = data(case.name), layout(case)
    v = activation(case, d.z.to(dtype), d.snake)
    if d.rbuf is None:
        return None if fault in ("resid_col_minus4", "alpha_after_resid") else v * case.alpha
    c0 = L.resid_col0 - (4 if fault == "resid_col_minus4" else 0)
    if c0 < 0:
        return None
    r = d.rbuf[:, c0:c0 + case.n_out].to(dtype)
    return (v + r) * case.alpha if fault == "alpha_after_resid" else v * case.alpha + r


Buffers = collections.namedtuple("Buffers", "out0 want out2_0 want2")


def place(case, val, fault=None, fill=NAN):
    """The whole output buffer(s) before and after the launch, float64: `fill` (NaN: the canaries) or -- in place -- the residual data wherever the kernel
    must not write, `val` where it must.  Faults: "partial_quad_unwritten" leaves the last n_out % 4 channels alone, "seq_col0_ignored" stores a transposed
    column at its global row, "len_mul_dropped" at y_seq_col0[b] + pos, "first_output_n_out_wide" stores the first of two outputs n_out wide.
    -> None where a fault does not apply."""
    d, L = data(case.name), layout(case)
    n = case.n_out
    out0 = d.rbuf.clone() if L.alias else torch.full(L.out_shape, fill, dtype=torch.float64)
    want = out0.clone()
    n_live = n - n % 4 if fault == "partial_quad_unwritten" else n
    if fault == "partial_quad_unwritten" and n % 4 == 0:
        return None
    if fault in ("seq_col0_ignored", "len_mul_dropped") and not (case.tr in ("vt", "seq") or case.split):
        return None
    if fault == "len_mul_dropped" and case.len_mul == 1:
        return None
    if fault == "first_output_n_out_wide" and not (case.split and L.out_col0 + n <= L.out_ld):
        return None

    def transposed(dst, v, ch0):
        col0, _ = seq_col0(case)
        o = 0
        for b, rl in enumerate(d.row_lens):
            if col0 is None or fault == "seq_col0_ignored":
                c = o
            elif fault == "len_mul_dropped":
                c = col0[b]
            else:
                c = col0[b] * case.len_mul
            dst[:v.shape[1], c:c + rl] = v[o:o + rl].t()
            o += rl

    if case.split:
        width = n if fault == "first_output_n_out_wide" else case.split
        want[:, L.out_col0:L.out_col0 + width] = val[:, :width]
        out2_0 = torch.full(L.out2_shape, fill, dtype=torch.float64)
        want2 = out2_0.clone()
        transposed(want2, val[:, case.split:n_live], case.split)
        return Buffers(out0, want, out2_0, want2)
    if case.tr:
        transposed(want, val[:, :n_live], 0)
    else:
        want[:, L.out_col0:L.out_col0 + n_live] = val[:, :n_live]
    return Buffers(out0, want, None, None)


@functools.lru_cache(maxsize=None)
def expected(name, fault=None):
    case = BY_NAME[name]
    v = value(case, fault if fault in ("resid_col_minus4", "alpha_after_resid") else None)
    return None if v is None else place(case, v, fault)


@functools.lru_cache(maxsize=None)
def bound(name):
    """Non-linear cases -> (err32, tol, allowed32, allowed16): the reference side's own float32 error of the same expression, tol = max(T_k, 4 err32), and
    the elementwise bound tol + tol |ref64| (+ 2**-10 |ref64| for an f16 store) laid out like the output buffers (NaN outside)."""
    case = BY_NAME[name]
    ref = value(case)
    r32 = value(case, dtype=torch.float32).double()
    err32 = float(((r32 - ref).abs() / (1.0 + ref.abs())).max())
    tol = max(T_K, 4.0 * err32)
    a32 = tol + tol * ref.abs()
    return err32, tol, place(case, a32), place(case, a32 + F16_EXTRA * ref.abs())


def same_buffers(a, b):
    """Two expected-buffer sets agree everywhere (NaN == NaN)."""
    return all((p is None and q is None) or torch.equal(torch.nan_to_num(p, nan=1e300), torch.nan_to_num(q, nan=1e300))
               for p, q in ((a.want, b.want), (a.want2, b.want2)))


def check_buffer(y, want, what, allowed=None):
    """A whole output buffer against its expectation: NaN exactly where `want` is NaN (nothing stored outside the window), finite everywhere else, and there
    equal to `want` after one rounding to y's dtype (allowed None) or inside the elementwise bound `allowed`.  -> the largest |d| / allowed (0 when exact)."""
    y = y.detach().cpu()
    assert tuple(y.shape) == tuple(want.shape), f"{what}: shape {tuple(y.shape)} != {tuple(want.shape)}"
    keep = torch.isnan(want)
    assert bool(torch.isnan(y[keep]).all()), f"{what}: {int((~torch.isnan(y[keep])).sum())} stores outside the output window"
    assert bool(torch.isfinite(y[~keep]).all()), f"{what}: {int((~torch.isfinite(y[~keep])).sum())} unwritten or non-finite elements inside the output window"
    if allowed is None:
        exp = want.to(y.dtype)
        bad = (y != exp) & ~keep
        if bool(bad.any()):
            rows = bad.any(1).nonzero().view(-1).tolist()
            dmax = float((y.double() - want)[bad].abs().max())
            raise AssertionError(f"{what}: {int(bad.sum())} of {int((~keep).sum())} elements differ from the integer reference (max |d| = {dmax:g}) in "
                                 f"{len(rows)} buffer rows, first {rows[:8]}")
        return 0.0
    worst = float(((y.double() - want).abs() / allowed)[~keep].max())
    assert worst <= 1.0, f"{what}: |y - ref64| is {worst:.3f} x the elementwise bound"
    return worst


# ------------------------------------------------------------------------------------------ the epilogue selection, in the sources' own words
# Every line below is program text of csrc/ (whitespace-normalised, comments stripped); tests/test_conv_store_cpu.py compares each with its file, and
# store_path EVALUATES these strings (translated token by token to Python: `c_expr`), so the model cannot drift from what it quotes.
ROWMAJOR = "const bool rowmajor = !d.y_transposed && (d.n_out & 7) == 0 && (reinterpret_cast<uintptr_t>(d.y) & 15) == 0;"
VEC = "const bool vec_r = d.resid && (d.ldr & 3) == 0, vec_y = (d.ldy & 3) == 0 && !d.y_transposed;"
VEC_STORE = "if (full && vec_y && (vec_r || !d.resid)) {"
USE_F32_TILE = ("if (rowmajor && f32_tile && (d.ldy & 3) == 0 && (!d.resid || ((d.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(d.resid) & 15) == 0))) {")
HAVE_F32_TILE_159 = "if (!d.y_transposed && (size_t)BT * (BN * 4 + 16) <= 159 * 1024) {"
SOURCE_PREDICATES = {
    "conv1d_impl.h": {
        "vec": VEC,
        "vec_store": VEC_STORE,
        "rowmajor": ROWMAJOR,
        "use_f16_tile": "if (rowmajor && !d.y_is_f32 && !d.resid && (d.ldy & 7) == 0) {",
        "use_f32_tile": ("if (rowmajor && (d.y_is_f32 || sizeof(T) == 4) && f32_tile && (d.ldy & 3) == 0 && (!d.resid || ((d.ldr & 3) == 0 && "
                         "(reinterpret_cast<uintptr_t>(d.resid) & 15) == 0))) {"),
        "have_f32_tile_f32": "if (!d.y_transposed && (size_t)BT * (BN * 4 + 16) <= 160 * 1024) {",
        "have_f32_tile_f16": "if (d.y_is_f32 && !d.y_transposed) {",
        "second_output": "if (d.n_split > 0 && n_first >= d.n_split) {",
    },
    "conv1d_direct.h": {
        "rowmajor": ("const bool rowmajor = !d.y_transposed && (d.n_out & 7) == 0 && (reinterpret_cast<uintptr_t>(d.y) & 15) == 0 && (d.ldy & 3) == 0 && "
                     "(!d.resid || ((d.ldr & 3) == 0 && (reinterpret_cast<uintptr_t>(d.resid) & 15) == 0));"),
        "direct_ok": ("return d.n_in == 1 && d.in_scale == 1.f && (d.pre_act == JATTS_PRE_NONE || (d.pre_act == JATTS_PRE_LRELU && d.pre_slope >= 0.f && "
                      "d.pre_slope <= 1.f)) && d.pad_mode == JATTS_PAD_ZERO && (d.ldx & 3) == 0 && (reinterpret_cast<uintptr_t>(d.x[0]) & 15) == 0 && "
                      "(reinterpret_cast<uintptr_t>(d.w) & 15) == 0 && (maxL + 256 + (int64_t)d.k_w * d.dil) * ld * 4 < (int64_t)1 << 31 && "
                      "(int64_t)d.k_w * d.c_in * n_pad * 4 < (int64_t)1 << 31;"),
    },
    "conv1d_split.h": {"rowmajor": ROWMAJOR, "use_f32_tile": USE_F32_TILE, "have_f32_tile": HAVE_F32_TILE_159},
    "conv1d_emul.h": {"rowmajor": ROWMAJOR, "use_f32_tile": USE_F32_TILE, "have_f32_tile": HAVE_F32_TILE_159},
    "conv1d_emul16.h": {
        "vec": VEC,
        "vec_store": VEC_STORE,
        "rowmajor": ROWMAJOR,
        "use_f32_tile": USE_F32_TILE,
        "direct_epi": "const bool direct_epi = d.resid == nullptr;",
        "have_f32_tile": "if (!direct_epi && !d.y_transposed && (size_t)BT * (BN * 4 + 16) <= 159 * 1024) {",
    },
}
# what the CPU test extracts from a source file to compare with the table above: every definition of these names, every condition that sets or tests f32_tile,
# the vector-store condition, the f16 tile's condition, the second-output test and conv_direct_ok's return
EXTRACT = [r"const bool (?:rowmajor|vec_r|direct_epi)\b[^;]*;", r"if \([^{};]*\) \{(?= f32_tile = 1;)", r"if \([^{};]*\bf32_tile\b[^{};]*\) \{",
           r"if \(full && [^{};]*\) \{", r"if \(rowmajor && !d\.y_is_f32[^{};]*\) \{", r"if \(d\.n_split > 0 && [^{};]*\) \{", r"return d\.n_in == 1[^;]*;"]


def normalise(text):
    """C text without // comments, every run of whitespace one blank."""
    return re.sub(r"\s+", " ", re.sub(r"//[^\n]*", "", text)).strip()


def source_predicates(fname):
    """{normalised statement} of a source file: everything EXTRACT matches."""
    with open(os.path.join(CSRC, fname)) as fh:
        text = normalise(fh.read())
    return {m.group(0) for pat in EXTRACT for m in re.finditer(pat, text)}


def c_expr(stmt):
    """The condition / right-hand side(s) of a quoted C statement as compiled Python: -> {name or "": code}.  A token-for-token translation: casts dropped,
    && || ! to and / or / not, float suffixes dropped, nullptr to 0; pointers are integers (their byte address)."""
    s = stmt.strip()
    s = re.sub(r"^(?:const bool |return )", "", s).rstrip(";")
    m = re.match(r"^if \((.*)\) \{$", s)
    parts = {"": m.group(1)} if m else dict(p.split(" = ", 1) for p in s.split(", ")) if " = " in s else {"": s}
    if len(parts) == 1:
        parts = {"": next(iter(parts.values()))}
    out = {}
    for name, e in parts.items():
        e = re.sub(r"reinterpret_cast<uintptr_t>", "", e)
        e = re.sub(r"\((?:size_t|int64_t)\)", "", e)
        e = re.sub(r"(\d)\.f\b", r"\1.0", e)
        e = e.replace("nullptr", "0").replace("&&", " and ").replace("||", " or ").replace("sizeof(T)", "sizeof_T")
        e = re.sub(r"!(?!=)", " not ", e)
        out[name.strip()] = compile(e.strip(), f"<{stmt[:40]}>", "eval")
    return out


_CODE = {f: {k: c_expr(v) for k, v in preds.items()} for f, preds in SOURCE_PREDICATES.items()}
_CONSTS = dict(JATTS_PRE_NONE=0, JATTS_PRE_LRELU=1, JATTS_PAD_ZERO=0, JATTS_PAD_REFLECT=1)


def _ev(fname, key, env, name=""):
    return bool(eval(_CODE[fname][key][name], dict(_CONSTS), env))


# A launch as the library sees it (jatts_conv_desc), addresses as byte offsets from a 16-byte aligned allocation
Launch = collections.namedtuple("Launch", "n_out ldy y y_is_f32 y_transposed resid ldr n_split ldy2 snake reflect k_w dil c_in n_seq max_len len_mul ldx n_in")


def launch_of(case, arith, y16=False):
    """The descriptor fields of a table case in arithmetic `arith` (y16: the f16 kernel storing f16).  Pointers: byte offset + 4096, so that a null
    residual is 0 as in the sources."""
    L = layout(case)
    esz = 2 if y16 else 4
    return Launch(case.n_out, L.out_ld, 4096 + L.out_col0 * esz, int(not y16), int(bool(case.tr)), (4096 + L.resid_col0 * 4) if case.r else 0, L.ldr,
                  case.split or 0, L.out2_shape[1] if case.split else 0, int(case.act == "snake"), int(case.reflect), case.geom[0], case.geom[1], case.c_in,
                  len(case.lens), max(case.lens), case.len_mul, case.c_in, case.n_in)


def _desc(L):
    d = types.SimpleNamespace(**L._asdict())
    d.in_scale, d.pre_act, d.pre_slope, d.pad_mode, d.x, d.w = 1.0, 0, 0.0, L.reflect, [4096], 4096
    return d


def tile_of(arith, w_layout, variant, L):
    """-> (kernel family, BT, BN): the dispatch of conv1d_f32.hip / conv1d_f32_direct.hip / conv1d_f16.hip / conv1d_split.hip / conv1d_emul.hip for one plain
    input.  Families: "direct" (conv1d_direct.h), "lds" (conv1d_impl.h), "split", "emul", "e16"."""
    maxL = L.max_len * L.len_mul
    n_seq, n = L.n_seq, L.n_out
    wgs128 = ((maxL + 127) // 128) * n_seq * ((n + 127) // 128)
    if arith == "F16":
        return ("lds", 256, 64) if n <= 64 else ("lds", 128, 128)
    if arith == "F32":
        if variant == 0 or variant >= 3:
            d = _desc(L)
            env = dict(d=d, maxL=maxL, n_pad=(n + 31) & ~31, ld=max(L.ldx, L.ldy, L.ldr))
            ok = _ev("conv1d_direct.h", "direct_ok", env)
            if ok and L.snake and (n <= 64 or variant not in (0, 3, 5)):
                ok = False
            if ok and n <= 64:
                if variant in (0, 3):
                    return ("direct", 256, 64)
                ok = False
            if ok:
                if variant == 0:
                    t128, t64 = (maxL + 127) // 128, (maxL + 63) // 64
                    variant = 5 if (t128 * n_seq * ((n + 127) // 128) <= 512 or t64 * 64 * 23 <= t128 * 128 * 20) else 3
                if variant in (3, 4, 5):
                    return ("direct", 64 if variant == 5 else 128, 128)
        if n <= 64:
            return ("lds", 256, 64)
        return ("lds", 64, 128) if variant == 1 or (variant == 0 and wgs128 <= 600) else ("lds", 128, 128)
    if arith == "F32S":
        return ("split", 128, 64) if n <= 64 and L.n_in == 1 else ("split", 128, 128)
    seven = arith == "F32E"
    if L.n_in > 1:                 # summed inputs: one 128 n x 128 t tile in both layouts
        return ("emul" if w_layout == 0 else "e16", 128, 128)
    if w_layout == 0:
        if n <= 64:
            return ("emul", 128, 64)
        if seven:
            small = (L.k_w > 1 and wgs128 <= 128 and (L.k_w - 1) * L.dil <= 32) or L.k_w == 1
        else:
            small = L.k_w == 1 and wgs128 <= 768
        return ("emul", 64, 128) if small else ("emul", 128, 128)
    if n <= 64:
        return ("e16", 64, 64)
    t64 = ((maxL + 63) // 64) * n_seq
    if L.n_split % 384 == 0 and (variant == 6 or (variant == 0 and n % 384 == 0 and t64 * (n // 384) >= 256)):
        return ("e16", 64, 384)
    if variant == 3 or (variant == 0 and n % 256 == 0 and t64 * (n // 256) >= 256):
        return ("e16", 64, 256)
    if variant == 9 or (variant == 0 and t64 * ((n + 127) // 128) <= 256):
        return ("e16", 32, 128)
    if variant == 1 or (variant == 0 and (L.k_w == 1 or wgs128 <= 128)):
        return ("e16", 64, 128)
    return ("e16", 128, 128)


def _frag(fname, d):
    """conv_epilogue / conv_epilogue16: which of its three store forms the launch takes (per quad: the ragged last quad of a vector launch is its tail)."""
    if d.y_transposed:
        return "transposed"
    env = dict(d=d)
    env["vec_r"], env["vec_y"] = _ev(fname, "vec", env, "vec_r"), _ev(fname, "vec", env, "vec_y")
    if _ev(fname, "vec_store", dict(env, full=True)):
        return "vec" if d.n_out % 4 == 0 else "vec+tail"
    return "scalar"


def _one_output(arith, fam, BT, BN, launcher_d, d):
    """The path of one output: `launcher_d` is the descriptor the host launcher saw (it decides f32_tile), `d` the kernel's private copy after
    conv_second_output."""
    sizeof_T = 2 if arith == "F16" else 4
    if fam == "direct":
        return "direct-rowmajor" if _ev("conv1d_direct.h", "rowmajor", dict(d=d)) else "direct-generic-" + _frag("conv1d_impl.h", d)
    if fam == "lds":
        f = "conv1d_impl.h"
        f32_tile = _ev(f, "have_f32_tile_f32" if sizeof_T == 4 else "have_f32_tile_f16", dict(d=launcher_d, BT=BT, BN=BN))
        env = dict(d=d, f32_tile=f32_tile, sizeof_T=sizeof_T)
        env["rowmajor"] = _ev(f, "rowmajor", env)
        if sizeof_T == 2 and _ev(f, "use_f16_tile", env):
            return "lds-f16tile"
        return "lds-f32tile" if _ev(f, "use_f32_tile", env) else "frag-" + _frag(f, d)
    if fam in ("split", "emul"):
        f = f"conv1d_{fam}.h"
        env = dict(d=d, f32_tile=_ev(f, "have_f32_tile", dict(d=launcher_d, BT=BT, BN=BN)))
        env["rowmajor"] = _ev(f, "rowmajor", env)
        return "lds-f32tile" if _ev(f, "use_f32_tile", env) else "frag-" + _frag("conv1d_impl.h", d)
    f = "conv1d_emul16.h"
    direct_epi = _ev(f, "direct_epi", dict(d=launcher_d))
    env = dict(d=d, f32_tile=_ev(f, "have_f32_tile", dict(d=launcher_d, direct_epi=direct_epi, BT=BT, BN=BN)))
    env["rowmajor"] = _ev(f, "rowmajor", env)
    return "e16-lds" if _ev(f, "use_f32_tile", env) else "e16-frag-" + _frag(f, d)


def store_path(arith, w_layout, variant, launch):
    """The epilogue(s) a launch takes.  One output: a name.  Two outputs: "<first>|2nd:<second>" -- the slabs below n_split see n_out = n_split, the slabs at
    or above it the rewritten descriptor of conv_second_output (transposed, ldy2: always the generic fragment-order store)."""
    fam, BT, BN = tile_of(arith, w_layout, variant, launch)
    d0 = _desc(launch)
    if not launch.n_split:
        return _one_output(arith, fam, BT, BN, d0, d0)
    paths = []
    for n_first in (0, launch.n_split):
        d = _desc(launch)
        if _ev("conv1d_impl.h", "second_output", dict(d=d, n_first=n_first)):
            d.y, d.ldy, d.y_transposed = 4096, launch.ldy2, 1          # (y2 shifted by whole rows: its own alignment no longer matters to any predicate)
        else:
            d.n_out = launch.n_split
        paths.append(_one_output(arith, fam, BT, BN, d0, d))
    return f"{paths[0]}|2nd:{paths[1]}"


# The predicate atoms of the selection, for the "flipped alone" proof: name -> value of a launch (None: does not exist for it)
ATOMS = collections.OrderedDict([
    ("y_transposed", lambda L: bool(L.y_transposed)),
    ("n_out % 8 == 0", lambda L: L.n_out % 8 == 0),
    ("n_out % 4 == 0", lambda L: L.n_out % 4 == 0),
    ("y % 16 == 0", lambda L: L.y % 16 == 0),
    ("ldy % 4 == 0", lambda L: L.ldy % 4 == 0),
    ("ldy % 8 == 0", lambda L: L.ldy % 8 == 0),
    ("resid", lambda L: bool(L.resid)),
    ("ldr % 4 == 0", lambda L: L.ldr % 4 == 0 if L.resid else None),
    ("resid % 16 == 0", lambda L: L.resid % 16 == 0 if L.resid else None),
    ("y_is_f32", lambda L: bool(L.y_is_f32)),
    ("n_split > 0", lambda L: L.n_split > 0),
])
# what else may differ between the two launches of a flip, because the atoms are not independent: a transposed output has another leading dimension (the rows),
# a tight row's leading dimension is its n_out, a residual brings its own atoms into existence, and the second of two outputs needs n_out > 256
COUPLED = {
    "y_transposed": {"ldy % 4 == 0", "ldy % 8 == 0"},
    "n_out % 8 == 0": {"ldy % 8 == 0"},
    "n_out % 4 == 0": {"ldy % 4 == 0", "ldy % 8 == 0"},
    "ldy % 4 == 0": {"ldy % 8 == 0"},
    "resid": {"ldr % 4 == 0", "resid % 16 == 0"},
    "n_split > 0": {"n_out % 8 == 0", "n_out % 4 == 0", "ldy % 4 == 0", "ldy % 8 == 0"},
}


def atoms_of(L):
    return {k: f(L) for k, f in ATOMS.items()}


def model_launches():
    """A grid of descriptors around every predicate, for enumerating what store_path CAN return per kernel: every n_out class, base alignment, leading
    dimension class, residual form, transposition, two outputs, f16 / f32 y, SnakeBeta, reflect padding, k 1 / 3, one utterance and many."""
    out = []
    for n in (1, 8, 13, 64, 131, 132, 136, 392):
        for y_off in (0, 8, 16):
            for pad_ld in (0, 1, 2, 4, 24):
                for y32 in (1, 0):
                    for resid, ldr in ((0, 0), (4096, n), (4096 + 8, n + 24), (4096, n + 2), (4096 + 32, n + 24)):
                        for tr in (0, 1):
                            base = Launch(n, (395 if tr else n) + pad_ld, 4096 + y_off, y32, tr, resid, ldr, 0, 0, 0, 0, 3, 1, 64, 6, 200, 1, 64, 1)
                            out += [base, base._replace(reflect=1)]
                            if not y_off and not pad_ld:
                                out += [base._replace(k_w=1), base._replace(n_in=2)]
                                if n % 4 == 0:
                                    out.append(base._replace(snake=1))
                            if n > 256 and not tr and not resid:
                                two = base._replace(n_split=256, ldy=256 + pad_ld, ldy2=440)
                                out += [two, two._replace(n_in=2)]
    return out
