"""Case tables and CPU references of tests/test_conv_geometry_{cpu,gpu}.py: the free geometry of jatts_conv1d / jatts_conv1d_wgrad
(pad, even k_w, dil, rg.len_mul, up to three summed inputs with in_scale and the LeakyReLU prologue, f32 / f16 stores) on small INTEGERS.

Every staged operand (in_scale * sum_i x_i, after the LeakyReLU prologue) is an integer with |u| <= 8, every weight an integer with
|w| <= 4, the bias an integer: every product and every partial sum is an integer below 2**24.  Such values are exact in f16 (operands
below 2048), in three bf16 terms (one term holds 8 bits), in split f16 hi / lo planes under a power-of-two scale and in every f32
accumulator, in any summation order, with or without FMA -- so the float64 (= int64) result of the definition

    y[t, n] = act( b[n] + sum_{tap, c} W[n, c, tap] * u[t + tap * dil - pad, c] ),     rows outside the utterance read as zero

is the expected output to the last bit in EVERY arithmetic; an f16 store rounds that exact value once (and the tables keep |y| < 2048, where
it does not round at all).  tests/test_conv_geometry_cpu.py proves the preconditions from the generated inputs.

Pure data and CPU functions: nothing here touches the GPU or the library (profiles/r12_notes.md lists kernel -> case -> path)."""
import collections
import functools
import zlib

import torch
import torch.nn.functional as F

F24 = 2 ** 24
F16_EXACT = 2048            # integers up to here are f16 numbers

# (k, dil, pad), 0 <= pad <= (k - 1) dil.  Left halo = pad, right halo = (k - 1) dil - pad.
GEOMS = [
    (2, 1, 1),    # Matcha's folded stride-2 down-conv: even width, no right halo
    (2, 1, 0),    # its mirror image: no left halo
    (4, 1, 2),    # Matcha's training up-conv: left 2, right 1
    (4, 1, 1),    # its data gradient: pad' = (k - 1) dil - pad
    (3, 1, 0),    # causal-in-reverse: right halo only
    (3, 1, 2),    # causal: left halo only
    (5, 2, 0),
    (5, 2, 8),
    (5, 2, 3),    # an offset that is no multiple of the dilation
    (7, 3, 5),    # halo 18: longer than the short sequences
    (3, 1, 1),    # the symmetric control
]
GEOM_IDS = [f"k{k}d{d}p{p}" for k, d, p in GEOMS]


def halo(geom):
    k, dil, _ = geom
    return (k - 1) * dil


# One launch configuration: channel shape (each n_out under another tile rule: 32 <= the 64-wide tile, 72 a multiple of 8 but not of 32, 160 and 288
# no multiple of 128), summed inputs, in_scale, LeakyReLU slope, epilogue activation, len_mul, a per-input x_col0 window of a wider row, an
# (out_ld, out_col0) window of a wider NaN-prefilled output, the tile width whose +-1 lengths the batch holds, and its one long sequence.
Config = collections.namedtuple("Config", "name c_in n_out n_in in_scale slope act len_mul x_window out_window tile long")
CONFIGS = [
    Config("plain",   64,  32, 1, 1.0,  None, None,   1, False, None,     32, 300),
    Config("window",  192, 160, 1, 1.0,  None, "relu", 1, True,  (184, 8), 128, 300),     # out_ld = n_out + 24, 16-byte aligned window
    Config("up2",     192, 288, 1, 1.0,  0.5,  None,   2, False, None,     64, 200),     # HiFi-GAN's second upsampling conv: prologue + len_mul
    Config("up8mrf3", 64,  72, 3, 0.25, 0.25, None,   8, True,  None,     32, 120),     # ... fed by an unfused MRF sum of three streams
    Config("mrf2",    192, 72, 2, 0.5,  0.5,  "relu", 2, False, (84, 4),  64, 200),     # out window on an 8-byte boundary only: the fragment-order stores
    Config("scaled",  64,  288, 1, 0.5,  None, None,   1, True,  (296, 8), 128, 300),    # one input, but in_scale != 1: no register-streamed kernel
]
CONFIG_IDS = [c.name for c in CONFIGS]


def lens_of(geom, cfg):
    """Base lengths of a case: 1, 2, one below the halo, the config's tile width - 1 / + 0 / + 1 and one long sequence, short ones between long
    ones so that every halo has a neighbouring utterance to read from by mistake."""
    below = max(halo(geom) - 1, 1)
    t = cfg.tile
    return [cfg.long, 1, t + 1, 2, t, below, t - 1]


def _one_thread(fn):
    """The references are many small float64 convs: on one thread they take a tenth of the time the intra-op pool's fork / join costs them."""
    @functools.wraps(fn)
    def run(*a, **kw):
        n = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            return fn(*a, **kw)
        finally:
            torch.set_num_threads(n)
    return run


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))       # (the same inputs in every process, whatever PYTHONHASHSEED is)


def int_operand(shape, cfg, g):
    """-> (xs, u): cfg.n_in integer-valued f32 inputs and the staged operand u = lrelu(in_scale * sum(xs)) they give, an integer with |u| <= 8.
    v = in_scale * sum is drawn first (negative values snapped to multiples of 1 / slope so that the prologue keeps them integers), then the sum
    v / in_scale is dealt out over the inputs."""
    v = torch.randint(-8, 9, shape, generator=g)
    if cfg.slope is not None:
        m = int(round(1.0 / cfg.slope))
        v = torch.where(v < 0, -((-v) // m) * m, v)
    total = v * int(round(1.0 / cfg.in_scale))
    xs = [torch.randint(-8, 9, shape, generator=g) for _ in range(cfg.n_in - 1)]
    xs.append(total - sum(xs) if xs else total)
    u = torch.where(v < 0, v.double() * (cfg.slope if cfg.slope is not None else 1.0), v.double())
    return [x.float() for x in xs], u


def int_weight(n_out, c_in, k, g, density=0.5):
    """Integer weights |w| <= 4, about half of them zero (keeps |y| below 2048 for the f16 stores), and an integer bias |b| <= 8."""
    w = torch.randint(-4, 5, (n_out, c_in, k), generator=g) * (torch.rand(n_out, c_in, k, generator=g) < density)
    return w.float(), torch.randint(-8, 9, (n_out,), generator=g).float()


# ------------------------------------------------------------------------------------------ references, written from the definition
@_one_thread
def reference_conv(u, w, b, lens, k, dil, pad, act=None, fault=None, tile=32):
    """Stride-1 conv of the staged operand u (rows, c_in), one utterance at a time, float64: explicit F.pad(left = pad, right = (k - 1) dil - pad)
    then F.conv1d.  `lens` are ROW counts (base length x len_mul).  `fault` builds a deliberately wrong geometry for the sensitivity tests:
    "pad_off_by_one" shifts the window by one row, "no_right_halo" lets a `tile`-row time tile read zeros beyond its own last row,
    "cross_utterance" lets the halo read the neighbouring utterances instead of zeros."""
    u, w = u.double(), w.double()
    b = None if b is None else b.double()
    right = (k - 1) * dil - pad
    if fault == "pad_off_by_one":
        pad, right = (pad + 1, right - 1) if right > 0 else (pad - 1, right + 1)
    if fault == "cross_utterance":
        y = F.conv1d(F.pad(u.t().unsqueeze(0), (pad, right)), w, b, dilation=dil)[0].t()
    else:
        outs, o = [], 0
        for L in lens:
            xs = u[o:o + L].t().unsqueeze(0)
            if fault == "no_right_halo":
                rows = []
                for t0 in range(0, L, tile):
                    cut = xs.clone()
                    cut[..., t0 + tile:] = 0
                    rows.append(F.conv1d(F.pad(cut, (pad, right)), w, b, dilation=dil)[0].t()[t0:t0 + tile])
                outs.append(torch.cat(rows))
            else:
                outs.append(F.conv1d(F.pad(xs, (pad, right)), w, b, dilation=dil)[0].t())
            o += L
        y = torch.cat(outs)
    return torch.relu(y) if act == "relu" else y


@_one_thread
def reference_wgrad(x, dy, lens, k, dil, pad):
    """dw[n, c, tap] = sum_t dy[t, n] x[t + tap dil - pad, c] and db[n] = sum_t dy[t, n], per utterance, float64, from the definition."""
    x, dy = x.double(), dy.double()
    dw = torch.zeros(dy.shape[1], x.shape[1], k, dtype=torch.float64)
    o = 0
    for L in lens:
        xp = F.pad(x[o:o + L].t(), (pad, (k - 1) * dil - pad))            # (c, L + halo)
        for tap in range(k):
            dw[:, :, tap] += dy[o:o + L].t() @ xp[:, tap * dil:tap * dil + L].t()
        o += L
    return dw, dy.sum(0)


def fold_stride2(wd):
    """Conv1d(C, C, 3, stride 2, padding 1) weight -> the k_w = 2, pad = 1 conv over PAIR rows [x[2j] | x[2j + 1]] (2 C channels) that computes it:
    tap 0 reads pair j - 1, whose second half is x[2j - 1]; tap 1 reads pair j.  The fold the Matcha decoder prepares its down-conv with."""
    C = wd.shape[0]
    w2 = torch.zeros(C, 2 * wd.shape[1], 2, dtype=wd.dtype)
    w2[:, wd.shape[1]:, 0] = wd[:, :, 0]
    w2[:, :wd.shape[1], 1] = wd[:, :, 1]
    w2[:, wd.shape[1]:, 1] = wd[:, :, 2]
    return w2


@_one_thread
def reference_stride2(x, wd, b, pair_lens):
    """The strided conv itself on the unfolded signal: x (2 * sum(pair_lens), C) -> (sum(pair_lens), C), float64."""
    outs, o = [], 0
    for P in pair_lens:
        outs.append(F.conv1d(x[o:o + 2 * P].double().t().unsqueeze(0), wd.double(), b.double(), stride=2, padding=1)[0].t())
        o += 2 * P
    return torch.cat(outs)


STRIDE2_CHANNELS = (64, 96, 128)                 # C0: the folded conv reads 2 C0 = 128 / 192 / 256 channels (256: the f16 kernel's 128-channel chunks)
STRIDE2_PAIR_LENS = [150, 1, 33, 2, 32, 31]      # lengths in PAIR rows (the signal is twice as long)


@functools.lru_cache(maxsize=None)
@_one_thread
def stride2_case(C0):
    g = _gen("stride2", C0)
    x = torch.randint(-8, 9, (2 * sum(STRIDE2_PAIR_LENS), C0), generator=g).float()
    wd, b = int_weight(C0, C0, 3, g)
    return collections.namedtuple("Stride2Case", "x wd b ref")(x, wd, b, reference_stride2(x, wd, b, STRIDE2_PAIR_LENS))


POLYPHASE = [(8, 16), (5, 10), (4, 8), (3, 6), (2, 4)]                        # (stride, kernel) of the HiFi-GAN / Matcha transposed convs
POLY_CHAINS = [(POLYPHASE[i], POLYPHASE[(i + 1) % 5]) for i in range(5)]      # two stages: every pair comes first once and second (len_mul = s1) once
POLY_CHAIN_IDS = [f"s{a[0]}K{a[1]}-s{b[0]}K{b[1]}" for a, b in POLY_CHAINS]
POLY_LENS = [33, 1, 20, 2]
POLY_CHANNELS = (64, 64, 32)                                                   # c0 -> c1 (feeds a conv: a multiple of 64) -> c2


def poly_padding(s):
    return s // 2 + s % 2


@_one_thread
def reference_polyphase(x, stages, lens):
    """conv_transpose1d(stride = s, padding = s // 2 + s % 2, output_padding = s % 2) stage after stage, one utterance at a time, float64.
    stages: [(w (c_in, c_out, K), bias (c_out), s)].  -> (sum(lens) * prod(s), c_last) time-major rows."""
    outs, o = [], 0
    for L in lens:
        h = x[o:o + L].double().t().unsqueeze(0)
        for w, b, s in stages:
            h = F.conv_transpose1d(h, w.double(), b.double(), stride=s, padding=poly_padding(s), output_padding=s % 2)
        outs.append(h[0].t())
        o += L
    return torch.cat(outs)


@functools.lru_cache(maxsize=None)
@_one_thread
def poly_case(chain_index):
    """Integer inputs of one two-stage chain: x |.| <= 8, sparse stage weights |.| <= 1 / <= 2 (a polyphase group has K / s = 2 real taps: the
    stage-1 output and the result stay below 2048, exact f16 operands / stores), integer biases."""
    (s1, K1), (s2, K2) = POLY_CHAINS[chain_index]
    g = _gen("poly", chain_index)
    c0, c1, c2 = POLY_CHANNELS
    x = torch.randint(-8, 9, (sum(POLY_LENS), c0), generator=g).float()
    w1 = (torch.randint(-1, 2, (c0, c1, K1), generator=g) * (torch.rand(c0, c1, K1, generator=g) < 0.5)).float()
    w2 = (torch.randint(-2, 3, (c1, c2, K2), generator=g) * (torch.rand(c1, c2, K2, generator=g) < 0.25)).float()
    b1, b2 = torch.randint(-8, 9, (c1,), generator=g).float(), torch.randint(-8, 9, (c2,), generator=g).float()
    stages = [(w1, b1, s1), (w2, b2, s2)]
    mid = reference_polyphase(x, stages[:1], POLY_LENS)
    return collections.namedtuple("PolyCase", "x stages mid ref")(x, stages, mid, reference_polyphase(x, stages, POLY_LENS))


# ------------------------------------------------------------------------------------------ the forward table
ForwardCase = collections.namedtuple("ForwardCase", "geom cfg lens row_lens xs u w b ref")


@functools.lru_cache(maxsize=None)
@_one_thread
def forward_case(gi, ci):
    """Inputs and the expected output (float64 holding integers) of geometry GEOMS[gi] under CONFIGS[ci]; computed once per process."""
    geom, cfg = GEOMS[gi], CONFIGS[ci]
    k, dil, pad = geom
    lens = lens_of(geom, cfg)
    row_lens = [v * cfg.len_mul for v in lens]
    g = _gen("fwd", gi, ci)
    xs, u = int_operand((sum(row_lens), cfg.c_in), cfg, g)
    w, b = int_weight(cfg.n_out, cfg.c_in, k, g)
    return ForwardCase(geom, cfg, lens, row_lens, xs, u, w, b, reference_conv(u, w, b, row_lens, k, dil, pad, cfg.act))


def abs_bound(case):
    """max |u| * max_n sum_{c, tap} |w[n, c, tap]| + max |b|: what no partial sum of any output of the case can exceed, in any order."""
    return float(case.u.abs().max()) * float(case.w.abs().sum((1, 2)).max()) + float(case.b.abs().max())


# ------------------------------------------------------------------------------------------ the comparison the GPU tests use
def check_exact(y, want, what=""):
    """`y` (a kernel's output, any float dtype, any device) equals the integer-valued float64 reference `want` bit for bit after ONE rounding of
    the exact value to y's dtype (none at all below 2**24 in f32 and below 2048 in f16); non-finite outputs never pass.  Raises AssertionError naming
    the first wrong rows."""
    y = y.detach().cpu()
    assert tuple(y.shape) == tuple(want.shape), f"{what}: shape {tuple(y.shape)} != {tuple(want.shape)}"
    exp = want.to(y.dtype)
    bad = (y != exp) | ~torch.isfinite(y)
    if bool(bad.any()):
        rows = bad.view(bad.shape[0], -1).any(1).nonzero().view(-1).tolist()
        d = float((y.double() - want)[bad].abs().max())
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ from the integer reference (max |d| = {d:g}) in {len(rows)} "
                             f"rows, first {rows[:8]}")


# backward / weight-gradient tables
BACKWARD_GEOMS = [(4, 1, 2), (2, 1, 1), (3, 1, 0), (5, 2, 8), (7, 3, 5),
                  (3, 17, 17), (5, 9, 4)]      # halo 34 / 36: beyond the split and emulated kernels' 32 rows (hip.conv_halo_fits)
WGRAD_GEOMS = [(1, 1, 0), (3, 1, 0), (3, 1, 2), (5, 2, 8), (5, 2, 3),      # the MFMA path (k 1 / 3 / 5)
               (2, 1, 1), (2, 1, 0), (4, 1, 2), (7, 3, 5)]                   # the VALU path
WGRAD_SHAPES = [(64, 72), (192, 160)]                                        # (c_in, n_out)


def wgrad_lens(geom, len_mul):
    below = max(halo(geom) - 1, 1)
    return [150, 1, 33, 2, 32, below, 31] if len_mul == 1 else [40, 1, 9, 2, 8, below, 7]


@functools.lru_cache(maxsize=None)
@_one_thread
def wgrad_case(gi, si, len_mul):
    geom = WGRAD_GEOMS[gi]
    k, dil, pad = geom
    c_in, n_out = WGRAD_SHAPES[si]
    lens = wgrad_lens(geom, len_mul)
    row_lens = [v * len_mul for v in lens]
    g = _gen("wgrad", gi, si, len_mul)
    x = torch.randint(-8, 9, (sum(row_lens), c_in), generator=g).float()
    dy = torch.randint(-4, 5, (sum(row_lens), n_out), generator=g).float()
    dw, db = reference_wgrad(x, dy, row_lens, k, dil, pad)
    return collections.namedtuple("WgradCase", "geom lens row_lens x dy dw db")(geom, lens, row_lens, x, dy, dw, db)
