"""The case tables of the alignment-learning kernel tests (csrc/alignment.hip: mas_kernel, align_logp_kernel, align_logp_bwd_frames_kernel,
align_logp_bwd_tokens_kernel; csrc/gaussian_train.hip: gauss_up_fwd_kernel, gauss_up_bwd_kernel): shapes, input generators, CPU references and a
host-side model of each kernel's structure (tiles, tails, LDS), shared by test_alignment_cases_cpu.py (the table reaches every class; no GPU) and
test_alignment_cases_gpu.py (the kernels against the references).  TEST INFRASTRUCTURE ONLY."""
import functools
import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---------------------------------------------------------------- tile constants, mirrored from the kernels (read back from the .hip text by the CPU test)
MAS_SLOTS, MAS_PF, MAS_RED = 4, 8, 4
AL_FB, AL_CC, AL_PAIRS = 16, 64, 32
ALB_TT, ALB_FK = 32, 32
GU_TMAX, GU_FT = 512, 64
GB_TT, GB_NT, GB_FK = 32, 128, 32
CONSTANTS = {"alignment.hip": dict(MAS_SLOTS=MAS_SLOTS, MAS_PF=MAS_PF, MAS_RED=MAS_RED, AL_FB=AL_FB, AL_CC=AL_CC, AL_PAIRS=AL_PAIRS, ALB_TT=ALB_TT,
                                   ALB_FK=ALB_FK),
             "gaussian_train.hip": dict(GU_TMAX=GU_TMAX, GU_FT=GU_FT, GB_TT=GB_TT, GB_NT=GB_NT, GB_FK=GB_FK)}
LDS_BYTES = 160 * 1024                      # LDS of one CU
MAS_LDS_MAX = LDS_BYTES - MAS_RED * 8       # mas_kernel keeps MAS_RED float64 partials in static LDS: the dynamic part may use the rest
U = 2.0 ** -24                              # unit roundoff of float32
FACTOR = 4.0                                # the project's yardstick factor for the f32 kernels (profiles/r11_notes.md)


def hip_constants(fname):
    """{NAME: value} of every `constexpr int NAME = <integer>` in jatts_amd/csrc/<fname>."""
    with open(os.path.join(ROOT, "jatts_amd", "csrc", fname)) as f:
        return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (\w+) = (\d+);", f.read())}


def ceil_div(a, b):
    return -(-a // b)


def round_up(v, m):
    return ceil_div(v, m) * m


def mas_lds(t_mel, t_inp):
    """Dynamic LDS of mas_kernel as jatts_mas_viterbi prices it: decision words, two Q columns, counts, path, 16 bytes of slack."""
    return t_mel * ceil_div(t_inp, 64) * 8 + 2 * (t_inp + 1) * 8 + t_inp * 4 + t_mel * 4 + 16


def align_lds(t_text):
    """Dynamic LDS of align_logp_kernel / align_logp_bwd_frames_kernel: token tile, frame tile, AL_FB x T scores."""
    return (t_text * (AL_CC + 1) + AL_FB * (AL_CC + 1) + AL_FB * t_text) * 4


# ================================================================ MAS
# (T_mel, T_inp).  Two shapes of the issue's list, (1100, 1023) and (1100, 1024), cannot be launched: mas_lds gives 165 692 and 165 712 bytes, above
# the 163 808 the kernel may use, and jatts_mas_viterbi refuses them (the CPU test asserts that).  The classes they were listed for -- 16 decision
# words, all four token slots, 1023 / 1024 tokens -- are reached at T_mel = 1085, the largest frame count 1024 tokens admit.
MAS_REFUSED = [(1100, 1023), (1100, 1024)]
MAS_SHAPES = [(1, 1), (2, 1), (1, 2), (8, 9), (9, 9), (10, 9), (17, 16),
              (64, 63), (64, 64), (64, 65), (66, 65),
              (300, 255), (300, 256), (300, 257),
              (600, 511), (600, 513),
              (1085, 1023), (1085, 1024)] + [(t, 5) for t in (2, 8, 9, 10, 16, 17, 18)]      # the last seven: the prefetch ring
MAS_KINDS = ("q4", "half", "const", "rand")
MAS_EXACT = MAS_KINDS[:3]                   # integer codes: every partial sum is exact in f32 and f64, in any order
MAS_SCALE = {"q4": 1.0, "half": 0.5, "const": 1.0}
MAS_FIXTURE_SHAPES = [s for s in MAS_SHAPES if s[1] <= 257]      # "up to (300, 257)": what tests/golden/mas_ties.npz holds
MAS_LIMIT_SHAPES = [(4407, 256), (1085, 1024)]                    # 163 804 and 163 732 bytes: the largest that run


def mas_decode(kind, codes):
    """int8 codes -> f32 log-probabilities: q4 -(0..3), half -0.5 x (0..15), const -2."""
    return (-MAS_SCALE[kind] * codes.astype(np.float32)).astype(np.float32)


def mas_q(lp):
    """The float64 Q table (T_inp, T_mel) of the search, row 0 as a running float64 sum (what mas_kernel and the oracle's default form do)."""
    lp = np.asarray(lp).T.astype(np.float64)
    t_inp, t_mel = lp.shape
    q = np.full((t_inp, t_mel), -np.inf)
    q[0] = np.cumsum(lp[0])
    for j in range(1, t_mel):
        hi = min(j + 1, t_inp)
        if hi > 1:
            q[1:hi, j] = np.maximum(q[0:hi - 1, j - 1], q[1:hi, j - 1]) + lp[1:hi, j]
    return q


def mas_backtrack(q, strict=False):
    """(path, finite ties met on it).  strict=True is the WRONG rule (`>` in place of the reference's `>=`): the mutation the tie inputs are there to catch."""
    t_inp, t_mel = q.shape
    a = np.full((t_mel,), t_inp - 1, dtype=np.int64)
    ties = 0
    for j in range(t_mel - 2, -1, -1):
        i = a[j + 1]
        if i == 0:
            a[j] = 0
            continue
        up, stay = q[i - 1, j], q[i, j]
        ties += int(up == stay and np.isfinite(up))
        a[j] = i - 1 if (up > stay if strict else up >= stay) else i
    return a, ties


def _mas_codes(kind, tm, ti, attempt):
    rng = np.random.default_rng([MAS_KINDS.index(kind), tm, ti, attempt])
    if kind == "const":
        return np.full((tm, ti), 2, dtype=np.int8)
    if kind == "q4":
        return rng.integers(0, 4, size=(tm, ti)).astype(np.int8)
    p = 0.6 ** np.arange(16)      # half: all of 0..15, small codes more often (the stored codes then deflate to 3 bits each: the fixture's size limit)
    return rng.choice(16, size=(tm, ti), p=p / p.sum()).astype(np.int8)


@functools.lru_cache(maxsize=None)
def mas_input(kind, tm, ti):
    """(codes int8 or None, log_p f32 (T_mel, T_inp)).  For q4 / half with slack (T_mel > T_inp >= 2) the generator's stream is advanced until the
    optimal path meets a finite tie, so that the tie rule decides at least one frame of every such case (most meet dozens on the first draw)."""
    if kind == "rand":
        z = np.random.default_rng([3, tm, ti]).standard_normal((tm, ti)).astype(np.float32) * 2.0
        return None, (z - np.log(np.exp(z).sum(1, keepdims=True))).astype(np.float32)
    for attempt in range(64):
        codes = _mas_codes(kind, tm, ti, attempt)
        solved = _solve(mas_decode(kind, codes))
        if kind == "const" or not (tm > ti >= 2) or solved[1] > 0:
            _SOLVED[kind, tm, ti] = solved
            return codes, mas_decode(kind, codes)
    raise AssertionError(("no tie on the optimal path", kind, tm, ti))


_SOLVED = {}


def _solve(lp):
    q = mas_q(lp)
    path, ties = mas_backtrack(q)
    return path, ties, mas_backtrack(q, strict=True)[0]


def mas_solved(kind, tm, ti):
    """(path, finite ties on it, the path of the WRONG `>` rule) of mas_input(kind, tm, ti) by the model above; computed once, shared by the tests."""
    lp = mas_input(kind, tm, ti)[1]
    if (kind, tm, ti) not in _SOLVED:
        _SOLVED[kind, tm, ti] = _solve(lp)
    return _SOLVED[kind, tm, ti]


def mas_fixture():
    """tests/golden/mas_ties.npz -> {(kind, T_mel, T_inp): (codes int8 (T_mel, T_inp), path int64 (T_mel,))}: the real reference function's paths."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "mas_ties.npz"))
    out = {}
    for kind in MAS_EXACT:
        codes, paths, oc, op = z[kind + "_codes"], z[kind + "_paths"], 0, 0
        for tm, ti in z["shapes"].tolist():
            out[kind, tm, ti] = (codes[oc:oc + tm * ti].reshape(tm, ti), paths[op:op + tm])
            oc, op = oc + tm * ti, op + tm
        assert oc == codes.size and op == paths.size
    return out


def mas_launches(shapes, limit=MAS_LDS_MAX, most=9):
    """The shapes in table order, split into ragged launches of at most `most` sequences whose batch maxima (what the launcher prices) fit the LDS limit."""
    out, cur = [], []
    for s in shapes:
        trial = cur + [s]
        if cur and (len(cur) == most or mas_lds(max(t for t, _ in trial), max(i for _, i in trial)) > limit):
            out.append(cur)
            cur = [s]
        else:
            cur = trial
    return out + [cur]


def mas_class(tm, ti):
    return dict(W=ceil_div(ti, 64), slots=ceil_div(ti, 256), mel_mod8=tm % MAS_PF, order="<" if tm < ti else "==" if tm == ti else ">",
                ring_rounds=ceil_div(tm - 1, MAS_PF), lds=mas_lds(tm, ti))


# ================================================================ alignment log-probabilities
# name: (frame lengths, token lengths, adim)
ALIGN_BATCHES = {"A": ([17, 0, 1, 16, 33], [33, 5, 1, 64, 65], 65),
                 "B": ([15, 2], [492, 31], 63),
                 "C": ([33], [130], 384),
                 "D": ([16, 17], [32, 63], 1),
                 "E": ([31], [63], 64),
                 "F": ([32, 1], [64, 32], 129)}


class AlignCase:
    """One launch of the forward / backward pair.  Rows are packed ragged: feats (sum frames, adim), text (sum tokens, adim), log_p / dlog_p
    (sum frames, ld / ld_g).  masked: {utterance: [columns set to -inf in the saved log_p]}; coincident: (utterance, frame, token) made equal rows."""

    def __init__(self, name, flens, tlens, adim, ld=None, masked=None, coincident=None, seed=0):
        self.name, self.flens, self.tlens, self.adim = name, list(flens), list(tlens), adim
        self.ld = ld if ld is not None else round_up(max(tlens), 8)
        self.masked, self.coincident, self.seed = masked or {}, coincident, seed

    def __repr__(self):
        return self.name

    @functools.cached_property
    def data(self):
        """(feats, text, dlog_p): dlog_p has finite garbage at every column >= the utterance's token count."""
        gen = torch.Generator().manual_seed(3100 + self.seed)
        nf, nt = sum(self.flens), sum(self.tlens)
        feats, text = torch.randn(nf, self.adim, generator=gen), torch.randn(nt, self.adim, generator=gen)
        if self.coincident:
            b, f, j = self.coincident
            text[sum(self.tlens[:b]) + j] = feats[sum(self.flens[:b]) + f]
        dlp = torch.randn(nf, self.ld, generator=gen)
        o = 0
        for fl, tl in zip(self.flens, self.tlens):
            dlp[o:o + fl, tl:] = 1e3 * (1.0 + torch.rand(fl, self.ld - tl, generator=gen))
            o += fl
        return feats, text, dlp

    def utterances(self):
        """(b, frame row slice, token row slice)."""
        fo = to = 0
        for b, (fl, tl) in enumerate(zip(self.flens, self.tlens)):
            yield b, slice(fo, fo + fl), slice(to, to + tl)
            fo, to = fo + fl, to + tl

    def _eval(self, dtype):
        """(log_p rows, dist rows, d_feats, d_text) in `dtype` on the CPU by autograd, one utterance at a time: log_softmax_j(-||f_i - t_j||_2) with the
        masked columns filled with -inf before the softmax, and plain `backward(dlog_p)` of that: masked_fill passes nothing back to a masked column,
        while its dlog_p (randn here, like any other column's) still counts in the log-softmax backward's sum_j g.  Only the padding's dlog_p (columns
        >= T_t, which the utterance's expression does not have) is left out."""
        feats, text, dlp = self.data
        lps, dists = [], []
        dF, dT = torch.zeros(feats.shape, dtype=dtype), torch.zeros(text.shape, dtype=dtype)
        for b, fs, ts in self.utterances():
            tl = self.tlens[b]
            f, t = feats[fs].to(dtype).clone().requires_grad_(True), text[ts].to(dtype).clone().requires_grad_(True)
            dist = torch.norm(f.unsqueeze(1) - t.unsqueeze(0), p=2, dim=2)
            mask = torch.zeros(tl, dtype=torch.bool)
            mask[self.masked.get(b, [])] = True
            lp = torch.log_softmax((-dist).masked_fill(mask.unsqueeze(0), float("-inf")), dim=-1)
            if fs.stop > fs.start:
                lp.backward(dlp[fs, :tl].to(dtype))
                dF[fs], dT[ts] = f.grad, t.grad
            lps.append(lp.detach())
            dists.append(dist.detach())
        return lps, dists, dF, dT

    @functools.cached_property
    def ref(self):
        return self._eval(torch.float64)

    @functools.cached_property
    def ref32(self):
        return self._eval(torch.float32)

    def fwd_bound(self, b):
        """Per element of utterance b (frames, tokens): the forward sums adim squares in ONE f32 chain, so |d score_j| <= (adim + 3) / 2 u dist_ij, and
        |d log_p_ij| <= 2 max_j |d score_j| + 4 u max(1, |log_p_ij|) (the log-sum-exp moves by at most the largest score error; expf, logf and the
        final subtraction round at the size of the result)."""
        lp, dist = self.ref[0][b], self.ref[1][b]
        ds = (self.adim + 3) / 2 * U * dist
        return 2 * ds.max(dim=1, keepdim=True).values + 4 * U * lp.abs().clamp_min(1.0)

    def classes(self):
        a, tm = self.adim, max(self.tlens)
        return dict(chunks=ceil_div(a, AL_CC), chunk_tail=a % AL_CC, nf=sorted({fl - AL_FB * ((fl - 1) // AL_FB) for fl in self.flens if fl} |
                                                                                 {AL_FB for fl in self.flens if fl > AL_FB}),
                    lane_strides=sorted({ceil_div(t, 64) for t in self.tlens}), lds=align_lds(tm), fill=self.ld - min(self.tlens),
                    token_tiles=sorted({ceil_div(t, ALB_TT) for t in self.tlens}), token_tail=sorted({t % ALB_TT for t in self.tlens}),
                    frame_chunk_tail=sorted({fl % ALB_FK for fl in self.flens if fl}), zero_frames=0 in self.flens)


ALIGN_FWD_CASES = [AlignCase(k, *v, seed=i) for i, (k, v) in enumerate(ALIGN_BATCHES.items())]
ALIGN_BWD_CASES = ALIGN_FWD_CASES + [
    AlignCase("train", [40] * 3, [17, 5, 1], 12, ld=17, seed=10),                                    # odd ld = ld_g, as autograd.AlignLogProb saves it
    AlignCase("masked", [17, 20], [33, 9], 65, masked={0: [5, 31], 1: [3, 4]}, seed=11),             # two interior valid columns at -inf
    AlignCase("coincident", [17, 3], [33, 5], 65, coincident=(0, 16, 32), seed=12),                  # d^2 = 0: the 1e-24 guard
]


# ================================================================ Gaussian upsampling
# name: (kv, kvo, Tm, To, C).  A..G are the issue's; H adds the one channel class its list names and its table lacks (C = 32: exactly one fragment).
GAUSS_BATCHES = {"A": ([1, 2, 3, 0], [5, 1, 0, 4], 3, 5, 1),
                 "B": ([17, 16, 15], [31, 32, 33], 17, 33, 20),
                 "C": ([63, 64, 65], [63, 64, 65], 65, 65, 33),
                 "D": ([512, 500], [65, 10], 512, 65, 31),
                 "E": ([33], [130], 33, 130, 129),
                 "F": ([9, 4], [40, 64], 9, 64, 384),
                 "G": ([8, 8], [32, 32], 8, 32, 128),
                 "H": ([5], [7], 5, 7, 32)}
GAUSS_DELTA = 0.1


class GaussCase:
    def __init__(self, name, kv, kvo, Tm, To, C, seed=0, identity=False):
        self.name, self.kv, self.kvo, self.Tm, self.To, self.C, self.seed, self.identity = name, list(kv), list(kvo), Tm, To, C, seed, identity
        assert Tm == max(kv) and To == max(kvo)

    def __repr__(self):
        return self.name

    @functools.cached_property
    def data(self):
        """(hs (B, Tm, C), ds (B, Tm), g (B, To, C)).  Durations: integers 0..6, zero past kv; token 0 of every utterance has duration 0; utterance 1
        (or 0) does not sum to its frames; batch A's utterance 2 is all zeros; batch F's utterance 1 has 30 frames a token (energies far below -60)."""
        gen = torch.Generator().manual_seed(3200 + self.seed)
        B = len(self.kv)
        hs, g = torch.randn(B, self.Tm, self.C, generator=gen), torch.randn(B, self.To, self.C, generator=gen)
        ds = torch.randint(0, 7, (B, self.Tm), generator=gen).float()
        for b, n in enumerate(self.kv):
            ds[b, n:] = 0.0
            ds[b, 0] = 0.0
        b = min(1, B - 1)
        if self.kv[b] > 1 and float(ds[b].sum()) == self.kvo[b]:
            ds[b, 1] += 1.0
        if self.name == "A":
            ds[2] = 0.0
        if self.name == "F":
            ds[1, :self.kv[1]] = 30.0
        if self.identity:       # hs = the identity on the first Tm channels, g on the first To: out and d_hs ARE the two kernels' weights
            hs, g = torch.zeros_like(hs), torch.zeros_like(g)
            hs[:, torch.arange(self.Tm), torch.arange(self.Tm)] = 1.0
            g[:, torch.arange(self.To), torch.arange(self.To)] = 1.0
        return hs, ds, g

    def _eval(self, dtype):
        """(out (B, To, C), d_hs (B, Tm, C)) in `dtype` on the CPU by autograd: the expression of tests/test_mas_train_ops_gpu.py::_gauss_expr, one
        utterance at a time so that an utterance without tokens (softmax over nothing) gives zero rows instead of NaN."""
        hs, ds, g = self.data
        out, dhs = torch.zeros(g.shape, dtype=dtype), torch.zeros(hs.shape, dtype=dtype)
        for b, (n, no) in enumerate(zip(self.kv, self.kvo)):
            if n == 0:
                continue
            h = hs[b, :n].to(dtype).clone().requires_grad_(True)
            d = ds[b, :n].to(dtype)
            tpos = torch.arange(self.To).to(dtype) * (torch.arange(self.To) < no).to(dtype)      # padded frames sit at t = 0
            cen = d.cumsum(-1) - d / 2
            p = torch.softmax(-GAUSS_DELTA * (tpos.unsqueeze(-1) - cen.unsqueeze(0)) ** 2, dim=1)
            o = torch.matmul(p, h)
            o.backward(g[b].to(dtype))
            out[b], dhs[b, :n] = o.detach(), h.grad
        return out, dhs

    @functools.cached_property
    def ref(self):
        return self._eval(torch.float64)

    @functools.cached_property
    def ref32(self):
        return self._eval(torch.float32)

    def classes(self):
        k2 = [(n + 1) & ~1 for n in self.kv]
        return dict(kv_parity=sorted({n % 2 for n in self.kv}), k2_mod16=sorted({k % 16 for k in k2}), frame_tail=sorted({n % GU_FT for n in self.kvo}),
                    store_tail=self.To % GU_FT, bwd_chunk_tail=self.To % GB_FK,
                    padded_tiles=sum(1 for n in self.kv for j0 in range(0, self.Tm, GB_TT) if j0 >= n),
                    partial_tiles=sum(1 for n in self.kv if n % GB_TT), wave_passes=ceil_div(self.C, GB_NT), C=self.C,
                    kv0=0 in self.kv, kvo0=0 in self.kvo, Tm=self.Tm)


GAUSS_CASES = [GaussCase(k, *v, seed=i) for i, (k, v) in enumerate(GAUSS_BATCHES.items())]
GAUSS_IDENTITY = [GaussCase(k + "-identity", *GAUSS_BATCHES[k][:4], 65, seed=20 + i, identity=True) for i, k in enumerate("BC")]


def held(name, got, ref, f32):
    """The project's yardstick: max|got - ref| <= FACTOR x the f32 CPU evaluation's, plus 4 u max|ref| so that an output the f32 evaluation gets
    exactly (T_t = 1: all zeros) does not ask for more than f32 can give.  Prints the figures before it asserts."""
    ref = ref.double()
    e = float((got.double().cpu() - ref).abs().max()) if ref.numel() else 0.0
    e32 = float((f32.double() - ref).abs().max()) if ref.numel() else 0.0
    floor = 4 * U * (float(ref.abs().max()) if ref.numel() else 0.0)
    print(f"{name}: max|err| {e:.3e}, f32 CPU {e32:.3e}, ratio {e / max(e32, 1e-300):.2f}, floor {floor:.1e}")
    assert bool(torch.isfinite(got).all()), name
    assert e <= FACTOR * e32 + floor, (name, e, e32, floor)
