"""Case table of tests/test_attention_cases_{cpu,gpu}.py: jatts_relpos_attention (csrc/attention.hip) at every instantiation, tile schedule,
V^T load path, bias form, mask and edge, each at the smallest shape that reaches it.

A case fixes (arithmetic, d_k, H, lens, bias form, u . k on / off, kv_len, Q / K layout, V^T layout, output stride, operand generator).  Every
buffer is built by `tensors()` as a view into a flat allocation that holds NaN wherever the kernel has no business: V^T slack columns, Q / K
buffer columns that belong to neither, the columns of a rel-pos row outside what the sequence's rel-shift addresses, the output's slack.
`branch(case)` restates launch_attn / relattn_kernel's constexpr logic -- (T, DK, KBT, REL, NW, schedule) -- and, per sequence, the run-time
facts (`seq_facts`), from the same description: no device and no library are needed to know where a case goes.

Two kinds of case.

  selection   the softmax is one-hot, so out[i] = v[pi(i)] to the last bit in every arithmetic: the winner's probability is exp(0) = 1, every
              other score lies at least 400 below it after scaling, __expf(-400) = 0 in f32, l = 1.  V holds non-zero integers in [-1023, 1023],
              a function of (sequence, head, key, channel): exact in f16, in the split hi / lo pair and in three bf16 planes; a wrong key, head,
              sequence, V^T column, swizzle unit or plane order is a different integer.  Compared by torch.equal.  Selectors:
                qk      Q and K rows are +-1 codes: q_i . k_j = d_k iff j = pi(i), <= 3/4 d_k otherwise (codes differ in >= 1 of 8 bits, each bit
                        fills d_k / 8 channels; a fixed sign per channel multiplies both, so a mispaired channel shows), scale = 256.  With kv_len
                        the keys >= Tk repeat the codes of keys 0, 1, ...: the winner exists on both sides of the mask and only the mask decides.
                qk11    every Q and K element is +-(256 + z), the sign fixed per channel, z in {0, 1} the 0 / 1 form of a Walsh code (d_k / 2 ones;
                        two different codes share d_k / 4): q_i . k_j = 65536 d_k + 256 d_k + (d_k / 2 if j = pi(i) else d_k / 4) -- the winner is
                        decided by the products of the operands' SECOND bf16 terms alone (by the lowest bits of the f16 / f32 products).  The sums
                        are integers <= 2**24 (1 + 2**-7): an accumulator above 2**24 may round an odd partial sum by 1, in the last few adds of
                        d_k = 256 only, against a gap of d_k / 4 = 64; T <= 31, scale = 256: the gap is >= 2048 after scaling.
                rel     Q = K = 0, the table holds 1 in the slot its mode maps to (i, pi(i)) -- found by pushing a table of its own flat indices
                        through the oracle's rel_shift_legacy / rel_shift_new -- and 0 elsewhere; scale = 512.
                relneg  legacy, the whole table -1: the wrap element j = i + 1 that legacy rel-shift leaves at 0 wins, row i < T - 1 is v[i + 1]
                        exactly; the last row is the uniform mean, held to the arithmetic bound.
                ku      Q = K = 0, u . k is 0 at one key per (sequence, head) and -1 elsewhere; scale = 512.
  arithmetic  operands with full 24-bit significands (f16-rounded for F16).  K and V magnitudes are scaled per 32-key block by powers of two in
              2**-6 .. 2**6, rising and falling, so the split arithmetic's tile scales change from tile to tile; even rows' q is sign-aligned with a
              key of the first block, odd rows' with one of the last, so the running maximum is set by the first tile in some rows and rises in the
              last in others; `scale` keeps the score condition kappa <~ 10.  Elementwise against the float64 attention (`Case.bound`).

The arithmetic bound.  u = 2**-23 (a whole ulp, as in bgemm_cases.bound_factor: the rounding inside the MFMAs is not documented).  For query i let
kappa_i = max_j scale (sum_c |q_ic k_jc| + |ku_j| + |bd_ij|) over the unmasked keys, p_ij the float64 probabilities, M_ic = sum_j p_ij |v_jc|,
l_i = sum_j exp(s_ij - max_j s_ij) >= 1, nt the number of key tiles, Tk the number of unmasked keys.

  score      s_ij is a d_k-term dot product plus two adds and the scale product: |ds_ij| <= S kappa_i u with
               F32, F16   S = d_k + 4              (d_k products and adds as in bgemm's exact bound d_k + 2, + 2 for the bias adds and the scale; f16
                                                    operands are exact and so are their products in the f32 accumulator)
               F32S       S = 1.05 d_k + 4 + 6     (three MFMAs into one accumulator: the two cross terms are 2**-11 of the leading one, 1.05 d_k
                                                    covers them as it does for the emulated product; per product the hi + lo pair of q and of k is
                                                    off by <= 2**-22 each and lo . lo (<= 2**-22) is dropped: 3 x 2**-22 = 6 u.  The pair's error is
                                                    relative to the ELEMENT as long as it lies within 2**-13 of its tile's maximum -- the residual
                                                    of hi then stays a normal f16 -- which the generator keeps: exponents -6 .. 6 within a tile)
               F32E       S = 1.05 d_k + 4 + PER_PRODUCT_7 / 2     (bgemm_cases.bound_factor's accounting: 1.05 d_k for the two accumulators,
                                                    PER_PRODUCT_7 x 2**-24 per product for the dropped products and the joining add)
  exp        the weight w_ij = exp(s_ij - m) is taken of an argument of magnitude <= 2 kappa_i: its subtraction and the product with log2(e) inside
             __expf round once each (<= 4 kappa_i u absolute), v_exp_f32 is good to one ulp, taken as 2 u: E_i = (4 kappa_i + 2) u
  rescale    a tile's weights are multiplied by the alpha of every later tile: (nt - 1) (E_i + u).  (The SAME alpha multiplies l and O, but tiles
             carry different numbers of them, so it does not cancel.)
  =>         a weight's relative error rho_i = S kappa_i u + E_i + (nt - 1) (E_i + u).  out = N / D with N = sum w v, D = sum w: 2 rho_i M_ic.
  sums       N is a Tk-term sum in f32 plus one product per rescale (Tk + nt), D one in 1/4 of the adds per lane plus two shuffles and the rescales
             (Tk / 4 + nt + 2), the final reciprocal and product 2: (1.25 Tk + 2 nt + 10) u M_ic with the second-order terms.  F32S: P's and V's
             hi + lo pairs and the dropped lo . lo add 6 u, 1.05 Tk for the three MFMAs; F32E: 1.05 Tk + PER_PRODUCT_7 / 2.
  F16        P is rounded to f16 for the MFMA (the normaliser sums the f32 p): 2**-11 M_ic; the output is rounded to f16: 2**-11 |out| <= 2**-11 M_ic.

  B_i = 2 rho_i / u + sums (in units of u)  [+ 2 x 2**-11 / u for F16];  |out - ref|_ic <= B_i u M_ic + A_ic.

  A_ic, the absolute term, is needed in two arithmetics only, where P underflows its operand format: F16 -- a p below 2**-14 is a subnormal f16,
  spaced 2**-24 -- and F32S -- P is split at the fixed scale 2**15, so the lo half of a p below 2**-18 is a subnormal f16: 2**-25 / 2**15 = 2**-40.
  Each key contributes that much of |v_jc| to N (in the running maximum's units, only shrunk by later alphas), N is divided by l_i:
  A_ic = a sum_j |v_jc| / l_i with a = 2**-25 (F16), 2**-40 (F32S), 0 (F32, F32E: f32 and bf16 have f32's exponent range); F16 adds 2**-25 for
  an output that is a subnormal f16.  With kappa <~ 10 every p >= exp(-20) > 2**-29, far above f32's own underflow.
"""
import functools
import math
import zlib

import torch

from test_train_emul_gpu import PER_PRODUCT_7      # 2.01 x 2**-24 |a b| per emulated product (the existing per-product tests)

NAN = float("nan")
F32, F16, F32S, F32E = 0, 1, 2, 3          # _abi's dtype codes (the CPU test compares)
ARITHS = [F16, F32, F32S, F32E]
ANAME = {F16: "f16", F32: "f32", F32S: "split", F32E: "emul"}
DKS = [32, 64, 96, 128, 192, 256]
LENGTHS = [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128, 129, 130]      # the issue's set; 3 added for the 13-sequence grid, 0 for the empty one
U = 2.0 ** -23
BIAS = ["none", "ku", "legacy", "new"]
VT_LOSE = ["ld", "col", "ptr"]             # the three vt_vec conditions: ldvt % 8, vt_col0 % 8, base pointer % 32 bytes
# the build's constants that the constexpr logic reads (attention.hip's #ifndef defaults; the Makefile defines none of them)
ATTN_HALFPF, ATTN_DMA = 1, 2


def esize(arith):
    return 2 if arith == F16 else 4


def tdtype(arith):
    return torch.float16 if arith == F16 else torch.float32


def round_up(v, m):
    return (v + m - 1) // m * m


# ------------------------------------------------------------------------------------------------------------------------------ dispatch, restated
def instantiation(arith, dk, has_g, has_ku):
    """launch_attn + the constexpr block of relattn_kernel -> (arith, DK, KBT, REL, NW, schedule)."""
    size = {F16: 2, F32: 4, F32S: 4, F32E: 6}[arith]      # sizeof(T): f16, float, f16s {hi, lo}, bf3 {b0, b1, b2}
    split, emul = arith == F32S, arith == F32E
    rel, nw = True, 4
    if emul:
        kbt = 64 if dk <= 96 else 32
    elif size == 4 and dk >= 128 and dk % 64 == 0:
        kbt = 32
        if dk == 256 and split:
            nw = 8
        elif dk == 256 and not has_g and not has_ku:
            rel = False
    else:
        kbt = 64
    dma_ok = size == 4 and not split and kbt == 32 and nw == 4 and dk % 64 == 0 and (ATTN_DMA >= 2 or (ATTN_DMA == 1 and not rel and dk == 256))
    prefetch = not dma_ok and (nw == 8 or emul or ((dk <= 192 or size != 2) and not (kbt == 32 and dk > 192)))
    halfpf = bool(ATTN_HALFPF) and not prefetch and not split and size == 4
    schedule = "dma" if dma_ok and halfpf else "half" if halfpf else "prefetch" if prefetch else "none"
    return (arith, dk, kbt, rel, nw, schedule)


ALL_INSTANTIATIONS = sorted({instantiation(a, dk, g, ku) for a in ARITHS for dk in DKS for g in (False, True) for ku in (False, True)})


class Case:
    def __init__(self, group, name, arith, dk, H, lens, kind, bias="none", ku=None, vt="layout", qk="sep", ldo_extra=0, kv=None, note="", seq_ids=None,
                 parent=None):
        self.group, self.name, self.arith, self.dk, self.H, self.lens, self.kind, self.bias = group, name, arith, dk, H, list(lens), kind, bias
        self.ku_on = (bias != "none") if ku is None else ku
        self.vt, self.qk, self.ldo_extra, self.kv, self.note = vt, qk, ldo_extra, kv, note
        self.seq_ids = list(range(len(lens))) if seq_ids is None else seq_ids      # operand values are a function of (seed, sequence id): `alone()`
        self.exact = kind != "arith"
        self.A, self.R, self.Tm = H * dk, sum(lens), max(lens)
        self.id = f"{group}/{ANAME[arith]}-dk{dk}/{name}"
        self.seed = parent.seed if parent else zlib.crc32(repr((group, name, arith, dk, H, kind, bias)).encode()) % 100003
        self.Tm_table = parent.Tm_table if parent else self.Tm      # the rel table's geometry stays the batch's when a sequence runs alone
        assert kind in ("qk", "qk11", "rel", "relneg", "ku", "arith") and bias in BIAS and vt in ("layout", "packed", *VT_LOSE) and qk in ("sep", "fused", "wide")
        assert kv is None or len(kv) == len(lens)
        if kind in ("rel", "relneg"):
            assert bias in ("legacy", "new") and not self.ku_on
        if kind == "ku":
            assert bias == "ku"
        self.scale = parent.scale if parent else {"qk": 256.0, "qk11": 256.0, "rel": 512.0, "relneg": 512.0, "ku": 512.0}.get(kind) or self._arith_scale()

    # ---- geometry
    @property
    def has_g(self):
        return self.bias in ("legacy", "new")

    @property
    def rel_mode(self):
        return {"none": 0, "ku": 0, "legacy": 1, "new": 2}[self.bias]

    @property
    def cap(self):
        return self.Tm_table + 3      # > max_len

    @property
    def center(self):
        return self.cap - 1 if self.bias == "new" else 0

    @property
    def n_pos(self):
        return self.Tm_table if self.bias == "legacy" else 2 * self.cap - 1 if self.bias == "new" else 0

    @property
    def ldg(self):
        return self.n_pos + 5 if self.has_g else 0      # rows of the table start at any element: the gather's 4-wide loads are unaligned by design

    def row0(self, b):
        return sum(self.lens[:b])

    def tk(self, b):
        """The kernel's clamp: min(max(kv_len, 1), Tn)."""
        T = self.lens[b]
        return T if self.kv is None else min(max(self.kv[b], 1), T)

    def qk_layout(self):
        """(ldq, q_col0, ldk, k_col0)."""
        A = self.A
        return {"sep": (A, 0, A, 0), "fused": (2 * A, 0, 2 * A, A), "wide": (A + 8, 8, A + 16, 0)}[self.qk]

    def vt_geometry(self):
        """(element offset of the base from the allocation, ldvt, [col0 per sequence] or None = the sequence's first row)."""
        if self.vt == "packed":
            return 0, self.R, None
        col, c = [], 0
        for T in self.lens:
            col.append(c)
            c += round_up(T, 8)
        ld = c + 8      # RaggedBatch.vt_layout()
        if self.vt == "ld":
            ld += 4
        if self.vt == "col":
            col, ld = [v + 4 for v in col], ld + 8
        off = 16 // esize(self.arith) if self.vt == "ptr" else 0      # 16 bytes: every 16-byte load stays aligned, the 32-byte test fails
        return off, ld, col

    def vt_props(self, b):
        """What vt_vec needs to be zero, by name."""
        off, ld, col = self.vt_geometry()
        return {"ld": ld % 8, "col": (self.row0(b) if col is None else col[b]) % 8, "ptr": off * esize(self.arith) % 32}

    def vt_vec(self, b):
        return all(v == 0 for v in self.vt_props(b).values())

    @property
    def ldo(self):
        return self.A + self.ldo_extra

    def alone(self, b):
        """Sequence b of this case as a batch of one: the same operand values (rows, table geometry), its own launch."""
        return Case(self.group, f"{self.name}-alone{b}", self.arith, self.dk, self.H, [self.lens[b]], self.kind, self.bias, self.ku_on, self.vt, self.qk,
                    self.ldo_extra, None if self.kv is None else [self.kv[b]], seq_ids=[self.seq_ids[b]], parent=self)

    # ---- operand values, per sequence: q, k, v (T, H, dk); ku (T, H) or None; g (T, H, n_pos) or None, NaN where the rel-shift must not look
    def _blocks(self, T):
        nb = (T + 31) // 32
        ek = [5] + [[-6, 6, -3][(i - 1) % 3] for i in range(1, nb - 1)] + ([6] if nb > 1 else [])
        ev = [[-6, 6, 0, -4, 3][i % 5] for i in range(nb)]
        return ek, ev

    def _arith_scale(self):
        ekmax = max(max(self._blocks(T)[0]) for T in self.lens if T > 0)
        return 2.0 ** math.floor(math.log2(8.0 / (2.25 * self.dk * 2.0 ** ekmax)))      # E |q| |k| = 2.25 2**ek per channel: kappa <~ 8

    def pi(self, b, h):
        """The selection cases' winner of every query of (sequence, head): crosses tiles in both directions."""
        T, Tk, sid = self.lens[b], self.tk(b), self.seq_ids[b]
        i = torch.arange(T)
        if self.kind == "ku":
            return torch.full((T,), (5 + 29 * h + 13 * sid) % Tk)
        if self.kind == "relneg":
            return torch.clamp(i + 1, max=T - 1)      # (the last row has no winner)
        p = Tk - 1 - i % Tk if h % 2 == 0 else (7 * i + 3) % Tk
        assert self.kind != "qk11" or T <= 31      # 31 Walsh codes of length 32 besides the constant one
        if self.bias == "legacy":      # the wrap element cannot be selected by the table
            p = torch.where(p == i + 1, i, p)
        return p

    def _seq(self, b):
        T, H, dk, sid = self.lens[b], self.H, self.dk, self.seq_ids[b]
        gen = torch.Generator().manual_seed(self.seed * 131 + sid)
        rnd16 = (lambda t: t.half().float()) if self.arith == F16 else (lambda t: t)
        ku = g = None
        if T == 0:
            e = torch.zeros(0, H, dk)
            return e, e, e, torch.zeros(0, H) if self.ku_on else None, torch.zeros(0, H, self.n_pos) if self.has_g else None
        if self.kind == "arith":
            def rnd(shape):
                mant = 1.0 + torch.rand(shape, generator=gen, dtype=torch.float64)
                sign = torch.randint(0, 2, shape, generator=gen).double() * 2 - 1
                return mant * sign
            ek, ev = self._blocks(T)
            blk = torch.arange(T) // 32
            k = rnd16((rnd((T, H, dk)) * (2.0 ** torch.tensor(ek, dtype=torch.float64))[blk, None, None]).float())
            v = rnd16((rnd((T, H, dk)) * (2.0 ** torch.tensor(ev, dtype=torch.float64))[blk, None, None]).float())
            q = rnd((T, H, dk)).abs()
            i = torch.arange(T)
            tgt = torch.where(i % 2 == 0, (5 * i) % min(T, 32), T - 1 - i % min(T, 2))
            q = rnd16((q * torch.sign(k[tgt].double())).float())
            if self.ku_on:
                ku = ((torch.rand((T, H), generator=gen, dtype=torch.float64) * 2 - 1) / self.scale).float()
            if self.has_g:
                g = rnd16(((torch.rand((T, H, self.n_pos), generator=gen, dtype=torch.float64) * 2 - 1) / self.scale).float())
        else:
            j, c, h = torch.arange(T)[:, None, None], torch.arange(dk)[None, None, :], torch.arange(H)[None, :, None]
            x = (97 * j + 7 * c + 523 * h + 211 * sid) % 2046
            v = torch.where(x < 1023, x - 1023, x - 1022).float()
            q = k = torch.zeros(T, H, dk)
            if self.kind == "qk":
                Tk = self.tk(b)
                jj = torch.where(j < Tk, j, (j - Tk) % Tk)                 # keys past the mask repeat the codes of keys 0, 1, ...
                code = (jj + 37 * h + 11 * sid) % 256
                chan = torch.where((c * c + c // 8) % 3 == 0, -1, 1)
                k = (((code >> (c % 8)) & 1) * 2 - 1).mul(chan).float()
                q = torch.stack([k[self.pi(b, h_), h_] for h_ in range(H)], 1)
            if self.kind == "qk11":
                row = 1 + (j + 5 * h + 3 * sid) % 31                       # distinct for the T <= 31 keys of a (sequence, head)
                par = row & (c % 32)
                for sh in (16, 8, 4, 2, 1):
                    par = par ^ (par >> sh)
                chan = torch.where((c * c + c // 8) % 3 == 0, -1, 1)
                k = ((256 + (1 - (par & 1))) * chan).float()               # chan x (256 + z), z = (1 + Walsh(row)[c % 32]) / 2
                q = torch.stack([k[self.pi(b, h_), h_] for h_ in range(H)], 1)
            if self.kind == "ku" or (self.kind == "qk" and self.ku_on):
                ku = torch.full((T, H), -1.0 if self.kind == "ku" else 0.0)
                if self.kind == "ku":
                    for h_ in range(H):
                        ku[int(self.pi(b, h_)[0]), h_] = 0.0
            if self.has_g:
                g = torch.full((T, H, self.n_pos), -1.0 if self.kind == "relneg" else 0.0)
                if self.kind == "rel":
                    flat = g.permute(1, 0, 2).reshape(-1)      # a copy in (H, T, n_pos) order
                    slots = self.shift(torch.arange(1, flat.numel() + 1).view(H, T, self.n_pos), T)      # (H, T, T) of flat index + 1; 0 = the wrap element
                    for h_ in range(H):
                        s = slots[h_, torch.arange(T), self.pi(b, h_)]
                        assert bool((s > 0).all())
                        flat[s - 1] = 1.0
                    g = flat.view(H, T, self.n_pos).permute(1, 0, 2).contiguous()
        if g is not None:      # poison what this sequence's rel-shift does not address
            lo, hi = (0, T) if self.bias == "legacy" else (self.center - (T - 1), self.center + T)
            g[:, :, :lo] = NAN
            g[:, :, hi:] = NAN
        return q, k, v, ku, g

    def shift(self, table, T):
        """(H, T, n_pos) table -> (H, T, T) bias, by the oracle's rel-shift (any dtype)."""
        from oracle.fs2_oracle import rel_shift_legacy
        from oracle.vits_oracle import rel_shift_new
        if self.bias == "legacy":
            return rel_shift_legacy(table[:, :, :T])
        return rel_shift_new(table[:, :, self.center - (T - 1):self.center + T])

    @functools.cached_property
    def data(self):
        """q, k, v (R, H, dk) f32; ku (R, H) f32 or None; g (R, H, n_pos) f32 or None."""
        seqs = [self._seq(b) for b in range(len(self.lens))]
        cat = lambda n: None if seqs[0][n] is None else torch.cat([s[n] for s in seqs])  # noqa: E731
        return tuple(cat(n) for n in range(5))

    # ---- the reference
    def attention(self, dtype):
        """Plain attention of the case's operands in `dtype` -> dict of (R, H, dk) / (R, H) tensors.  float64: the reference and the bound's
        ingredients; float32: the CPU test's honest f32 evaluation."""
        q, k, v, ku, g = (None if t is None else t.to(dtype) for t in self.data)
        H, dk = self.H, self.dk
        out, M, absv = (torch.zeros(self.R, H, dk, dtype=dtype) for _ in range(3))
        kappa, l, gap = (torch.zeros(self.R, H, dtype=dtype) for _ in range(3))
        o = 0
        for b, T in enumerate(self.lens):
            if T == 0:
                continue
            Tk, sl = self.tk(b), slice(o, o + T)
            qs, ks, vs = (t[sl].transpose(0, 1) for t in (q, k, v))      # (H, T, dk)
            s = qs @ ks.transpose(1, 2)
            cond = qs.abs() @ ks.abs().transpose(1, 2)
            if ku is not None:
                s = s + ku[sl].t().unsqueeze(1)
                cond = cond + ku[sl].t().unsqueeze(1).abs()
            if g is not None:
                bd = self.shift(torch.nan_to_num(g[sl].permute(1, 0, 2), nan=0.0), T)      # (the slots the rel-shift does not address: CPU test)
                s = s + bd
                cond = cond + bd.abs()
            s = s * self.scale
            s[:, :, Tk:] = float("-inf")
            m = s.max(-1, keepdim=True).values
            w = torch.exp(s - m)
            p = w / w.sum(-1, keepdim=True)
            top2 = s.topk(min(2, T), -1).values
            gap[sl] = (top2[..., 0] - top2[..., -1] if Tk > 1 else torch.full((H, T), float("inf"), dtype=dtype)).t()
            out[sl], M[sl] = (p @ vs).transpose(0, 1), (p @ vs.abs()).transpose(0, 1)
            absv[sl] = vs[:, :Tk].abs().sum(1, keepdim=True).transpose(0, 1).expand(T, H, dk)
            kappa[sl], l[sl] = (cond[:, :, :Tk].max(-1).values * self.scale).t(), w.sum(-1).t()
            o += T
        return dict(out=out, M=M, absv=absv, kappa=kappa, l=l, gap=gap)

    @functools.cached_property
    def ref(self):
        return self.attention(torch.float64)

    def expected(self):
        """Selection cases: out (R, H, dk) f32 = v[pi(i)], by construction (the CPU test holds the float64 softmax against it)."""
        _, _, v, _, _ = self.data
        out, o = torch.empty_like(v), 0
        for b, T in enumerate(self.lens):
            for h in range(self.H):
                out[o:o + T, h] = v[o + self.pi(b, h), h]
            o += T
        return out

    def exact_rows(self):
        """(R,) bool: the rows the selection criterion covers (relneg: all but each sequence's last, which is the uniform mean)."""
        m, o = torch.ones(self.R, dtype=torch.bool), 0
        for T in self.lens:
            if self.kind == "relneg" and T:
                m[o + T - 1] = False
            o += T
        return m

    def n_tiles(self):
        """(R,) key tiles per row."""
        kbt = branch(self)[2]
        return torch.cat([torch.full((T,), (self.tk(b) + kbt - 1) // kbt) for b, T in enumerate(self.lens)] + [torch.zeros(0, dtype=torch.long)])

    def bound(self, arith=None):
        """(R, H, dk) float64: the elementwise bound on |out - ref| (module docstring)."""
        arith = self.arith if arith is None else arith
        r, dk = self.ref, self.dk
        nt = self.n_tiles().double()[:, None]
        tk = torch.cat([torch.full((T,), float(self.tk(b))) for b, T in enumerate(self.lens)] + [torch.zeros(0)]).double()[:, None]
        S = {F32: dk + 4.0, F16: dk + 4.0, F32S: 1.05 * dk + 10.0, F32E: 1.05 * dk + 4.0 + PER_PRODUCT_7 / 2}[arith]
        E = 4.0 * r["kappa"] + 2.0
        rho = S * r["kappa"] + E + (nt - 1.0) * (E + 1.0)
        sums = {F32: 1.25 * tk, F16: 1.25 * tk, F32S: 1.3 * tk + 6.0, F32E: 1.3 * tk + PER_PRODUCT_7 / 2}[arith] + 2.0 * nt + 10.0
        B = 2.0 * rho + sums + (2.0 * 2.0 ** 12 if arith == F16 else 0.0)      # 2 x 2**-11 in units of 2**-23
        a = {F32: 0.0, F32E: 0.0, F16: 2.0 ** -25, F32S: 2.0 ** -40}[arith]
        return B.unsqueeze(-1) * U * r["M"] + a * r["absv"] / r["l"].unsqueeze(-1) + (2.0 ** -25 if arith == F16 else 0.0)

    def criterion(self):
        if self.kind == "arith":
            return "|out-ref| <= B u M + A (float64)"
        return "torch.equal(v[pi(i)])" + (" + last row: uniform mean at the arithmetic bound" if self.kind == "relneg" else "")


# ------------------------------------------------------------------------------------------------------------------------------ placement
def tensors(c, device="cpu"):
    """Every buffer of the case on `device`, NaN wherever no operand lives -> dict: q, k (base tensors for _ptr(col0)), vt, g, ku, out (flat buffers /
    views), kv, vt_col0, and `covered`: name -> bool mask over the flat buffer of the elements that hold values."""
    dt = tdtype(c.arith)
    q, k, v, ku, g = c.data
    R, A, H = c.R, c.A, c.H
    ldq, qc0, ldk, kc0 = c.qk_layout()
    t, cov = {}, {}

    def flat(n):
        return torch.full((n,), NAN, dtype=dt, device=device)
    if c.qk == "fused":
        buf = flat(R * 2 * A + 8)
        view = buf[:R * 2 * A].view(R, 2 * A)
        view[:, :A], view[:, A:] = q.reshape(R, A).to(device, dt), k.reshape(R, A).to(device, dt)
        t["q"] = t["k"] = t["qk_buf"] = buf
        cov["qk_buf"] = torch.arange(buf.numel()) < R * 2 * A
    else:
        for name, vals, ld, c0 in (("q", q, ldq, qc0), ("k", k, ldk, kc0)):
            buf = flat(R * ld + 8)
            buf[:R * ld].view(R, ld)[:, c0:c0 + A] = vals.reshape(R, A).to(device, dt)
            t[name] = buf
            col = torch.arange(buf.numel()) % ld
            cov[name] = (torch.arange(buf.numel()) < R * ld) & (col >= c0) & (col < c0 + A)
    off, ldvt, col0 = c.vt_geometry()
    buf = flat(off + A * ldvt + 16)
    view = buf[off:off + A * ldvt].view(A, ldvt)
    mask = torch.zeros(A, ldvt, dtype=torch.bool)
    for b, T in enumerate(c.lens):
        c0, r0 = (c.row0(b) if col0 is None else col0[b]), c.row0(b)
        view[:, c0:c0 + T] = v[r0:r0 + T].reshape(T, A).t().to(device, dt)
        mask[:, c0:c0 + T] = True
    t["vt_buf"], t["vt"] = buf, buf[off:]
    cov["vt_buf"] = torch.cat([torch.zeros(off, dtype=torch.bool), mask.reshape(-1), torch.zeros(16, dtype=torch.bool)])
    t["vt_col0"] = None if col0 is None else torch.tensor(col0, dtype=torch.int32, device=device)
    t["g"] = None
    if g is not None:
        buf = flat(R * H * c.ldg + 8)
        buf[:R * H * c.ldg].view(R, H, c.ldg)[:, :, :c.n_pos] = g.to(device, dt)
        t["g"] = buf
    t["ku"] = None if ku is None else ku.to(device)
    t["kv"] = None if c.kv is None else torch.tensor(c.kv, dtype=torch.int32, device=device)
    t["out"] = flat(R * c.ldo + 8)
    col = torch.arange(R * c.ldo + 8) % c.ldo
    cov["out"] = (torch.arange(R * c.ldo + 8) < R * c.ldo) & (col < A)
    t["covered"] = cov
    return t


def out_view(c, out_buf):
    return out_buf[:c.R * c.ldo].view(c.R, c.ldo)[:, :c.A].reshape(c.R, c.H, c.dk)


# ------------------------------------------------------------------------------------------------------------------------------ run-time facts
def branch(c):
    return instantiation(c.arith, c.dk, c.has_g, c.ku_on)


def grid_total(c):
    nw = branch(c)[4]
    return (c.Tm + 16 * nw - 1) // (16 * nw) * len(c.lens) * c.H


def seq_facts(c, b):
    """The run-time facts of sequence b: which loads, tiles and gather branches its workgroups take."""
    _, _, kbt, rel, nw, _ = branch(c)
    T, Tk = c.lens[b], c.tk(b)
    f = dict(T=T, Tk=Tk, vt_vec=c.vt_vec(b), tiles=(Tk + kbt - 1) // kbt if T else 0, wgs=(T + 16 * nw - 1) // (16 * nw),
             clamped_queries=T % (16 * nw) != 0, gather=set())
    if T == 0:
        return f
    last = (f["tiles"] - 1) * kbt
    f["last_partial"] = last + kbt > T                       # the V^T mask / zero fill runs (relative to Tn, not Tk)
    f["tk_vs_tn"] = "eq" if Tk == T else "lt"
    f["tk_vs_edge"] = "at" if Tk % kbt == 0 else "after" if Tk % kbt == 1 else "before" if Tk % kbt == kbt - 1 else "inside"
    if rel and c.has_g:
        for qi in range(T):
            for jq in range(0, f["tiles"] * kbt, 4):
                inside = jq + 3 < T
                if c.rel_mode == 2:
                    f["gather"].add("new-4wide" if inside else "new-edge")
                elif inside and jq + 3 <= qi:
                    f["gather"].add("legacy-below")
                elif inside and jq > qi + 1:
                    f["gather"].add("legacy-above")
                else:
                    f["gather"].add("legacy-straddle")
    return f


def winner_gather(c):
    """Selection by the table: the gather branch that delivers each winner's 1 (the other branches deliver the zeros around it)."""
    seen = set()
    for b, T in enumerate(c.lens):
        for h in range(c.H):
            for qi, j in enumerate(c.pi(b, h).tolist()):
                jq = j // 4 * 4
                inside = jq + 3 < T
                if c.rel_mode == 2:
                    seen.add("new-4wide" if inside else "new-edge")
                else:
                    seen.add("legacy-below" if inside and jq + 3 <= qi else "legacy-above" if inside and jq > qi + 1 else "legacy-straddle")
    return seen


GATHER = ["legacy-below", "legacy-above", "legacy-straddle", "new-4wide", "new-edge"]

# ------------------------------------------------------------------------------------------------------------------------------ the table
SEL_LENS = [130, 17]            # three 64-key / five 32-key tiles with a partial last one, and one partial tile
ARITH_LENS = [17, 64, 130]      # one (partial) tile, an exact tile multiple, a partial last tile
KV_LENS = [130] * 7


def kv_values(kbt, T):
    return [1, kbt, kbt - 1, kbt + 1, T, 0, T + 5]      # 0 and T + 5: the kernel clamps them to 1 and T


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))  # noqa: E731
    for arith in ARITHS:
        for dk in DKS:
            H = 2 if dk <= 128 else 1
            for vt in ("layout", "packed"):
                # 1. selection, every instantiation x both V^T paths: by q . k (no bias: REL = false at f32 d_k 256), by either table, by u . k
                add("sel", f"qk-{vt}", arith, dk, H, SEL_LENS, "qk", "none", vt=vt)
                add("sel", f"legacy-{vt}", arith, dk, H, SEL_LENS, "rel", "legacy", ku=False, vt=vt)
                add("sel", f"new-{vt}", arith, dk, H, SEL_LENS, "rel", "new", ku=False, vt=vt)
                add("sel", f"ku-{vt}", arith, dk, H, SEL_LENS, "ku", "ku", vt=vt)
                # 2. arithmetic, every instantiation x the four bias forms x both V^T paths
                for bias in BIAS:
                    add("arith", f"{bias}-{vt}", arith, dk, H, ARITH_LENS, "arith", bias, vt=vt)
            # the second bf16 terms decide (the emulated product's b1 . b1; T <= 31: one partial tile)
            add("sel", "qk11", arith, dk, H, [31, 17], "qk11", "none")
    # 3. the wrap element of legacy rel-shift, and the key mask at every edge -- one d_k per (arithmetic, tile size, schedule) family, the NW = 8 and
    #    the REL = false kernels among them; the mask cases select by q . k with the winner's code on both sides of kv_len
    fam = [(F16, 64), (F16, 256), (F32, 32), (F32, 128), (F32, 256), (F32S, 96), (F32S, 192), (F32S, 256), (F32E, 64), (F32E, 256)]
    for arith, dk in fam:
        kbt = instantiation(arith, dk, False, False)[2]
        add("wrap", "relneg", arith, dk, 1, [130, 1, 33], "relneg", "legacy", ku=False)
        for vt in ("layout", "packed"):
            add("mask", f"kv-{vt}", arith, dk, 1, KV_LENS, "qk", "none", vt=vt, kv=kv_values(kbt, 130))
        add("mask", "kv-ku", arith, dk, 1, KV_LENS, "qk", "ku", kv=kv_values(kbt, 130), note="REL = true at f32 d_k 256: u . k of zeros")
        add("mask", "kv-arith", arith, dk, 1, [130, 65, 65, 130], "arith", "legacy", kv=[kbt + 1, 64, 40, 97], note="Tk < Tn under the legacy geometry of Tn")
    add("mask", "kv-nw8-129", F32S, 256, 1, [129] * 7, "qk", "none", kv=kv_values(32, 129), note="the second 128-query workgroup holds one query")
    # 4. layout and indexing
    for arith in ARITHS:
        for dk in (32, 128):
            add("layout", "fused-qk", arith, dk, 2, SEL_LENS, "qk", "none", qk="fused", note="the models' call: ldq = ldk = 2A, k_col0 = A")
            add("layout", "fused-arith", arith, dk, 2, [33, 130], "arith", "new", qk="fused")
            add("layout", "wide-ldo", arith, dk, 2, [65, 16], "qk", "none", qk="wide", ldo_extra=8, note="NaN columns around Q and K, out with slack")
            add("layout", "ldo-arith", arith, dk, 2, [65, 16], "arith", "ku", ldo_extra=24)
            for what in VT_LOSE:
                add("losevec", what, arith, dk, 2, [33, 64], "qk", "none", vt=what)
            add("losevec", "aligned", arith, dk, 2, [33, 64], "qk", "none", vt="layout")
            add("losevec", "packed-aligned", arith, dk, 2, [16, 32], "qk", "none", vt="packed", note="ldvt = R = 48, rows 0 and 16: the 16-byte path without vt_col0")
        for H in (1, 3):
            add("heads", f"H{H}", arith, 32, H, [65, 2], "qk", "none", qk="fused")
            add("heads", f"H{H}-legacy", arith, 64, H, [65, 2], "rel", "legacy", ku=False)
        # grids: 1, 39, 9 (NW = 4: three query blocks x 3 heads) and 16 workgroups in launches of 8, 40, 16, 16
        add("grid", "one", arith, 32, 1, [2], "qk", "none")
        add("grid", "13seq", arith, 32, 3, [1, 2, 3] * 4 + [1], "qk", "none")
        add("grid", "130x3", arith, 32, 3, [130], "qk", "none")
        add("grid", "8x2", arith, 32, 2, [64] * 8, "qk", "none")
        add("empty", "middle", arith, 64, 2, [17, 0, 33], "qk", "none")
        add("empty", "middle-legacy", arith, 64, 2, [17, 0, 33], "rel", "legacy", ku=False, vt="packed")
        # 5. a sequence alone == inside the batch, bit for bit (arithmetic operands: every bit of the result is at stake)
        for dk in (64, 256):
            for bias in ("none", "legacy", "new"):
                add("alone", bias, arith, dk, 2 if dk == 64 else 1, [65, 1, 130, 33], "arith", bias)
    add("grid", "nw8-129", F32S, 256, 2, [129], "qk", "none", note="NW = 8: two query workgroups per head, the second with one query")
    add("grid", "nw8-130x3", F32S, 256, 3, [130, 128], "ku", "ku")
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def case_id(c):
    return c.id


def release(c):
    for attr in ("data", "ref"):
        c.__dict__.pop(attr, None)
