"""Case table of tests/test_bgemm_cases_{cpu,gpu}.py: jatts_bgemm and jatts_bgemm_emul (csrc/bgemm.hip) at every tile, load path, batch
index and edge, each at the smallest shape that reaches it.

A case is (kernel, batch (O, I), m, n, k, transpose form, one memory layout per operand and for C, operand generator, alpha, accumulate,
forced tile).  A layout (`Lay`) is the element offset of matrix (0, 0) from a 16-byte aligned allocation and the strides of (outer, inner,
row); `place()` builds the tensor from it -- a view into a flat buffer that holds NaN in every element the view does not cover, so that a
load mask that lets one slack element through, or a store outside the matrix, shows.  The GPU test builds its tensors with the same
function; `branch(case)` reads pointer alignment and strides from the same description, so no device is needed to know where a case goes.

`branch(case)` restates the dispatch of jatts_bgemm and bgemm_emul_launch: (kernel, WNF, BK, MF, vec, AK, BKC) = 64 WNF columns and 64 MF
rows per tile, chunk depth BK, 16-byte loads, K contiguous in A / in B.

Two kinds of case:

  integer (`exact`)   operands are integers stored in f32; every product and every partial sum in any order is an integer below 2**24
                      (`Case.absref`: sum |a| |b| per output, the CPU test proves it), so the float64 product of the same integers IS the
                      expected value to the last bit, in any summation order, with or without FMA; compared by torch.equal.
                      gen "small": both operands in [-4, 4].  gen "odd16": A holds odd integers 257 .. 65 535 (two non-zero bf16 terms),
                      B values in {-2, -1, 1, 2}, K <= 64: |sum| <= 64 x 65 535 x 2 < 2**23 -- the emulated kernel's routing of the first
                      two terms of A is checked to the bit.
  arithmetic          positive operands with random full 24-bit significands and exponents 2**-6 .. 2**6: nothing cancels, (|A| |B|)_ij is
                      the result itself.  Elementwise against the float64 product: |c - ref| <= B(K) 2**-23 (|A| |B|)_ij, B below.
"""
import functools
import zlib

import torch

from test_train_emul_gpu import PER_PRODUCT_7      # taken from the existing per-product tests: 2.01 x 2**-24 |a b|
from train_ops_scale_cases import F24, PATTERN_MAX, pattern

NAN = float("nan")
F32E = 3                      # _abi.F32E (the CPU test compares)
FORMS = [(False, False), (False, True), (True, False), (True, True)]
NN, NT, TN, TT = FORMS
U = 2.0 ** -23                # unit of the arithmetic bounds


def bound_factor(kernel, k):
    """B(K) of the arithmetic cases, in units of 2**-23 (|A| |B|)_ij.  Derived from the number format, not measured.

    exact: K + 2.  A length-K dot product in f32 takes K - 1 additions and K products, each with a relative error of at most u; the a-priori
    bound is gamma_K sum |a| |b| ~ K u sum |a| |b| (Higham, Accuracy and Stability, 3.5).  u is taken as 2**-23, a whole ulp rather than
    half of one: the rounding mode inside v_mfma_f32_32x32x2_f32 is not documented, truncation doubles u.  + 2 covers the second-order
    terms of gamma_K (K u << 1) and the epilogue's alpha product.

    emulated: 1.05 K + 3.  The splits are exact (a = a0 + a1 + a2, |a1| <= 2**-8 |a|, |a2| <= 2**-16 |a|).  The K leading products a0 b0 go into
    one f32 accumulator like the exact kernel's: K (1 + 2**-8)**2 <= 1.008 K.  The 6 K small products go into the second; per k they sum to at most
    (2 x 2**-8 + 3 x 2**-16 + 2**-24) |a| |b| <= 2.02 x 2**-8 |a| |b|, so their accumulation adds at most 6 K x 2.02 x 2**-8 = 0.047 K (the issue
    counts 6 K 2**-8 = 0.023 K).  The dropped products and the one add that joins the two accumulators are PER_PRODUCT_7 x 2**-24 = 1.005 x 2**-23
    of |a| |b| per product, i.e. 1.005 of the sum.  Together 1.055 K + 1.005 <= 1.05 K + 3 - 1.6 for the K <= 70 used here: 0.005 K <= 0.35, the
    rest of the + 3 covers second-order terms and alpha as above."""
    assert k <= 70
    if kernel == "exact":
        return k + 2.0
    return 1.05 * k + 3.0


def ceil4(v):
    return (v + 3) // 4 * 4


class Lay:
    """One operand in memory: `off` elements from a 16-byte aligned allocation to matrix (0, 0); element strides of the outer and the inner batch
    index and of a row (ld); the last stride is 1.  dims3: handed to hip.bgemm as a 3-dim tensor (shared over the outer index, so = 0)."""

    def __init__(self, off, so, si, ld, dims3=False):
        self.off, self.so, self.si, self.ld, self.dims3 = off, so, si, ld, dims3
        assert not dims3 or so == 0

    def key(self):
        return (self.off, self.so, self.si, self.ld)

    def vec_props(self):
        """The properties the 16-byte path needs to be zero, by name."""
        return {"ptr": self.off % 4, "s_outer": self.so % 4, "s_inner": self.si % 4, "ld": self.ld % 4}

    def __repr__(self):
        return f"off{self.off}/so{self.so}/si{self.si}/ld{self.ld}" + ("/3d" if self.dims3 else "")


def lay(kind, O, I, rows, cols):
    """Named layouts of an (O, I, rows, cols) operand."""
    name, arg = kind if isinstance(kind, tuple) else (kind, None)
    if isinstance(name, Lay):
        return name
    if name == "pad4":        # rows padded to a multiple of 4 floats: the 16-byte path, a straddling last piece when cols % 4 != 0
        ld = ceil4(cols)
        return Lay(0, I * rows * ld, rows * ld, ld)
    if name == "gap4":        # pad4 with `arg` floats of slack between the matrices as well
        ld = ceil4(cols)
        return Lay(0, I * (rows * ld + arg) + arg, rows * ld + arg, ld)
    if name == "tight":       # contiguous: the 16-byte path iff cols % 4 == 0 (and then every stride is)
        return Lay(0, I * rows * cols, rows * cols, cols)
    if name == "off1":        # one float off a 16-byte boundary, ld = cols + 1: element loads
        return Lay(1, I * rows * (cols + 1), rows * (cols + 1), cols + 1)
    if name == "perm":        # the (B, H, T, d) permutation of a (B, T, H, d) tensor, d = arg >= cols
        return Lay(0, rows * I * arg, arg, I * arg)
    if name == "shared":      # one set of I matrices for every outer index: a 3-dim tensor, outer stride 0
        ld = ceil4(cols)
        return Lay(0, 0, rows * ld, ld, dims3=True)
    if name == "roomy":       # aligned, with room for any ONE stride to grow by 2 (LOSE_VEC below) without matrices overlapping
        ld = ceil4(cols) + 4
        si = ceil4(rows * (ld + 2)) + 4
        return Lay(0, ceil4(I * (si + 2)) + 4, si, ld)
    raise KeyError(name)


class Case:
    def __init__(self, group, name, kernel, batch, m, n, k, form, la="pad4", lb="pad4", lc="tight", gen="small", alpha=1.0, acc=0, tile=0,
                 expect=None, note=""):
        self.group, self.name, self.kernel = group, name, kernel
        (self.O, self.I), self.m, self.n, self.k = batch, m, n, k
        self.ta, self.tb = form
        self.gen, self.alpha, self.acc, self.tile, self.expect, self.note = gen, alpha, acc, tile, expect, note
        self.exact = gen != "arith"
        self.a_rc = (k, m) if self.ta else (m, k)
        self.b_rc = (n, k) if self.tb else (k, n)
        self.la, self.lb, self.lc = lay(la, self.O, self.I, *self.a_rc), lay(lb, self.O, self.I, *self.b_rc), lay(lc, self.O, self.I, m, n)
        self.id = f"{group}/{kernel}/{name}/{'NT'[self.ta]}{'NT'[self.tb]}"
        # operand values depend on shape, form and generator only: cases that differ in layout or tile see the same numbers
        self.seed = zlib.crc32(repr((group, batch, m, n, k, form, gen)).encode()) % 100003

    # ---- shapes of the tensors in memory
    def a_shape(self):
        return (1 if self.la.dims3 else self.O, self.I) + self.a_rc

    def b_shape(self):
        return (1 if self.lb.dims3 else self.O, self.I) + self.b_rc

    def c_shape(self):
        return (self.O, self.I, self.m, self.n)

    @functools.cached_property
    def data(self):
        """(a, b) as CPU f32 tensors of a_shape() / b_shape(): every matrix of the batch has its own values."""
        g = torch.Generator().manual_seed(self.seed)
        sa, sb = self.a_shape(), self.b_shape()
        if self.gen == "small":
            return (torch.randint(-4, 5, sa, generator=g).float(), torch.randint(-4, 5, sb, generator=g).float())
        if self.gen == "odd16":
            sign = lambda s: torch.randint(0, 2, s, generator=g) * 2 - 1  # noqa: E731
            a = (2 * torch.randint(128, 32768, sa, generator=g) + 1) * sign(sa)          # odd, 257 .. 65 535
            b = (torch.randint(1, 3, sb, generator=g)) * sign(sb)
            return a.float(), b.float()
        if self.gen == "arith":
            def rnd(s):
                mant = 1.0 + torch.rand(s, generator=g, dtype=torch.float64)
                e = torch.randint(-6, 7, s, generator=g).double()
                return (mant * 2.0 ** e).float()      # (the float64 significand rounds to f32's 24 bits here)
            return rnd(sa), rnd(sb)
        raise KeyError(self.gen)

    def _prod(self, a, b):
        a = a.transpose(-1, -2) if self.ta else a
        b = b.transpose(-1, -2) if self.tb else b
        return (a @ b).expand(self.c_shape())

    @functools.cached_property
    def ref(self):
        """op(A) op(B) in float64 (integer cases: exact, every value is an integer far below 2**53), WITHOUT alpha and the start pattern."""
        a, b = self.data
        return self._prod(a.double(), b.double())

    @functools.cached_property
    def absref(self):
        """(|A| |B|)_ij in float64: the integer cases' precondition, the arithmetic cases' unit."""
        a, b = self.data
        return self._prod(a.double().abs(), b.double().abs())

    @functools.cached_property
    def ref32(self):
        """The same product accumulated in f32 (torch on the CPU): the reference side's own check of the arithmetic bound."""
        a, b = self.data
        return self._prod(a, b)

    def start(self):
        """What C holds before the call where the kernel accumulates: train_ops_scale_cases.pattern, never zeros."""
        return pattern(self.c_shape()).double()

    def expected(self):
        """Integer cases: C after the call(s), float64.  acc = 0: one overwriting call; acc = 1 / 2: that many accumulating calls onto start()."""
        if self.acc == 0:
            return self.alpha * self.ref
        return self.start() + self.acc * self.alpha * self.ref

    def magnitude(self):
        """Largest |partial sum| any order can reach, in units of the smallest step of the values involved (1, or |alpha| < 1): < 2**24 = exact."""
        unit = min(abs(self.alpha), 1.0)
        return float(((PATTERN_MAX if self.acc else 0) + max(self.acc, 1) * abs(self.alpha) * self.absref).max()) / unit

    def bound(self):
        """Arithmetic cases: the elementwise bound on |c - ref|."""
        return bound_factor(self.kernel, self.k) * U * self.absref

    def criterion(self):
        if self.exact:
            return "torch.equal(int product)" + (f" gen={self.gen}" if self.gen != "small" else "")
        return f"|c-ref| <= {bound_factor(self.kernel, self.k):.2f} x 2^-23 (|A||B|)ij"


def place(layout, shape, values=None, device="cpu"):
    """-> (flat buffer, view of `shape` into it).  The buffer is NaN wherever the view does not reach (`values` None: everywhere).  The allocation is
    16-byte aligned (torch's allocators align to 64 bytes and more; the GPU test asserts data_ptr() % 16), so the view starts 4 * off bytes past a boundary."""
    o, i, rows, cols = shape
    size = layout.off + layout.so * (o - 1) + layout.si * (i - 1) + rows * layout.ld + 8
    buf = torch.full((size,), NAN, dtype=torch.float32, device=device)
    view = buf[layout.off:].as_strided(shape, (layout.so, layout.si, layout.ld, 1))
    if values is not None:
        view.copy_(values.to(device=device, dtype=torch.float32))
    return buf, view


def covered(layout, shape):
    """Flat indices of the buffer that the view covers, in view order (the CPU test: all distinct, NaN exactly elsewhere)."""
    o, i, rows, cols = shape
    size = layout.off + layout.so * (o - 1) + layout.si * (i - 1) + rows * layout.ld + 8
    return torch.arange(size)[layout.off:].as_strided(shape, (layout.so, layout.si, layout.ld, 1)).reshape(-1), size


def is_vec(c):
    """16-byte loads: both operand pointers on a 16-byte boundary and all of sa_outer, sa_inner, sb_outer, sb_inner, lda, ldb = 0 mod 4."""
    return all(v == 0 for lay_ in (c.la, c.lb) for v in lay_.vec_props().values())


def branch(c):
    """(kernel, WNF, BK, MF, vec, AK, BKC): jatts_bgemm's and bgemm_emul_launch's choice, restated."""
    vec = is_vec(c)
    n_batch = c.O * c.I
    n128, n64 = (c.n + 127) // 128 * 128, (c.n + 63) // 64 * 64
    tile = 3 if 128 < c.n <= 192 else (1 if n64 * 4 <= n128 * 3 else 2)
    wg128 = n_batch * ((c.m + 127) // 128) * ((c.n + 191) // 192)
    half_m = c.m > 64 and wg128 < 1024
    ak, bkc = not c.ta, c.tb
    if c.kernel == "exact":
        if not vec:
            wnf, bk, mf = (3, 16, 1) if tile == 3 else (2, 16, 2)
        elif tile == 3:
            wnf, bk, mf = 3, 16, 1 if half_m else 2
        else:
            wnf, bk, mf = tile, 32, 2
        return ("exact", wnf, bk, mf, vec, ak, bkc)
    wnf = tile
    mf = 1 if (wnf == 3 and half_m) or (wnf == 3 and not vec) else 2
    if c.tile:
        wnf, mf = c.tile & 15, c.tile >> 4
    assert (wnf, mf) in ((1, 2), (2, 2), (3, 2), (3, 1)), "bgemm_emul: no such tile"
    return ("emul", wnf, 32, mf, vec, ak, bkc)


# ------------------------------------------------------------------------------------------------------------------------------ the table
# launch classes (WNF, BK, MF, vec) -> the smallest (m, n, layout, forced tile) that reaches each; x four forms = the instantiations
EXACT_CLASSES = {
    "v64": ((1, 32, 2, True), 70, 48, "pad4", 0),        # n <= 64: P v at every small d_k
    "v128": ((2, 32, 2, True), 70, 100, "pad4", 0),
    "v192h": ((3, 16, 1, True), 130, 132, "pad4", 0),    # 64-row tiles by half_m
    "v192": ((3, 16, 2, True), 64, 132, "pad4", 0),      # 128-row tiles by m <= 64 (by count: COUNT below)
    "e192h": ((3, 16, 1, False), 70, 132, "off1", 0),
    "e128": ((2, 16, 2, False), 70, 100, "off1", 0),
}
EMUL_CLASSES = {
    "v64": ((1, 32, 2, True), 70, 48, "pad4", 0),
    "v128": ((2, 32, 2, True), 70, 100, "pad4", 0),
    "v192": ((3, 32, 2, True), 64, 132, "pad4", 0),
    "v192h": ((3, 32, 1, True), 130, 132, "pad4", 0),
    "e64": ((1, 32, 2, False), 70, 48, "off1", 0),
    "e128": ((2, 32, 2, False), 70, 100, "off1", 0),
    "e192h": ((3, 32, 1, False), 70, 132, "off1", 0),
    "e192": ((3, 32, 2, False), 64, 132, "off1", 3 | 2 << 4),      # the dispatcher never chooses it: forced
}
CLASSES = {"exact": EXACT_CLASSES, "emul": EMUL_CLASSES}
ALL_BRANCHES = sorted((kern, w, bk, mf, vec, ak, bkc) for kern, cl in CLASSES.items() for (w, bk, mf, vec), *_ in cl.values()
                      for ak in (False, True) for bkc in (False, True))

M_EDGES = [1, 63, 64, 65, 127, 128, 129]
N_EDGES = [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 257]
BATCHES = [(1, 1), (7, 1), (1, 8), (3, 3), (17, 1), (5, 7), (2, 48)]
LOSE_VEC = ["a.ptr", "b.ptr", "a.s_outer", "a.s_inner", "a.ld", "b.s_outer", "b.s_inner", "b.ld"]
BITS_TILES = [1 | 2 << 4, 2 | 2 << 4, 3 | 2 << 4, 3 | 1 << 4]


def k_edges(bk):
    return [1, bk - 1, bk, bk + 1, 2 * bk, 2 * bk + 1, 3 * bk + 5]


def int_gen(kernel, k):
    """odd16 wherever its K <= 64 precondition allows it on the emulated kernel; the geometry generator otherwise."""
    return "odd16" if kernel == "emul" and k <= 64 else "small"


def lose(base, what):
    o, so, si, ld = base.key()
    return {"ptr": Lay(1, so, si, ld), "s_outer": Lay(o, so + 2, si, ld), "s_inner": Lay(o, so, si + 2, ld), "ld": Lay(o, so, si, ld + 2)}[what]


def _build():
    cases = []
    add = lambda *a, **kw: cases.append(Case(*a, **kw))  # noqa: E731
    for kern, classes in CLASSES.items():
        # 1. every instantiation: one integer case (K = 20: two 16-deep chunks with a tail, one partial 32-deep chunk) and one arithmetic case (K = 8) per
        #    form; K = 1 and K = 33 in the two forms that between them put each operand on each commit path
        for name, (cls, m, n, layout, tile) in classes.items():
            for form in FORMS:
                add("inst", name + "-int", kern, (1, 2), m, n, 20, form, layout, layout, gen=int_gen(kern, 20), tile=tile, expect=cls)
                add("inst", name + "-k8", kern, (1, 2), m, n, 8, form, layout, layout, gen="arith", tile=tile, expect=cls)
            for form in (NT, TN):
                for k in (1, 33):
                    add("inst", f"{name}-k{k}", kern, (1, 2), m, n, k, form, layout, layout, gen="arith", tile=tile, expect=cls)
        # the 128 x 192 tile on the dispatcher's own route: 1024 workgroups of 128-row tiles; one matrix fewer goes back to 64 rows
        bk = 16 if kern == "exact" else 32
        for form in (FORMS if kern == "exact" else [NT]):
            add("count", "1024", kern, (128, 8), 65, 132, 20, form, gen=int_gen(kern, 20), expect=(3, bk, 2, True))
        add("count", "1023", kern, (341, 3), 65, 132, 20, NT, gen=int_gen(kern, 20), expect=(3, bk, 1, True))
        # three 128-wide tiles: the Gaussian upsampling's n = adim
        for form in FORMS:
            add("inst", "adim384", kern, (1, 2), 70, 384, 20, form, gen=int_gen(kern, 20), expect=(2, 32, 2, True))
        # 2. M and N edges: rows padded to 4 floats (16-byte path, K = 9 straddles) and contiguous (K = 8: 16-byte path iff the long dimension % 4 == 0)
        for layout, k in (("pad4", 9), ("tight", 8)):
            for form in (NN, TT):
                for m in M_EDGES:
                    add("medge", f"{layout}-m{m}", kern, (1, 2), m, 65, k, form, layout, layout, gen=int_gen(kern, k))
                for n in N_EDGES:
                    add("nedge", f"{layout}-n{n}", kern, (1, 2), 65, n, k, form, layout, layout, gen=int_gen(kern, k))
        # 3. K edges per chunk depth: odd and even chunk counts, a tail after a buffer swap
        kcls = ([("bk16e", (2, 16, 2, False), 70, "off1"), ("bk16v", (3, 16, 1, True), 132, "pad4"), ("bk32v", (2, 32, 2, True), 70, "pad4")]
                if kern == "exact" else [("bk32v", (2, 32, 2, True), 70, "pad4"), ("bk32e", (2, 32, 2, False), 70, "off1")])
        for name, cls, n, layout in kcls:
            for k in k_edges(cls[1]):
                for form in FORMS:
                    add("kedge", f"{name}-k{k}", kern, (1, 2), 65, n, k, form, layout, layout, gen=int_gen(kern, k), expect=cls)
        # 4. the 16-byte piece that straddles the K edge (K = 5 in rows of 8: NT) or the row edge (m = 65 in rows of 68, n = 70 in 72: TN), NaN behind it;
        #    and NaN between the matrices
        for layout in ("pad4", ("gap4", 8)):
            for form in FORMS:
                add("straddle", layout if isinstance(layout, str) else "gap4", kern, (2, 2), 65, 70, 5, form, layout, layout, gen=int_gen(kern, 5),
                    expect=(2, 32, 2, True))
        # 5. each way to lose the 16-byte path, alone
        for form in FORMS:
            base = Case("losevec", "aligned", kern, (2, 2), 70, 70, 12, form, "roomy", "roomy", gen=int_gen(kern, 12),
                        expect=(2, 32, 2, True))
            cases.append(base)
            for what in LOSE_VEC:
                op, prop = what.split(".")
                la = lose(base.la, prop) if op == "a" else base.la
                lb = lose(base.lb, prop) if op == "b" else base.lb
                add("losevec", what, kern, (2, 2), 70, 70, 12, form, la, lb, gen=int_gen(kern, 12),
                    expect=(2, 16 if kern == "exact" else 32, 2, False))
        # 6. batch index: two tiles per matrix (m = 130 in 128-row tiles), so mloc / tiles and mloc % tiles both vary
        for batch in BATCHES:
            b = "b%dx%d" % batch
            add("batch", b + "-perm12", kern, batch, 130, 70, 9, NT, ("perm", 12), ("perm", 12), gen=int_gen(kern, 9),
                expect=(2, 32, 2, True), note="q k^T on (B, H, T, d) permutations of (B, T, H, 12)[..., :9]")
            add("batch", b + "-shared", kern, batch, 130, 70, 9, NT, "pad4", "shared", gen=int_gen(kern, 9), expect=(2, 32, 2, True),
                note="q p^T: B shared over the outer index")
            add("batch", b + "-perm27", kern, batch, 130, 70, 27, NN, ("perm", 27), ("gap4", 8), gen=int_gen(kern, 27),
                expect=(2, 16 if kern == "exact" else 32, 2, False), note="A permuted with the odd d_k = 27, B a 4-dim view with slack")
        # 7. store side.  alpha = 0.5 and -2 are exact; C contiguous or a view with ldc = n + 3 and slack between matrices, NaN around
        for form in (NT, TN):
            for alpha, acc in ((0.5, 0), (-2.0, 0), (0.5, 1), (-2.0, 1), (0.5, 2)):
                add("store", f"alpha{alpha}-acc{acc}", kern, (2, 2), 65, 70, 9, form, alpha=alpha, acc=acc)
        for m, n in ((64, 64), (65, 129), (128, 192), (129, 193)):
            lc = Lay(0, 2 * (m * (n + 3) + 5) + 7, m * (n + 3) + 5, n + 3)
            add("store", f"ldc-m{m}n{n}", kern, (2, 2), m, n, 9, NT, lc=lc)
        add("store", "ldc-acc1", kern, (2, 2), 65, 129, 9, NT, lc=Lay(0, 2 * (65 * 132 + 5) + 7, 65 * 132 + 5, 132), alpha=-2.0, acc=1)
    # 8. one bit pattern per output, whatever computed it: emulated kernel, arithmetic, K = 70, every forced tile on both load paths
    for form in FORMS:
        for layout in ("pad4", "off1"):
            for tile in BITS_TILES:
                add("bits", f"{layout}-w{tile & 15}m{tile >> 4}", "emul", (1, 2), 130, 70, 70, form, layout, layout, gen="arith", tile=tile,
                    expect=(tile & 15, 32, tile >> 4, layout == "pad4"))
    ids = [c.id for c in cases]
    assert len(set(ids)) == len(ids), "duplicate case id"
    return cases


CASES = _build()
BY_ID = {c.id: c for c in CASES}


def case_id(c):
    return c.id


def release(c):
    """Drop a case's cached tensors (the by-count cases hold 35 MB outputs)."""
    for attr in ("data", "ref", "absref", "ref32"):
        c.__dict__.pop(attr, None)
