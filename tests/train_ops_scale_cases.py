"""Case table of tests/test_train_ops_scale_{cpu,gpu}.py: the training kernels' cross-workgroup sums on small INTEGERS stored in f32.

Every term and every partial sum of a case is an integer (or a multiple of a power of two) below 2**24 -- 2**53 for the double outputs --
so the sum is exact in any order, with or without FMA, and the int64 sum of the same terms is the expected value to the last bit.
`reference(kernel, inputs)` returns, per output, (expected value as float64, sum of |terms| per output element, accumulates); the CPU
test proves the 2**24 precondition from the second, the GPU test compares the kernel with the first by torch.equal.  An accumulating
(`+=`) output starts from `pattern()`, never from zeros.

The shapes sit on both sides of every launcher threshold of csrc/train_ops.hip (profiles/r09_notes.md lists kernel -> case -> path)."""
import torch

F24, F53 = 2 ** 24, 2 ** 53
PATTERN_MAX = 3


def ints(shape, lo, hi, seed):
    return torch.randint(lo, hi + 1, tuple(shape), generator=torch.Generator().manual_seed(seed)).float()


def pattern(shape):
    """The non-zero integer pattern an accumulating output starts from (|p| <= PATTERN_MAX)."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    n = 1
    for v in shape:
        n *= v
    return ((torch.arange(n) % 7) - 3).float().view(shape)


def ragged(n_seq, max_len):
    """Lengths that mix 1 with the longest sequence: workgroups past a short sequence's end still deposit a zero slab and take a ticket."""
    return [max_len, 1] + [1 + (i * 197) % max_len for i in range(n_seq - 2)]


def cu_of(lens):
    cu = [0]
    for v in lens:
        cu.append(cu[-1] + v)
    return cu


RECIPE_FRAMES = ragged(32, 768)

# rows x dim of the column reductions: gridDim.y = min(ceil(rows / 256), 256) -- one slab (1, 255, 256), two (257), 96 at the recipe's
# 24 576 frame rows, exactly 256 without a loop (65 536), capped and looping (65 836, 70 000); dims around the 64-channel tile
COL = [(1, 1), (255, 63), (256, 64), (257, 65), (513, 81), (4096, 1536), (24576, 384), (65536, 64), (65836, 5), (70000, 12)]
# LayerNorm launcher: 16 rows per workgroup, <= 512 workgroups (loop above 8 192 rows), first-level groups of 32 workgroups (two above 512
# rows, the last one ragged unless the workgroup count divides by 32); odd dim = the scalar slab path
LN = [(1, 81), (511, 384), (512, 384), (513, 81), (513, 384), (1040, 1536), (8176, 64), (8192, 65), (8208, 81), (24576, 384)]
# (B, T, H, d_k) of the Q|K|V split: 32 rows per workgroup up to 16 384 rows, 64 from 16 385 (16 416 -> 257 workgroups, 24 576 -> 384)
QKV = [(1, 1, 1, 1), (1, 513, 3, 27), (1, 1025, 2, 32), (32, 512, 2, 192), (32, 513, 3, 27), (32, 513, 2, 192), (32, 768, 2, 192)]
# (lens, dim): time splits = min(ceil(max_len / 64), 16), a loop above 1 024 steps
SEQ_SUM = [([1], 1), ([1, 1025, 64, 65], 65), ([1024, 1], 64), ([1025, 1, 1], 63), (RECIPE_FRAMES, 384), ([768] * 32, 81)]
# (lens, dim, k): tiled k = 7 / 31 (one tile per workgroup up to 512 steps, four from 513), generic k (time splits capped at 64: a loop
# above 4 096 steps)
DWCONV = [([50, 1], 1, 3), ([512, 1], 64, 7), ([513, 1], 65, 7), (RECIPE_FRAMES, 384, 7), ([512], 64, 31), ([513, 2], 81, 31),
          ([768, 1, 300], 63, 31), ([768] * 32, 384, 31), ([4096, 1], 64, 15), ([4100], 65, 15), ([1, 4100], 64, 3), (RECIPE_FRAMES, 384, 15)]
# n: 4 096 elements per workgroup, <= 1 024 workgroups
SUMSQ = [1, 4096, 4097, 4194304, 4194304 + 3]
# (source rows, destination rows, dim, scale): the index list goes through LDS in windows
INDEX_ADD = [(90, 20, 64, 1.0), (1025, 40, 65, 8.0), (3000, 40, 300, 0.5), (4096, 60, 384, 16.0)]
# (token lens, dim)
LR_SEG = [([1, 5], 8), ([1, 128, 64, 100], 81), ([128] * 32, 384)]
# (lens, c_in, n_out, k): the VALU weight gradient (k = 7 / 9) and the bias gradient that goes with it
CONV_WGRAD = [([40, 9], 1, 1, 7), ([1, 300, 77], 65, 63, 7), ([768] * 32, 80, 64, 9)]
# (B, T, dim): kind 1; the backward loops once T * dim > 65 536 (768 x 80 = 61 440 below, 1 000 x 80 above)
MLOSS = [(3, 14, 5), (32, 128, 1), (32, 768, 80), (32, 1000, 80)]

INT_CASES = {
    "col_sum": COL, "col_wsum": COL, "col_stats0": COL, "col_stats1": COL, "ln_dbeta": LN, "qkv_split_bwd": QKV, "seq_sum": SEQ_SUM,
    "dwconv_wgrad": DWCONV, "sumsq": SUMSQ, "index_add_rows": INDEX_ADD, "lr_segment_sum": LR_SEG, "conv1d_wgrad": CONV_WGRAD,
    "masked_loss1": MLOSS,
}
ALL_INT = [(k, c) for k, cases in INT_CASES.items() for c in cases]


def case_id(kc):
    k, c = kc
    if not isinstance(c, tuple):
        return f"{k}-{c}"
    return k + "-" + "x".join(f"r{len(v)}m{max(v)}" if isinstance(v, list) else str(v) for v in c)


def _seed(kernel, case):
    return sum(ord(ch) for ch in kernel + repr(case)) % 100003


def make(kernel, case):
    """The case's inputs as CPU tensors (f32 holding integers; int64 indices)."""
    s = _seed(kernel, case)
    if kernel in ("col_sum", "col_wsum", "col_stats0", "col_stats1"):
        rows, dim = case
        inp = {"x": ints((rows, dim), -3, 3, s)}
        if kernel == "col_sum":
            inp["x"] = ints((rows, dim), -4, 4, s)
        if kernel == "col_wsum":
            inp["x"], inp["v"] = ints((rows, dim), -4, 4, s), ints((rows,), -3, 3, s + 1)
        if kernel in ("col_stats0", "col_stats1"):
            inp["shift"] = None if (kernel == "col_stats0" and rows % 2) else ints((dim,), -1, 1, s + 2)       # |x - shift| <= 4
        if kernel == "col_stats1":
            inp["dy"], inp["mul"] = ints((rows, dim), -3, 3, s + 3), 2.0 ** ints((dim,), 0, 2, s + 4)
        return inp
    if kernel == "ln_dbeta":
        rows, dim = case
        return {"x": ints((rows, dim), -4, 4, s), "dy": ints((rows, dim), -3, 3, s + 1), "gamma": ints((dim,), 1, 2, s + 2)}
    if kernel == "qkv_split_bwd":
        B, T, H, dk = case
        return {n: ints((B, H, T, dk), -3, 3, s + i) for i, n in enumerate(("dqu", "dqv", "dk", "dvv"))}
    if kernel == "seq_sum":
        lens, dim = case
        return {"lens": lens, "x": ints((sum(lens), dim), -4, 4, s)}
    if kernel == "dwconv_wgrad":
        lens, dim, k = case
        return {"lens": lens, "k": k, "pad": (k - 1) // 2, "x": ints((sum(lens), dim), -4, 4, s), "dy": ints((sum(lens), dim), -3, 3, s + 1)}
    if kernel == "sumsq":
        return {"x": ints((case,), -4, 4, s), "start": 5.0}
    if kernel == "index_add_rows":
        rows, n_dst, dim, scale = case
        idx = torch.randint(-1, n_dst + 1, (rows,), generator=torch.Generator().manual_seed(s + 1))     # -1 and n_dst: out of range, dropped
        idx[idx == n_dst // 2] = n_dst // 2 + 1                                                       # row n_dst // 2 is never touched
        return {"src": ints((rows, dim), -4, 4, s), "idx": idx, "n_dst": n_dst, "scale": scale, "skip": 0, "untouched": [0, n_dst // 2]}
    if kernel == "lr_segment_sum":
        lens, dim = case
        d = torch.randint(0, 13, (sum(lens),), generator=torch.Generator().manual_seed(s + 1))
        cu = cu_of(lens)
        cum = torch.cat([d[cu[b]:cu[b + 1]].cumsum(0) for b in range(len(lens))])
        to = max(max(int(cum[cu[b + 1] - 1]) for b in range(len(lens))) - 3, 1)     # the longest sequence is cut short, the others padded
        return {"lens": lens, "cum": cum, "to": to, "dy": ints((len(lens) * to, dim), -3, 3, s)}
    if kernel == "conv1d_wgrad":
        lens, c_in, n_out, k = case
        return {"lens": lens, "k": k, "pad": (k - 1) // 2, "x": ints((sum(lens), c_in), -4, 4, s), "dy": ints((sum(lens), n_out), -3, 3, s + 1)}
    if kernel == "masked_loss1":
        B, T, dim = case
        return {"B": B, "T": T, "valid": ragged(B, T)[:B] if B > 2 else [T, 1][:B], "a": ints((B * T, dim), -1, 1, s), "b": ints((B * T, dim), -1, 1, s + 1),
                "scale": 2.0 ** -12, "up": 2.0}
    raise KeyError(kernel)


def _shifted(x, lens, off):
    """rows of x moved by `off` steps inside each sequence (x[t + off], zero outside the sequence)."""
    out = torch.zeros_like(x)
    o = 0
    for n in lens:
        lo, hi = max(0, -off), min(n, n - off)
        if hi > lo:
            out[o + lo:o + hi] = x[o + lo + off:o + hi + off]
        o += n
    return out


def reference(kernel, inp):
    """{output: (expected float64 tensor WITHOUT the start pattern, sum of |terms| per element as float64, accumulates)}: int64 sums (fp64
    matrix products where noted: exact, every value is an integer far below 2**53)."""
    L = lambda t: t.long()  # noqa: E731
    D = lambda t: t.double()  # noqa: E731
    if kernel == "col_sum":
        x = L(inp["x"])
        return {"out": (D(x.sum(0)), D(x.abs().sum(0)), True)}
    if kernel == "col_wsum":
        t = L(inp["v"])[:, None] * L(inp["x"])
        return {"out": (D(t.sum(0)), D(t.abs().sum(0)), True)}
    if kernel == "col_stats0":
        v = L(inp["x"]) - (L(inp["shift"]) if inp["shift"] is not None else 0)
        return {"o0": (D(v.sum(0)), D(v.abs().sum(0)), True), "o1": (D((v * v).sum(0)), D((v * v).sum(0)), True)}
    if kernel == "col_stats1":
        dy = L(inp["dy"])
        t = dy * (L(inp["x"]) - L(inp["shift"])) * L(inp["mul"])
        return {"o0": (D(dy.sum(0)), D(dy.abs().sum(0)), True), "o1": (D(t.sum(0)), D(t.abs().sum(0)), True)}
    if kernel == "ln_dbeta":
        dy = L(inp["dy"])
        return {"db": (D(dy.sum(0)), D(dy.abs().sum(0)), True)}
    if kernel == "qkv_split_bwd":
        B, H, T, dk = inp["dqu"].shape
        rows = lambda t: L(t).permute(0, 2, 1, 3).reshape(B * T, H * dk)  # noqa: E731
        qu, qv, k, v = (rows(inp[n]) for n in ("dqu", "dqv", "dk", "dvv"))
        dqkv = torch.cat([qu + qv, k, v], dim=1)
        return {"dqkv": (D(dqkv), D(dqkv.abs()), False), "du": (D(qu.sum(0)), D(qu.abs().sum(0)), True),
                "dv": (D(qv.sum(0)), D(qv.abs().sum(0)), True)}
    if kernel == "seq_sum":
        x, cu = L(inp["x"]), cu_of(inp["lens"])
        val = torch.stack([x[cu[b]:cu[b + 1]].sum(0) for b in range(len(inp["lens"]))])
        bnd = torch.stack([x[cu[b]:cu[b + 1]].abs().sum(0) for b in range(len(inp["lens"]))])
        return {"out": (D(val), D(bnd), True)}
    if kernel == "dwconv_wgrad":
        x, dy, k, pad = L(inp["x"]), L(inp["dy"]), inp["k"], inp["pad"]
        val, bnd = [], []
        for j in range(k):
            t = dy * _shifted(x, inp["lens"], j - pad)
            val.append(t.sum(0))
            bnd.append(t.abs().sum(0))
        return {"dw": (D(torch.stack(val, 1)), D(torch.stack(bnd, 1)), True)}
    if kernel == "sumsq":
        v = (L(inp["x"]) ** 2).sum()
        return {"out": (D(v), D(v), True)}
    if kernel == "index_add_rows":
        idx, n_dst = inp["idx"], inp["n_dst"]
        ok = (idx >= 0) & (idx < n_dst) & (idx != inp["skip"])
        t = D(inp["src"])[ok] * inp["scale"]                     # (a power-of-two scale: exact)
        z = torch.zeros(n_dst, inp["src"].shape[1], dtype=torch.float64)
        unit = min(inp["scale"], 1.0)                            # (terms are multiples of `unit`: the bound counts in units)
        return {"dst": (z.clone().index_add_(0, idx[ok], t), z.clone().index_add_(0, idx[ok], t.abs() / unit), True)}
    if kernel == "lr_segment_sum":
        lens, to, dy, cum = inp["lens"], inp["to"], L(inp["dy"]), inp["cum"]
        cu, val, bnd = cu_of(lens), [], []
        for b in range(len(lens)):
            seg = dy[b * to:(b + 1) * to]
            zero = torch.zeros(1, seg.shape[1], dtype=torch.int64)
            P, Pa = torch.cat([zero, seg.cumsum(0)]), torch.cat([zero, seg.abs().cumsum(0)])
            hi = cum[cu[b]:cu[b + 1]].clamp(max=to)
            lo = torch.cat([torch.zeros(1, dtype=torch.int64), hi[:-1]])
            val.append(P[hi] - P[lo])
            bnd.append(Pa[hi] - Pa[lo])
        return {"dhs": (D(torch.cat(val)), D(torch.cat(bnd)), False)}
    if kernel == "conv1d_wgrad":
        x, dy, k, pad = D(inp["x"]), D(inp["dy"]), inp["k"], inp["pad"]
        val = torch.stack([dy.t() @ _shifted(x, inp["lens"], j - pad) for j in range(k)], 2)             # fp64 products of integers: exact
        bnd = torch.stack([dy.abs().t() @ _shifted(x, inp["lens"], j - pad).abs() for j in range(k)], 2)
        return {"dw": (val, bnd, False), "db": (dy.sum(0), dy.abs().sum(0), False)}
    if kernel == "masked_loss1":
        B, T = inp["B"], inp["T"]
        m = (torch.arange(T)[None, :] < torch.tensor(inp["valid"])[:, None]).reshape(-1, 1).long()
        dlt = (L(inp["a"]) - L(inp["b"])) * m
        s = (dlt * dlt).sum()
        da = D(dlt) * (2.0 * inp["up"] * inp["scale"])
        return {"loss": (D(s) * inp["scale"], D(s), False), "da": (da, D(dlt.abs()) * 2.0 * inp["up"], False)}
    raise KeyError(kernel)


def limit(kernel, name):
    return F53 if kernel == "sumsq" else F24
