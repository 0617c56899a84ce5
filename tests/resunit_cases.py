"""Case tables, dispatcher model and CPU references of tests/test_resunit_cases_{cpu,gpu}.py: the TWO-CONV fused HiFi-GAN dilation unit
(jatts_hifigan_resunit with w2 != NULL) and the fused ResBlock (jatts_hifigan_resblock) on small dyadic numbers on which every arithmetic is EXACT.

    a = lrelu(x),  h = conv_{k,d}(a; w1) + b1 inside the utterance and ZERO outside it,
    g = lrelu(h),  y = x + conv_{k,1}(g; w2) + b2,            all halo rows outside the utterance read as zero
    block: x <- unit_d(x) for d in dils;   MRF store pass: y <- out_scale (y + add0 [+ add1])

Three things live here (pure data and CPU functions: nothing touches the GPU or the library; profiles/r34_notes.md lists kernel -> case -> tests):

  * tile_of(): a host model of the dispatchers (csrc/resunit_*.hip, csrc/resblock_*.hip and the launchers' refusals), restated with the expressions
    the sources use.  It names the kernel instantiation a launch takes, its window width WGCOLS, the outputs per window tt_out and the form
    (windowed / sliding).  tests/test_resunit_cases_cpu.py holds its instantiation set equal to the `launch_*<...>` lists of the sources.
  * the operands.  LeakyReLU slopes are powers of two (0.5; 0 for the f16 blocks), x holds small integers whose negative values are even,
    the weights hold exactly `m` values of +-1 / +-2 in every (c_in, tap) column -- one per output channel a column reaches, dealt out by a
    permutation per tap, so every output channel sums exactly m k products per conv -- and the biases and MRF partners are small integers.  Every
    staged value is then a dyadic number a few bits wide; preconditions() proves from the float64 intermediates of the reference that no arithmetic
    rounds anywhere, so the float64 result is the expected output to the last bit and check_exact (conv_geometry_cases) compares without a tolerance.
  * CASES: every instantiation the model can return is launched by a case, with lengths around each launched window's tt_out (tt - 1, tt, tt + 1,
    2 tt - 1, 2 tt, 2 tt + 1), utterances of 1 and 2 rows and one below the per-side halo between the long ones, and one of three windows or more.
"""
import collections
import functools
import os
import re

import torch
import torch.nn.functional as F

from conv_geometry_cases import _gen, check_exact  # noqa: F401  (check_exact: the comparison of the GPU tests)

F24 = 2 ** 24
KIB = 1024
LDS_MAX = 160 * KIB
CUS = 256                        # compute units of the MI355X (the GPU tests pass the device's own count)
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "jatts_amd", "csrc")

# arithmetic spec -> (dtype name in jatts_amd.hip, w_layout, arithmetic class).  The w_layout 1 units run as variant 1 (windowed), 2 (sliding) and 0.
SPECS = {
    "f32": ("F32", 0, "f32"), "f16": ("F16", 0, "f16"), "f32s": ("F32S", 0, "f32"),
    "e7w0": ("F32E", 0, "f32"), "e6w0": ("F32E6", 0, "f32"), "e7w1": ("F32E", 1, "f32"), "e6w1": ("F32E6", 1, "f32"),
}
UNIT_SPECS = ("f32", "f16", "f32s", "e7w0", "e6w0", "e7w1", "e6w1")
BLOCK_SPECS = ("f32", "f16", "f32s", "e7w0", "e6w0")       # (the emulated ResBlocks are 32 x 32 x 16 kernels: w_layout 0 weights)


# ------------------------------------------------------------------------------------------ the dispatchers, restated
Tile = collections.namedtuple("Tile", "file launcher args wgcols tt_out sliding")


def _tile(file, launcher, args, lose, sliding=False):
    """`args`: the template-argument list as the source spells it.  WGCOLS follows the channel count; a window stores WGCOLS - lose columns."""
    parts = [p.strip() for p in args.split(",")]
    i = 1 if parts[0].isdigit() else 2
    wgcols = int(parts[i])
    return Tile(file, launcher, ", ".join(parts), wgcols, wgcols - lose, sliding)


def _unit_lds(wgcols, C, k, dil, elem, extra, pitch_x=None):
    """launch_resunit*: (rows_x > rows_h ? rows_x : rows_h) * pitch + biases (h overlays x); emulated: rows_x * pitch_x against rows_h * pitch."""
    p2 = (k - 1) // 2
    p1 = p2 * dil
    pitch = C * elem + 16
    rows_x, rows_h = wgcols + 2 * p1, wgcols + k - 1
    region = max(rows_x * (pitch_x or pitch), rows_h * pitch)
    return region + extra


def _unit_f32(C, k, dil):
    halo = (k - 1) * dil
    f = "resunit_f32.hip"
    if C == 32:
        return _tile(f, "launch_resunit", "float, 32, 512, 1, 4, 8, 2, true", k - 1)
    if C == 64:
        return _tile(f, "launch_resunit", "float, 64, 256, 1, 2, 8, 2, true", k - 1)
    if C == 128:
        if (128 + halo) * 528 + 1024 <= 80 * 1024:
            return _tile(f, "launch_resunit", "float, 128, 128, 2, 2, 8, 2, true" if k <= 7 else "float, 128, 128, 2, 2, 8, 2", k - 1)
        return _tile(f, "launch_resunit", "float, 128, 256, 2, 2, 8, 2", k - 1)
    if C == 256:
        if (128 + halo) * 1040 + 2048 <= 160 * 1024:
            return _tile(f, "launch_resunit", "float, 256, 128, 4, 4, 8, 1", k - 1)
        return _tile(f, "launch_resunit", "float, 256, 96, 4, 3, 8, 1, true", k - 1)
    return None


def _unit_f16(C, k, dil):
    if C == 32:
        return _tile("resunit_f16_narrow.hip", "launch_resunit", "f16, 32, 512, 1, 4, 2" if k > 7 else "f16, 32, 256, 1, 2", k - 1)
    if C == 64:
        return _tile("resunit_f16_narrow.hip", "launch_resunit", "f16, 64, 512, 1, 4, 4" if k > 3 else "f16, 64, 256, 1, 2", k - 1)
    f = "resunit_f16_wide.hip"
    if C == 128:
        if ((256 + (k - 1) * dil) * 272 + 1024) * 2 > 160 * 1024:
            return _tile(f, "launch_resunit", "f16, 128, 192, 2, 3, 4", k - 1)
        return _tile(f, "launch_resunit", "f16, 128, 256, 2, 4, 4", k - 1)
    if C == 256:
        return _tile(f, "launch_resunit", "f16, 256, 128, 4, 4, 4", k - 1)
    if C == 512:
        return _tile(f, "launch_resunit", "f16, 512, 32, 4, 1", k - 1)
    return None


def _unit_split(C, k, dil):
    halo = (k - 1) * dil
    f = "resunit_split.hip"
    if C == 32:
        return _tile(f, "launch_resunit_split", "32, 256, 1, 2, 2, 2", k - 1)
    if C == 64:
        return _tile(f, "launch_resunit_split", "64, 256, 1, 2, 2, 2", k - 1)
    if C == 128:
        if (128 + halo) * 528 + 2048 + 64 <= 80 * 1024:
            return _tile(f, "launch_resunit_split", "128, 128, 2, 2, 4, 2", k - 1)
        return _tile(f, "launch_resunit_split", "128, 256, 2, 2, 4, 1", k - 1)
    if C == 256:
        if (128 + halo) * 1040 + 4096 + 64 <= 160 * 1024:
            return _tile(f, "launch_resunit_split", "256, 128, 4, 4, 2, 1", k - 1)
        return _tile(f, "launch_resunit_split", "256, 96, 4, 3, 2, 1", k - 1)
    return None


def _unit_emul(C, k, dil, n_seq, max_len, len_mul):
    """resunit_emul (w_layout 0, 32 x 32 x 16): C = 128 / 256 choose the window from the launch size."""
    halo = (k - 1) * dil
    cols = max_len * len_mul

    def wgs(window):
        tt = window - (k - 1)
        return -(-cols // tt) * n_seq if tt > 0 else 1 << 40
    f = "resunit_emul.hip"
    if C == 32:
        return _tile(f, "launch_resunit_emul", "T, 32, 256, 1, 2, 2, 2, false, true", k - 1)
    if C == 64:
        if k >= 11:
            return _tile(f, "launch_resunit_emul", "T, 64, 256, 1, 2, 2, 1, false, true", k - 1)
        return _tile(f, "launch_resunit_emul", "T, 64, 128, 2, 2, 2, 2, false, true", k - 1)
    if C == 128:
        if wgs(128) <= 448 and (64 + halo) * 784 + 1024 <= 80 * 1024:
            return _tile(f, "launch_resunit_emul", "T, 128, 64, 2, 1, 2, 2", k - 1)
        return _tile(f, "launch_resunit_emul", "T, 128, 128, 2, 2, 2, 1", k - 1)
    if C == 256:
        if wgs(64) <= 160:
            return _tile(f, "launch_resunit_emul", "T, 256, 32, 4, 1, 2, 1", k - 1)
        if (64 + halo) * 1552 + 2048 <= 160 * 1024:
            return _tile(f, "launch_resunit_emul", "T, 256, 64, 4, 2, 2, 1", k - 1)
        return _tile(f, "launch_resunit_emul", "T, 256, 64, 4, 2, 2, 1, true", k - 1)
    return None


def _unit_emul16(C, k, dil):
    halo = (k - 1) * dil
    f = "resunit_emul.hip"
    if C == 32:
        return _tile(f, "launch_resunit_emul16", "T, 32, 256, 1, 4, 2, false, true", k - 1)
    if C == 64:
        if k >= 11:
            return _tile(f, "launch_resunit_emul16", "T, 64, 256, 1, 4, 1, false, true", k - 1)
        return _tile(f, "launch_resunit_emul16", "T, 64, 128, 2, 2, 2, false, true", k - 1)
    if C == 128:
        return _tile(f, "launch_resunit_emul16", "T, 128, 128, 2, 2, 1", k - 1)
    if C == 256:
        if (64 + halo) * 1552 + 2048 <= 160 * 1024:
            return _tile(f, "launch_resunit_emul16", "T, 256, 64, 4, 1, 1", k - 1)
        return _tile(f, "launch_resunit_emul16", "T, 256, 64, 4, 1, 1, true", k - 1)
    return None


def resunit16_pick(variant, runs, wgcols, slide_auto, slide_fits, n_seq, max_len, total_rows, len_mul):
    """csrc/resunit_emul16_impl.h resunit16_pick: 1 = windowed, 2 = sliding.  total_rows > 0: the 1-D ragged geometry (host lengths)."""
    positions = total_rows * len_mul if total_rows > 0 else n_seq * max_len * len_mul
    slide = variant == 2 or (variant == 0 and slide_auto and positions >= 2 * runs * wgcols)
    return 2 if slide and slide_fits else 1


def _flags(tile):
    """(KSPLIT, RREG) of an emulated unit instantiation: its last two template arguments, where spelled."""
    parts = tile.args.split(", ")
    n = 7 if tile.launcher == "launch_resunit_emul" else 6      # arguments before KSPLIT
    return (len(parts) > n and parts[n] == "true", len(parts) > n + 1 and parts[n + 1] == "true")


def _block_geometry(k, dils):
    p2 = (k - 1) // 2
    H = sum(p2 * (d + 1) for d in dils)
    M = max(p2 * d for d in dils)
    return H, M


def tile_of(form, arith, w_layout, variant, C, k, dils, n_seq, max_len, total_rows, len_mul, cus=CUS):
    """The kernel instantiation a launch takes: Tile(file, launcher, template arguments, WGCOLS, tt_out, sliding), or None where the library refuses
    the shape (no tile for the channel count, a window narrower than the kernel, a halo beyond the one-batch staging, a tile beyond 160 KiB LDS).
    form "unit" / "block"; arith "f32" / "f16" / "f32s" / "e7" / "e6"; dils: the unit's one dilation or the block's list; total_rows = 0: the
    rectangular geometry (a uniform batch), else the rows of a ragged batch with host lengths (its 1-D grid)."""
    dils = (dils,) if isinstance(dils, int) else tuple(dils)
    if w_layout not in (0, 1) or (w_layout == 1 and (arith not in ("e7", "e6") or form != "unit")):
        return None
    p2 = (k - 1) // 2
    if form == "unit":
        dil, = dils
        p1 = p2 * dil
        if arith == "f32":
            t, lds = _unit_f32(C, k, dil), None
            if t:
                lds = _unit_lds(t.wgcols, C, k, dil, 4, 2 * C * 4)
        elif arith == "f16":
            t = _unit_f16(C, k, dil)
            if t:
                lds = _unit_lds(t.wgcols, C, k, dil, 2, 2 * C * 4)
        elif arith == "f32s":
            t = _unit_split(C, k, dil)
            if t:
                if 2 * p1 > 64:
                    return None
                lds = _unit_lds(t.wgcols, C, k, dil, 4, 4 * C * 4 + 64)
        elif arith in ("e7", "e6"):
            t = _unit_emul16(C, k, dil) if w_layout == 1 else _unit_emul(C, k, dil, n_seq, max_len, len_mul)
            if t:
                ksplit, rreg = _flags(t)
                if ksplit and 2 * p1 > 64:
                    return None
                lds = _unit_lds(t.wgcols, C, k, dil, 6, 2 * C * 4, pitch_x=(C // 2) * 6 + 16 if ksplit else None)
                if w_layout == 1 and t.tt_out >= 8 and lds <= LDS_MAX:
                    tail = (k - 1) * C * 6
                    occ = int(t.args.split(", ")[5])
                    form_ = resunit16_pick(variant, cus * occ, t.wgcols, not rreg, lds + tail <= 160 * 1024, n_seq, max_len, total_rows, len_mul)
                    t = t._replace(sliding=form_ == 2)
        else:
            return None
        if t is None or t.tt_out < 8 or lds > LDS_MAX:
            return None
        return t
    if form != "block" or not 1 <= len(dils) <= 3:
        return None
    H, M = _block_geometry(k, dils)
    if arith == "f16":
        if 2 * H > 128:
            return None
        args = {32: "f16, 32, 512, 1, 4, 2, 2", 64: "f16, 64, 256, 1, 2, 4, 2" if 2 * H <= 32 else "f16, 64, 512, 1, 4, 4, 1", 128: "f16, 128, 256, 2, 4, 4, 1"}.get(C)
        t = args and _tile("resblock_f16.hip", "launch_resblock", args, 2 * H)
        elem, extra = 2, len(dils) * 2 * C * 4
    elif arith == "f32":
        if 2 * H > 32:
            return None
        args = {32: "float, 32, 512, 1, 4, 2, 2", 64: "float, 64, 256, 1, 2, 2, 2"}.get(C)
        t = args and _tile("resblock_f32.hip", "launch_resblock", args, 2 * H)
        elem, extra = 4, len(dils) * 2 * C * 4
    elif arith == "f32s":
        args = {32: "32, 512, 1, 4, 2, 2", 64: "64, 256, 1, 2, 2, 2"}.get(C)
        t = args and _tile("resblock_split.hip", "launch_resblock_split", args, 2 * H)
        elem, extra = 4, len(dils) * 4 * C * 4 + 64
        if 2 * M > 64:
            return None
    elif arith in ("e7", "e6"):
        args = {32: "T, 32, 256, 1, 2, 2, 2", 64: "T, 64, 128, 2, 2, 2, 2"}.get(C)
        t = args and _tile("resblock_emul.hip", "launch_resblock_emul", args, 2 * H)
        elem, extra = 6, len(dils) * 2 * C * 4
        if 2 * M > 64:
            return None
    else:
        return None
    if not t or t.tt_out < 32 or (t.wgcols + 2 * M) * (C * elem + 16) + extra > LDS_MAX:
        return None
    return t


DISPATCHERS = ("resunit_f32.hip", "resunit_f16_narrow.hip", "resunit_f16_wide.hip", "resunit_split.hip", "resunit_emul.hip",
               "resblock_f16.hip", "resblock_f32.hip", "resblock_split.hip", "resblock_emul.hip")


def source_instantiations():
    """{(file, launcher, template arguments)}: every `launch_*<...>(d, s` of the dispatcher sources (comments stripped)."""
    out = set()
    for f in DISPATCHERS:
        with open(os.path.join(CSRC, f)) as fh:
            text = re.sub(r"//[^\n]*", "", fh.read())
        for m in re.finditer(r"\b(launch_\w+)<([^<>;]*)>\(d, s", text):
            out.add((f, m.group(1), ", ".join(p.strip() for p in m.group(2).split(","))))
    return out


def arith_of(spec):
    return {"f32": "f32", "f16": "f16", "f32s": "f32s", "e7w0": "e7", "e6w0": "e6", "e7w1": "e7", "e6w1": "e6"}[spec]


def _key(form, spec, t):
    return (form, spec, t.file, t.launcher, t.args, t.sliding)


def model_instantiations(cus=CUS):
    """{(form, spec, file, launcher, arguments, sliding)}: everything tile_of can return, by enumeration: every channel count, k = 3 / 7 / 11, every
    dilation up to 32 (halos to both sides of every LDS rule and of the one-batch staging limit), one utterance of one row and a batch beyond every
    launch-size rule, every variant."""
    out = set()
    for spec in UNIT_SPECS:
        arith, w_layout = arith_of(spec), SPECS[spec][1]
        for C in (32, 64, 128, 256, 512):
            for k in (3, 7, 11):
                for dil in range(1, 33):
                    for n_seq, max_len in ((1, 1), (64, 1 << 20)):
                        for variant in ((0, 1, 2) if w_layout == 1 else (0,)):
                            t = tile_of("unit", arith, w_layout, variant, C, k, dil, n_seq, max_len, 0, 1, cus)
                            if t:
                                out.add(_key("unit", spec, t))
    for spec in BLOCK_SPECS:
        for C in (32, 64, 128, 256, 512):
            for k in (3, 7, 11):
                for dils in ((1,), (1, 3), (1, 3, 5), (2, 6), (1, 2, 3)):
                    t = tile_of("block", arith_of(spec), 0, 0, C, k, dils, 1, 1, 0, 1, cus)
                    if t:
                        out.add(_key("block", spec, t))
    return out


# ------------------------------------------------------------------------------------------ the case table
# kind "edges": lengths around every window the specs launch, at either side of the launch-size rules.  "small": the small-launch windows only.
# "wgs": the w_layout 0 emulated units beyond their launch-size rule (`thr` workgroups of the `win`-column window), by the smallest batch: the edge lengths plus 1- and 2-row utterances until the rectangular workgroup count crosses it.
# "auto": the library's own sliding pick (variant 0): positions >= 2 x runs x WGCOLS in a ragged batch.  "carry": a ragged batch of three windows per
# run (CUS x workgroups per CU runs), so that the forced sliding form carries h tails from window to window on every tile.
Case = collections.namedtuple("Case", "name form C k dils specs kind len_mul n_add out_scale m")


def _c(name, form, C, k, dils, specs, kind="edges", len_mul=1, n_add=0, out_scale=1.0, m=None):
    return Case(name, form, C, k, (dils,) if isinstance(dils, int) else tuple(dils), tuple(specs), kind, len_mul, n_add, out_scale, m or (2 if k == 3 else 1))


F32CLASS = ("f32", "f32s", "e7w0", "e6w0", "e7w1", "e6w1")
ALLU = UNIT_SPECS
CASES = [
    # ---- two-conv units: (C, k, d) at both sides of every dispatcher rule
    _c("u32-k3-d1", "unit", 32, 3, 1, ALLU),
    _c("u32-k7-d3", "unit", 32, 7, 3, ALLU),
    _c("u32-k11-d5", "unit", 32, 11, 5, ALLU),                  # f16: k > 7 -> the 512-column window
    _c("u64-k3-d5", "unit", 64, 3, 5, ALLU),                    # f16: k <= 3 -> 256 columns
    _c("u64-k7-d1", "unit", 64, 7, 1, ALLU),                    # f16: k > 3 -> 512 columns; emulated: k < 11 -> 128 columns
    _c("u64-k11-d3", "unit", 64, 11, 3, ALLU),                  # emulated: k >= 11 -> 256 columns
    _c("u128-k3-d1", "unit", 128, 3, 1, ALLU),
    _c("u128-k7-d3", "unit", 128, 7, 3, ALLU),                  # halo 18: f32 / split 128 columns, residual registers
    _c("u128-k7-d5", "unit", 128, 7, 5, ALLU),                  # halo 30: f32 / split <128, 256>
    _c("u128-k11-d1", "unit", 128, 11, 1, ALLU),                # halo 10, k > 7: f32 128 columns without residual registers
    _c("u128-k11-d5", "unit", 128, 11, 5, ALLU),                # halo 50: f16 <128, 192>; emulated w_layout 0: 128 columns at any launch size
    _c("u256-k3-d1", "unit", 256, 3, 1, ALLU),                  # f32 / split <256, 128>
    _c("u256-k7-d3", "unit", 256, 7, 3, ALLU),                  # halo 18: still <256, 128>
    _c("u256-k7-d5", "unit", 256, 7, 5, ALLU),                  # halo 30: f32 / split <256, 96>
    _c("u256-k11-d4", "unit", 256, 11, 4, ("e7w1", "e6w1")),    # halo 40: one-piece x tile whose sliding tail does not fit 160 KiB -> stays windowed
    _c("u256-k11-d5", "unit", 256, 11, 5, ALLU),                # halo 50: the channel-halves tile (w_layout 1)
    _c("u512-k3-d3", "unit", 512, 3, 3, ("f16",)),
    _c("u512-k7-d1", "unit", 512, 7, 1, ("f16",)),
    # ---- launch-size rules
    _c("u256-k3-d1-small", "unit", 256, 3, 1, ("e7w0", "e6w0"), kind="small"),      # wgs(64) <= 160: the 32-column window
    _c("u128-k3-d1-wgs", "unit", 128, 3, 1, ("e7w0", "e6w0"), kind="wgs"),          # wgs(128) > 448
    _c("u256-k3-d1-wgs", "unit", 256, 3, 1, ("e7w0", "e6w0"), kind="wgs"),          # wgs(64) > 160: the one-piece 64-column window
    _c("u256-k3-d21-wgs", "unit", 256, 3, 21, ("e7w0", "e6w0"), kind="wgs"),        # ... halo 42: the channel-halves tile
    _c("u128-k3-d1-auto", "unit", 128, 3, 1, ("e7w1", "e6w1"), kind="auto"),        # variant 0 picks the sliding form
    # ---- the sliding form with carried h tails (three windows per run) on the other w_layout 1 tiles
    _c("u256-k3-d1-carry", "unit", 256, 3, 1, ("e7w1", "e6w1"), kind="carry"),
    _c("u256-k3-d21-carry", "unit", 256, 3, 21, ("e7w1", "e6w1"), kind="carry"),    # the channel-halves tile
    _c("u64-k3-d1-carry", "unit", 64, 3, 1, ("e7w1", "e6w1"), kind="carry"),        # residual registers: sliding only when forced
    _c("u32-k3-d1-carry", "unit", 32, 3, 1, ("e7w1", "e6w1"), kind="carry"),
    # ---- len_mul and the MRF store passes (power-of-two scales)
    _c("u64-k7-d3-lm2", "unit", 64, 7, 3, ALLU, len_mul=2),
    _c("u128-k3-d3-lm3", "unit", 128, 3, 3, ALLU, len_mul=3),
    _c("u32-k3-d2-add1", "unit", 32, 3, 2, ALLU, n_add=1, out_scale=0.5),
    _c("u64-k3-d1-add2", "unit", 64, 3, 1, ALLU, n_add=2, out_scale=0.25),
    _c("u128-k3-d3-add2", "unit", 128, 3, 3, ALLU, n_add=2, out_scale=0.25),
    _c("u256-k3-d5-add1", "unit", 256, 3, 5, ALLU, n_add=1, out_scale=0.5),
    # ---- ResBlocks
    _c("b32-k3", "block", 32, 3, (1, 3, 5), BLOCK_SPECS),
    _c("b64-k3", "block", 64, 3, (1, 3, 5), BLOCK_SPECS),                           # f16: 2H = 24 <= 32 -> 256 columns
    _c("b32-k7", "block", 32, 7, (1, 3, 5), ("f16", "f32s", "e7w0", "e6w0")),       # (f32: 2H > 32 is refused)
    _c("b64-k7", "block", 64, 7, (1, 3, 5), ("f16", "f32s", "e7w0", "e6w0")),       # f16: 2H = 72 -> 512 columns
    _c("b128-k3", "block", 128, 3, (1, 3, 5), ("f16",)),
    _c("b128-k7", "block", 128, 7, (1, 3, 5), ("f16",)),
    _c("b64-k3-2units", "block", 64, 3, (2, 6), BLOCK_SPECS),
    _c("b32-k3-lm2", "block", 32, 3, (1, 3, 5), BLOCK_SPECS, len_mul=2),
    _c("b64-k3-add1", "block", 64, 3, (1, 3, 5), BLOCK_SPECS, n_add=1, out_scale=0.5),
    _c("b32-k3-add2", "block", 32, 3, (1, 3, 5), BLOCK_SPECS, n_add=2, out_scale=0.25),
    _c("b128-k3-add1", "block", 128, 3, (1, 3, 5), ("f16",), n_add=1, out_scale=0.5),
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
AUTO_PATTERN = [1, 7, 33, 129, 1000, 2, 4001, 50, 12345, 3, 777, 16, 5]


def side_halo(case):
    """Rows a result reads beyond its own position, per side: p1 + p2 of a unit, H of a block."""
    p2 = (case.k - 1) // 2
    return sum(p2 * (d + 1) for d in case.dils)


def _variants(spec):
    return (1, 2, 0) if SPECS[spec][1] == 1 else (0,)


def _edge_tts(case, n_seq, max_len):
    """tt_out of every window the case's specs launch on a batch of this rectangular size (the windowed form: the sliding form's first window)."""
    tts = set()
    for spec in case.specs:
        t = tile_of(case.form, arith_of(spec), SPECS[spec][1], 1, case.C, case.k, case.dils, n_seq, max_len, 0, case.len_mul)
        assert t is not None, (case.name, spec)
        tts.add(t.tt_out)
    return sorted(tts)


def _ceil(a, b):
    return -(-a // b)


@functools.lru_cache(maxsize=None)
def lens_of(name):
    """Base lengths of a case (rows = length x len_mul).  Short utterances sit between the long ones: every halo has a neighbour to read by mistake."""
    case = CASE_BY_NAME[name]
    lm = case.len_mul
    if case.kind == "auto":
        return tuple(AUTO_PATTERN * 4)
    if case.kind == "carry":
        t = tile_of(case.form, arith_of(case.specs[0]), 1, 2, case.C, case.k, case.dils, 1, 1, 0, lm)
        want, lens = 3 * CUS * int(t.args.split(", ")[5]) * t.wgcols, []
        while sum(lens) < want:
            lens += AUTO_PATTERN
        return tuple(lens)
    below = max(side_halo(case) - 1, 1)
    shorts = [1, 2, below]
    small, large = _edge_tts(case, 1, 1), _edge_tts(case, 1 << 20, 1 << 20)      # the windows to both sides of the launch-size rules
    tts = {"small": small, "wgs": large}.get(case.kind, sorted(set(small) | set(large)))
    edges = []
    for tt in tts:
        edges += [tt - 1, tt, tt + 1, 2 * tt - 1, 2 * tt, 2 * tt + 1]
    longest = 3 * max(tts) + 5
    lens = [_ceil(longest, lm)]
    for i, e in enumerate(edges):
        lens += [shorts[i % 3], _ceil(e, lm)]
    lens.append(1)
    if case.kind == "wgs":
        thr, win = (448, 128) if case.C == 128 else (160, 64)
        per_seq = _ceil(max(lens) * lm, win - (case.k - 1))
        i = 0
        while per_seq * len(lens) <= thr:
            lens.append(shorts[i % 2])
            i += 1
    return tuple(lens)


def launch_geometry(name, rect=False):
    """(n_seq, max_len, total_rows) as jatts_ragged carries them: total_rows = 0 for the rectangular geometry."""
    lens = lens_of(name)
    ragged = len(lens) > 1 and min(lens) != max(lens) and not rect
    return len(lens), max(lens), sum(lens) if ragged else 0


def case_tile(name, spec, variant=0, cus=CUS, rect=False, lens=None):
    case = CASE_BY_NAME[name]
    if lens is None:
        n_seq, max_len, total = launch_geometry(name, rect)
    else:
        n_seq, max_len, total = len(lens), max(lens), (sum(lens) if len(lens) > 1 and min(lens) != max(lens) and not rect else 0)
    return tile_of(case.form, arith_of(spec), SPECS[spec][1], variant, case.C, case.k, case.dils, n_seq, max_len, total, case.len_mul, cus)


def reached(cus=CUS):
    """{(form, spec, file, launcher, arguments, sliding): [case names]}: what the table launches (every variant of the w_layout 1 specs)."""
    out = collections.defaultdict(list)
    for case in CASES:
        for spec in case.specs:
            for variant in _variants(spec):
                t = case_tile(case.name, spec, variant, cus)
                assert t is not None, (case.name, spec)
                out[_key(case.form, spec, t)].append(case.name)
    return out


# ------------------------------------------------------------------------------------------ operands
# recipe -> (slope, |x| bound, weight magnitudes).  "half": slope 0.5, negative x even -> a = lrelu(x) is an integer; every later lrelu halves the lsb.
# "relu": slope 0, +-1 weights: everything stays an integer (the f16 blocks of two and three units: 11 bits hold no halved lsb at their magnitudes).
RECIPES = {"half": (0.5, 8, (1, 2)), "relu": (0.0, 2, (1,))}


def recipe_of(case, spec):
    return "relu" if case.form == "block" and len(case.dils) >= 2 and spec == "f16" else "half"


def perm_weight(C, k, m, mags, g):
    """(C, C, k) weights with exactly m non-zeros (+- a value of `mags`) in every (c_in, tap) column and exactly m k in every output channel's row:
    per tap, output channel perm[c] + j * step (mod C), j < m, for a random permutation and an odd step."""
    w = torch.zeros(C, C, k)
    c = torch.arange(C)
    for tap in range(k):
        perm = torch.randperm(C, generator=g)
        step = 2 * int(torch.randint(0, C // 2, (1,), generator=g)) + 1
        for j in range(m):
            n = (perm + j * step) % C
            val = torch.tensor(mags, dtype=torch.float32)[torch.randint(0, len(mags), (C,), generator=g)]
            sign = torch.randint(0, 2, (C,), generator=g).float() * 2 - 1
            w[n, c, tap] = val * sign
    return w


Inputs = collections.namedtuple("Inputs", "x units adds slope lens row_lens ref stages")


def _lrelu(t, slope):
    return torch.where(t < 0, t * slope, t)


def _conv(u, w, b, dil, pad):
    """(rows, C) -> (rows, C): conv over the rows with `pad` zero rows a side, float64."""
    return F.conv1d(F.pad(u.t().unsqueeze(0), (pad, pad)), w, b, dilation=dil)[0].t()


def _unit_ref(xs, unit, k, slope, fault, stages):
    w1, b1, w2, b2, dil = unit
    p2 = (k - 1) // 2
    a = _lrelu(xs, slope)
    h = _conv(a, w1, b1, dil, p2 * dil)
    g = _lrelu(h, slope)
    d2 = dil if fault == "dil_on_conv2" else 1
    if fault == "h_not_masked":                 # rows of h outside the utterance hold lrelu(b1) instead of zero
        edge = _lrelu(b1, slope).unsqueeze(0).expand(p2 * d2, -1)
        c2 = _conv(torch.cat([edge, g, edge]), w2, b2, d2, 0)
    else:
        c2 = _conv(g, w2, b2, d2, p2 * d2)
    y = c2 if fault == "no_residual" else xs + c2
    if stages is not None:
        stages.append(dict(x=xs, a=a, h=h, g=g, c2=c2, y=y, w1=w1, w2=w2, b1=b1, b2=b2))
    return y


FAULTS = ("h_not_masked", "window_halo_zero", "cross_utterance", "no_residual", "dil_on_conv2")


def reference_block(x, units, lens, k, slope, fault=None, tt=None, stages=None):
    """x <- x + conv_{k,1}(lrelu(conv_{k,d}(lrelu(x)) + b1)) + b2 for every unit (w1, b1, w2, b2, d) in turn, one utterance of `lens` (ROW counts) at a
    time, float64, every conv zero-padding its own input at the utterance's ends.  `stages`: a list that receives every intermediate, per utterance
    and unit.  `fault` builds a deliberately wrong result for the sensitivity tests: "h_not_masked" (h outside the utterance keeps lrelu(b1)),
    "window_halo_zero" (each window of `tt` outputs reads zeros beyond its own columns), "cross_utterance" (the halo reads the neighbouring
    utterances), "no_residual" (the residual add is dropped), "dil_on_conv2" (conv2 runs at conv1's dilation)."""
    x = x.double()
    units = [(w1.double(), b1.double(), w2.double(), b2.double(), d) for w1, b1, w2, b2, d in units]
    if fault == "cross_utterance":
        lens = [sum(lens)]
    elif fault == "window_halo_zero":
        cut = []
        for L in lens:
            cut += [min(tt, L - t0) for t0 in range(0, L, tt)]
        lens = cut
    f = fault if fault in ("h_not_masked", "no_residual", "dil_on_conv2") else None
    outs, o = [], 0
    n = torch.get_num_threads()
    if x.shape[0] * x.shape[1] < (1 << 22):
        torch.set_num_threads(1)          # many small convs: the intra-op pool's fork / join costs more than it gives
    try:
        for L in lens:
            xs = x[o:o + L]
            for unit in units:
                xs = _unit_ref(xs, unit, k, slope, f, stages)
            outs.append(xs)
            o += L
    finally:
        torch.set_num_threads(n)
    return torch.cat(outs)


def reference_unit(x, w1, b1, w2, b2, lens, k, dil, slope, fault=None, tt=None, stages=None):
    """The two-conv unit: reference_block of one unit."""
    return reference_block(x, [(w1, b1, w2, b2, dil)], lens, k, slope, fault, tt, stages)


def mix(y, adds, out_scale):
    """The MRF store pass: out_scale (y + add0 [+ add1]); without partners y itself."""
    return (y + sum(a.double() for a in adds)) * out_scale if adds else y


@functools.lru_cache(maxsize=None)
def inputs(name, recipe):
    """Operands, float64 reference (after the MRF pass) and reference intermediates of a case under a recipe; computed once per process and shared
    by every arithmetic of the recipe.  Leave them unchanged."""
    case = CASE_BY_NAME[name]
    slope, amp, mags = RECIPES[recipe]
    g = _gen("resunit", name, recipe)
    lens = list(lens_of(name))
    row_lens = [v * case.len_mul for v in lens]
    R, C = sum(row_lens), case.C
    x = torch.randint(-amp, amp + 1, (R, C), generator=g)
    if slope:
        q = int(round(1 / slope))
        x = torch.where(x < 0, -((-x) // q) * q, x)
    x = x.float()
    units = []
    for d in case.dils:
        w1, w2 = perm_weight(C, case.k, case.m, mags, g), perm_weight(C, case.k, case.m, mags, g)
        b1, b2 = torch.randint(-2, 3, (C,), generator=g).float(), torch.randint(-2, 3, (C,), generator=g).float()
        units.append((w1, b1, w2, b2, d))
    adds = [torch.randint(-8, 9, (R, C), generator=g).float() for _ in range(case.n_add)]
    stages = []
    y = reference_block(x, units, row_lens, case.k, slope, stages=stages)
    return Inputs(x, units, adds, slope, lens, row_lens, mix(y, adds, case.out_scale), stages)


def reference_fault(name, recipe, fault, tt=None):
    case = CASE_BY_NAME[name]
    d = inputs(name, recipe)
    return mix(reference_block(d.x, d.units, d.row_lens, case.k, d.slope, fault=fault, tt=tt), d.adds, case.out_scale)


# ------------------------------------------------------------------------------------------ exactness, from the reference's own intermediates
def lsb_exp(t):
    """e: every element of the float64 tensor is a multiple of 2^e (the largest such e; 0 for an all-zero tensor)."""
    t = t[t != 0]
    if t.numel() == 0:
        return 0
    mant, ex = torch.frexp(t.double())
    m = (mant.abs() * 2.0 ** 53).long()
    low = m & -m                                        # lowest set bit of the 53-bit significand
    tz = torch.log2(low.double()).round().long()
    return int((ex.long() - 53 + tz).min())


def _is_f16(t):
    return bool((t.half().double() == t).all())


def preconditions(name, spec):
    """Proves that the arithmetic class of `spec` computes the case without a single rounding; -> the measured maxima {max_a, max_g, max_y, lsb, bits,
    sum_units}.  From the reference intermediates of every utterance and unit (never from a worst-case bound alone):
      f32 class (f32, split f16 hi / lo, three bf16 terms): every staged operand (a, g, the residual x, the adds) spans at most 22 bits between the
        largest operand of the conv and its own lsb; max|operand| * max_n sum|w[n]| + max|b| stays below 2^24 units of the lsb, so no partial sum
        rounds in any order; the residual add, the MRF sum and its scaled value stay below 2^24 units of their lsb; the weights are one-term values.
      f16: the sum bound as above (f32 accumulators), and a, g, acc + b2, x, every unit's x + acc + b2 and the stored value are f16 numbers."""
    case = CASE_BY_NAME[name]
    cls = SPECS[spec][2]
    d = inputs(name, recipe_of(case, spec))
    out = dict(max_a=0.0, max_g=0.0, max_y=0.0, lsb=0, bits=0, sum_units=0.0)
    for w1, b1, w2, b2, _ in d.units:
        for w in (w1, w2):
            assert float(w.abs().max()) <= 2 and bool((w == w.round()).all()), "weights are +-1 / +-2: one bf16 / f16 term, exact under power-of-two scales"
    n_units = len(d.units)
    for u in range(n_units):
        st = d.stages[u::n_units]
        T = {key: torch.cat([s[key] for s in st]) for key in ("x", "a", "h", "g", "c2", "y")}
        w1, b1, w2, b2 = (st[0][key] for key in ("w1", "b1", "w2", "b2"))
        for operand, w, b, res in ((T["a"], w1, b1, T["h"]), (T["g"], w2, b2, T["c2"])):
            e = min(lsb_exp(operand), lsb_exp(b))
            top = float(operand.abs().max())
            bits = 0 if top == 0 else int(torch.log2(torch.tensor(top / 2.0 ** e)).floor()) + 1
            bound = (top * float(w.abs().sum((1, 2)).max()) + float(b.abs().max())) / 2.0 ** e
            assert bound < F24, f"{name} unit {u}: partial sums reach {bound:g} lsb units"
            assert float(res.abs().max()) / 2.0 ** e <= bound
            if cls == "f32":
                assert bits <= 22, f"{name} unit {u}: a staged operand spans {bits} bits"
            out["bits"], out["sum_units"], out["lsb"] = max(out["bits"], bits), max(out["sum_units"], bound), min(out["lsb"], e)
        e = min(lsb_exp(T["x"]), lsb_exp(T["c2"]))
        top = max(float(T[key].abs().max()) for key in ("x", "c2", "y")) / 2.0 ** e
        assert top < F24, f"{name} unit {u}: the residual add reaches {top:g} lsb units"
        if cls == "f32":
            assert top < 2 ** 22, f"{name} unit {u}: the residual spans more than 22 bits"
        else:
            for key in ("x", "a", "g", "c2", "y"):
                assert _is_f16(T[key]), f"{name} unit {u}: {key} is no f16 tensor"
            if case.form == "block":             # (the unit kernel rounds g = lrelu(h), the block kernel h itself and then its lrelu)
                assert _is_f16(T["h"]), f"{name} unit {u}: h is no f16 tensor"
        out["max_a"], out["max_g"] = max(out["max_a"], float(T["a"].abs().max())), max(out["max_g"], float(T["g"].abs().max()))
        out["max_y"], out["lsb"] = max(out["max_y"], float(T["y"].abs().max())), min(out["lsb"], e)
    if d.adds:
        y = torch.cat([s["y"] for s in d.stages[n_units - 1::n_units]])
        total = y + sum(a.double() for a in d.adds)
        e = min(lsb_exp(y), 0)
        top = (float(y.abs().max()) + sum(float(a.abs().max()) for a in d.adds)) / 2.0 ** e
        assert top < (F24 if cls == "f16" else 2 ** 22), f"{name}: the MRF sum reaches {top:g} lsb units"
        assert bool((total * case.out_scale == d.ref).all())
        assert case.out_scale in (0.5, 0.25)              # a power of two: the product is exact
    if cls == "f16":
        assert _is_f16(d.ref), f"{name}: the stored value is no f16 tensor"
    else:
        assert bool((d.ref.float().double() == d.ref).all())
    out["max_out"] = float(d.ref.abs().max())
    return out
