"""CPU half of the row-wise edge cases (tests/rowwise_edge_cases.py): the references are checked against themselves -- the float64 formula
against its float32 evaluation -- and every case is shown to reach the launcher branch it was built for, from the dispatch conditions of
csrc/rowwise.hip / csrc/spkemb.hip restated in Python (rowwise_edge_cases.branch).  No GPU, no library."""
import os

import pytest
import torch
import torch.nn.functional as F

import rowwise_edge_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# What the float32 evaluation of a formula may differ from float64 by, in the bound's own units |r32 - ref64| / (1 + |ref64|), from the
# number format alone (eps = 2**-24; derived, not taken from any kernel's result):
#   a normalisation carries the error of its float32 mean, divided by std: a blocked / pairwise sum of n values of size m errs by up to
#     log2(n) * eps * m, times |gamma| <= 4.  LayerNorm on mean 100 / std 1, n = 2048: 11 * eps * 100 * 4 = 2.6e-4 -> 3e-4; GroupNorm on
#     mean 50 / std 0.5, n <= 16 512: 14 * eps * 50 / 0.5 * 4 = 3.3e-4 -> 4e-4;
#   the depthwise conv sums up to 93 taps of a sequence scaled by 1e3 (|a w| reaches 1e3 * 4 * 0.3 * 4 = 5e3) and the sum may cancel, so
#     1 + |ref| does not normalise it: sqrt(93) * eps * 5e3 = 3e-3 in a random walk -> 3e-3;
#   fbank: 10 log10 p reaches 120 dB, 1 + |ref| normalises it; the time mean of 300 frames adds 300 * eps / 2 -> 2e-5;
#   everything else is a handful of operations on O(1) values -> 64 * eps = 4e-6.
ERR32_CAP = {"layernorm": 3e-4, "groupnorm_mish": 4e-4, "glu_dwconv_bn_swish": 3e-3, "fbank_post": 2e-5}
ERR32_CAP_DEFAULT = 64 * 2.0 ** -24


@pytest.mark.parametrize("cid", list(RC.CASES))
def test_reference_agrees_with_its_float32_evaluation(cid):
    c = RC.CASES[cid]
    assert set(c.ref64) == set(c.r32)
    for k, r in c.ref64.items():
        assert r.shape == c.r32[k].shape and bool(torch.isfinite(r.double()).all()), (cid, k)
        if not r.is_floating_point():
            assert torch.equal(r, c.r32[k]), (cid, k)                    # integer outputs do not depend on the float width
        elif c.exact:                                                     # a move or one rounding: float32 is float64 rounded once
            assert float(((c.r32[k].double() - r).abs() - 2.0 ** -24 * r.abs()).max()) <= 0, (cid, k)
        else:
            assert r.dtype == torch.float64, (cid, k)
            assert bool(((c.r32[k].double() - r).abs() <= c.allowed(k)).all()), (cid, k)
    cap = ERR32_CAP.get(c.kernel, ERR32_CAP_DEFAULT)
    assert c.err32 <= cap, (cid, c.err32, cap)


@pytest.mark.parametrize("cid", list(RC.CASES))
def test_case_reaches_its_branch(cid):
    c = RC.CASES[cid]
    assert RC.branch(c) == c.expect, (cid, RC.branch(c), c.expect)


def test_refused_shapes_are_refused_by_the_restated_dispatch():
    mk = lambda kernel, p: RC.Case(kernel, "refused", p, None, None, None)          # noqa: E731
    assert RC.branch(mk("layernorm", RC.LN_REFUSED)) == "refused" and RC.branch(mk("layernorm", dict(dim=2048))) == "full"
    for want, p in RC.GLU_REFUSED.items():
        assert RC.branch(mk("glu_dwconv_bn_swish", p)) == want
    # K = 93 is the widest odd kernel whose tile + transposed taps fit the 64 KiB of LDS, from the launcher's own formula
    assert RC.glu_lds_bytes(93) <= 64 * 1024 < RC.glu_lds_bytes(95)
    assert RC.branch(mk("hifigan_output", dict(RC.HO_REFUSED, lens=[1], mul=1))) == "refused-lds"
    assert RC.hifigan_lds_bytes(32, 7) <= 64 * 1024 and RC.hifigan_lds_bytes(12, 7) <= 64 * 1024
    assert RC.branch(mk("gaussian_upsample", RC.GU_REFUSED)) == "refused-text"
    assert RC.branch(mk("gaussian_upsample", dict(lens=[16384], dim=16))) == "lanes2-ctail"
    assert RC.branch(mk("fbank_post", RC.FB_REFUSED)) == "refused"


def test_every_branch_of_the_issue_table_has_a_case():
    got = {(c.kernel, c.expect) for c in RC.CASES.values()}
    for want in [("snakebeta", "scalar"), ("snakebeta", "scalar-stride2"), ("snakebeta", "vec-stride2"), ("hifigan_output", "scalar-tiles"),
                 ("hifigan_output", "vec-tiles"), ("groupnorm_mish", "split-groups"), ("groupnorm_mish", "split-rows"),
                 ("groupnorm_mish", "single-workgroup"), ("glu_dwconv_bn_swish", "vec-kmax0-ctail"), ("glu_dwconv_bn_swish", "scalar-kmax0-ctail"),
                 ("glu_dwconv_bn_swish", "vec-kmax32-ctail"), ("layernorm", "tail"), ("layernorm", "full"), ("gaussian_upsample", "lanes2-ctail"),
                 ("gaussian_upsample", "lanes2"), ("variance_embed_add", "cloop2"), ("add_seq_vector", "cloop2"), ("gated_tanh_sigmoid", "cloop2"),
                 ("embed_scale", "cloop2"), ("lr_durations", "per2-rule2"), ("lr_durations", "per2-rule1"), ("zero_pad_rows", "stride2"),
                 ("affine_cast", "stride2"), ("gaussian_sample", "stride2"), ("flip_channels", "stride2"), ("frame_signal", "stride2"),
                 ("sq_err_sum", "blocks256-stride2")]:
        assert want in got, want
    # the widest channels-per-group that still takes the time-split form, and the first that does not
    gcs = {c.p["C"] // c.p["G"]: c.expect for c in RC.of("groupnorm_mish") if c.p["time_split"]}
    assert gcs[128] == "split-rows" and gcs[136] == "single-workgroup" and gcs[4] == "single-workgroup"


def test_case_data_has_the_edges_it_claims():
    for c in RC.of("layernorm"):
        if c.p["kind"] == "offset":
            assert abs(float(c.x["x"].mean()) - 100.0) < 0.5
        if c.p["kind"] == "const":
            assert float(c.x["x"][0].std()) == 0.0 and torch.equal(c.r32["y"][0], c.x["beta"])
    for c in RC.of("groupnorm_mish"):
        assert abs(float(c.x["x"].mean()) - 50.0) < 0.1 and abs(float(c.x["x"].std()) - 0.5) < 0.1
    for c in RC.of("gaussian_upsample"):
        d = c.x["d"]
        assert int((d == 0).sum()) > 0 and int(d.max()) == 40 and all(n % 4 for n in RC.gu_olens(c))
    for c in RC.of("fbank_post"):
        assert RC.fb_floor_binds(c) == [True, False, False]
    for c in RC.of("l2_normalize"):
        assert not c.x["x"][2].any() and not c.ref64["y"][2].any()
    for c in RC.of("lr_durations"):
        assert bool((c.ref64["index"] == -1).any()) == bool(sum(c.p["extra"]))
        if c.p["zero_seqs"] and c.p["zero_rule"] == 2:
            assert c.ref64["fallback"].tolist() == [int(b in c.p["zero_seqs"]) for b in range(len(c.p["lens"]))]
    assert RC.CASES["lr_durations/lout-15-16-17"].ref64["olens"].tolist() == [15, 16, 17]
    for c in RC.of("seq_mean_std"):
        if c.p["logits"]:
            assert float(c.x["logits"].max()) == 80.0 and float(c.x["logits"].min()) == -80.0
        assert torch.allclose(c.ref64["std"][0], torch.full_like(c.ref64["std"][0], 1e-6))       # T = 1: sqrt(eps)


def test_written_out_norms_equal_the_library_ones():
    """LayerNorm / GroupNorm are written out in the case table (two passes); in float64 they are F.layer_norm / F.group_norm + F.mish.  A
    constant row or group amplifies the library's own float64 rounding by rstd = eps^-1/2 (1e6 / 316), hence 1e-8."""
    for c in RC.of("layernorm"):
        lib = F.layer_norm(c.x["x"].double(), (c.p["dim"],), c.x["gamma"].double(), c.x["beta"].double(), c.p["eps"])
        assert float(((lib - c.ref64["y"]).abs() / (1 + lib.abs())).max()) <= 1e-8, c.id
    for c in RC.of("groupnorm_mish"):
        lib = RC.gn_library_form(c)
        assert float(((lib - c.ref64["y"]).abs() / (1 + lib.abs())).max()) <= 1e-8, c.id


def test_predictor_head_near_ties_stay_rare():
    """The one masked comparison of the GPU tests: a duration within 1e-4 of a .5 rounding boundary (the existing rule of
    test_predictor_head_and_durations) is not compared.  On these seeds that is under 1 % of the rows."""
    near = rows = 0
    for c in RC.of("predictor_head"):
        _, nr = RC.durations_of(c.ref64["v"], c.p["offset"])
        near, rows = near + int(nr.sum()), rows + nr.numel()
    assert near < 0.01 * rows, (near, rows)


def test_write_bounds_table():
    """profiles/rowwise_edge_bounds.txt: per case, the reference's own float32 error and the bound the GPU tests hold the kernel to, so that
    a reader sees which term binds.  (err32 is printed with two digits: it moves in the last ones with the CPU's vector width.)"""
    lines = ["# case  T_k  err32  tol = max(T_k, 4 * err32)  binding term   (|y - ref64| <= tol + tol * |ref64|, + 2**-10 |ref64| for f16 outputs)"]
    for c in RC.CASES.values():
        if c.exact:
            lines.append(f"{c.id}  exact")
        else:
            lines.append(f"{c.id}  {c.tk:.0e}  {c.err32:.1e}  {c.tol:.1e}  {'T_k' if c.tol == c.tk else 'err32'}")
    path = os.path.join(ROOT, "profiles", "rowwise_edge_bounds.txt")
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    assert os.path.getsize(path) < 1 << 20
