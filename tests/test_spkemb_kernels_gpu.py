"""GPU: the six kernels of csrc/spkemb.hip one at a time (case table, references and bounds: tests/rowwise_edge_cases.py).  Through the
fbank / ECAPA end-to-end tests one wrong pooling channel or one SE gate is invisible; here every output element is held to
|y - ref64| <= tol + tol |ref64| with tol = max(1e-5, 4 err32), or to exact equality where the kernel only moves data."""
import pytest
import torch

import rowwise_edge_cases as RC
from rowwise_edge_cases import ERR_ARG, SENTINEL, dev, dt_of, hold, ragged, refused, same

pytestmark = pytest.mark.gpu


def test_frame_signal(cuda, lib):
    """n_fft = 16, hop = 4, ldo = 24; signals of 3, 16 and 4 200 samples (1 051 frames: the grid-stride step past 1 024 workgroups).  Exact:
    one float32 product per element, zeros outside the signal and in the padding columns."""
    from jatts_amd import hip
    c = RC.CASES["frame_signal/n16-hop4"]
    p = c.p
    cu = torch.tensor(RC.cu_of(p["samples"]), dtype=torch.int32, device=cuda)
    y = hip.frame_signal(ragged(p["frames"], cuda), cu, dev(c.x["x"], cuda), dev(c.x["window"], cuda), p["n_fft"], p["hop"], p["ldo"])
    same(c, "y", y)


def test_power_spectrum(cuda, lib):
    from jatts_amd import hip
    c = RC.CASES["power_spectrum/bins9"]
    p = c.p
    y = hip.power_spectrum(dev(c.x["x"], cuda), p["n_bins"], p["ldo"])
    hold(c, "y", y)
    assert not y[:, p["n_bins"]:].any()                       # ldo > n_bins zero-fills
    with refused(ERR_ARG, "power_spectrum: bad strides"):     # ldx < 2 n_bins
        hip.power_spectrum(dev(c.x["x"], cuda)[:, :2 * p["n_bins"] - 1].contiguous(), p["n_bins"], p["ldo"])
    with refused(ERR_ARG, "power_spectrum: bad strides"):     # ldo < n_bins
        hip.power_spectrum(dev(c.x["x"], cuda), p["n_bins"], p["n_bins"] - 1)


@pytest.mark.parametrize("cid", RC.ids_of("fbank_post"))
def test_fbank_post(cuda, lib, cid):
    """Utterance 0 spans 150 dB (the top_db floor binds), utterances 1 (one frame) and 2 stay within 6 dB (it does not): the floor is per
    utterance.  ldo = n_mels + 8 zero-fills."""
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    y = hip.fbank_post(ragged(p["lens"], cuda), dev(c.x["p"], cuda), p["n_mels"], p["ldo"], amin=p["amin"], top_db=p["top_db"])
    hold(c, "y", y)
    assert not y[:, p["n_mels"]:].any()


def test_fbank_post_refuses_257_mels(cuda, lib):
    from jatts_amd import hip
    n = RC.FB_REFUSED["n_mels"]
    with refused(ERR_ARG, "fbank_post: bad geometry"):
        hip.fbank_post(ragged([3], cuda), torch.ones(3, n, device=cuda), n, n)


@pytest.mark.parametrize("want_std", [True, False])
@pytest.mark.parametrize("cid", RC.ids_of("seq_mean_std"))
def test_seq_mean_std(cuda, lib, cid, want_std):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    out = hip.seq_mean_std(ragged(p["lens"], cuda), dev(c.x["x"], cuda), p["dim"], logits=dev(c.x["logits"], cuda), want_std=want_std, eps=p["eps"])
    assert out.shape == (len(p["lens"]), (2 if want_std else 1) * p["dim"])
    hold(c, "mean", out[:, :p["dim"]])
    if want_std:
        hold(c, "std", out[:, p["dim"]:])


@pytest.mark.parametrize("out16", [False, True])
@pytest.mark.parametrize("cid", RC.ids_of("seq_affine_act"))
def test_seq_affine_act(cuda, lib, cid, out16):
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    y = hip.seq_affine_act(ragged(p["lens"], cuda), dev(c.x["x"], cuda), p["dim"], dt_of(out16), seq_vec=dev(c.x["vec"], cuda),
                           pre_act=hip.ACT_RELU if p["pre"] else hip.ACT_NONE, scale=dev(c.x["scale"], cuda), shift=dev(c.x["shift"], cuda),
                           post_act=hip.ACT_TANH if p["post"] else hip.ACT_NONE, ldy=p["ldy"])
    hold(c, "y", y, out16)
    assert not y[:, p["dim"]:].any()


def test_seq_affine_act_refuses_short_strides(cuda, lib):
    from jatts_amd import hip
    x = torch.zeros(4, 16, device=cuda)
    with refused(ERR_ARG, "seq_affine_act: bad strides"):     # ldy < dim
        hip.seq_affine_act(ragged([4], cuda), x, 16, hip.F32, ldy=15)
    with refused(ERR_ARG, "seq_affine_act: bad strides"):     # ldx < dim
        hip.seq_affine_act(ragged([4], cuda), x, 17, hip.F32)


@pytest.mark.parametrize("cid", RC.ids_of("se_scale_add"))
def test_se_scale_add(cuda, lib, cid):
    """Fresh output, then into columns 4 .. 4 + dim of a wider sentinel-filled matrix."""
    from jatts_amd import hip
    c = RC.CASES[cid]
    p = c.p
    rb, x, s, resid = ragged(p["lens"], cuda), dev(c.x["x"], cuda), dev(c.x["s"], cuda), dev(c.x["resid"], cuda)
    hold(c, "y", hip.se_scale_add(rb, x, s, resid=resid))
    wide = torch.full((x.shape[0], p["dim"] + 9), SENTINEL, device=cuda)
    hip.se_scale_add(rb, x, s, resid=resid, out=wide, out_col0=4)
    hold(c, "y", wide[:, 4:4 + p["dim"]])
    assert bool((wide[:, :4] == SENTINEL).all()) and bool((wide[:, 4 + p["dim"]:] == SENTINEL).all())
