"""CPU: the tap windows of the polyphase upsampling convs (hip.convtranspose_tap_groups) against the zero pattern of hip.convtranspose_as_conv, and the
argument checks of jatts_conv_desc's tap-window hint.  No compute calls."""
import ctypes as C

import pytest
import torch

STRIDES = (2, 3, 4, 5, 8)


def _pad(s):
    return s // 2 + s % 2


@pytest.mark.parametrize("s", STRIDES)
def test_tap_groups_agree_with_the_zero_pattern(s):
    """An all-ones ConvTranspose1d weight leaves ones exactly at the real taps of the polyphase weight: the windows must name those taps and no others."""
    from jatts_amd import hip
    c_in, c_out, K = 3, 2, 2 * s
    tg = hip.convtranspose_tap_groups(K, s, _pad(s))
    assert tg is not None
    a, a0, b0, k = tg
    wc, _ = hip.convtranspose_as_conv(torch.ones(c_in, c_out, K), s, _pad(s))
    assert wc.shape == (s * c_out, c_in, 3)
    assert 0 < a < s and k == 2 and (a0, b0) == (0, 1)
    assert a == {2: 1, 3: 1, 4: 2, 5: 2, 8: 4}[s]                     # even strides split in halves, s = 5 as 2 | 3, s = 3 as 1 | 2
    want = torch.zeros(s * c_out, 3)
    want[:a * c_out, a0:a0 + k] = 1
    want[a * c_out:, b0:b0 + k] = 1
    for c in range(c_in):
        assert torch.equal(wc[:, c, :], want)
    hip.check_tap_window(wc, (a * c_out, a0, b0, k))
    planted = wc.clone()
    planted[0, 1, 2] = 1.0                                           # group A's zero tap
    with pytest.raises(ValueError, match="not zero outside"):
        hip.check_tap_window(planted, (a * c_out, a0, b0, k))
    planted = wc.clone()
    planted[-1, 0, 0] = -1.0                                         # group B's zero tap
    with pytest.raises(ValueError, match="not zero outside"):
        hip.check_tap_window(planted, (a * c_out, a0, b0, k))


@pytest.mark.parametrize("K,s,p", [(3, 1, 1),      # one phase: one window
                                   (12, 4, 4),     # K = 3 s: every phase uses all three taps
                                   (4, 4, 0),      # K = s: one tap for every phase
                                   (6, 2, 2),      # K = 3 s, s = 2
                                   (7, 2, 2)])     # phases of unequal tap counts
def test_geometries_without_two_equal_groups_give_none(K, s, p):
    from jatts_amd import hip
    assert hip.convtranspose_tap_groups(K, s, p) is None


def _desc(p, n_out=64, k_w=3):
    from jatts_amd import _abi
    d = _abi.ConvDesc()
    d.rg = _abi.Ragged(p, 1, 0, 1, 0, None)            # max_len 0: a well-formed descriptor returns JATTS_OK without a launch
    d.dtype, d.n_in, d.ldx, d.in_scale = _abi.F32, 1, 64, 1.0
    d.x[0], d.w, d.y = p, p, p
    d.c_in, d.n_out, d.k_w, d.dil, d.pad, d.ldy, d.y_is_f32, d.alpha = 64, n_out, k_w, 1, 1, n_out, 1, 1.0
    return d


def test_conv1d_refuses_malformed_tap_windows(lib):
    """include/jatts_hip.h: windows inside [0, k_w], tap_k >= 1, tap_group_n <= n_out, no n_split.  The refusal comes from the argument checks, before
    anything is launched (the pointers are host scratch that no kernel ever sees)."""
    scratch = (C.c_float * 64)()
    p = C.addressof(scratch)

    def rc(n_out=64, n_split=0, **win):
        d = _desc(p, n_out)
        d.tap_group_n, d.tap_a0, d.tap_b0, d.tap_k = (win.get(k, v) for k, v in (("n", 32), ("a0", 0), ("b0", 1), ("k", 2)))
        if n_split:
            d.n_split, d.y2, d.ldy2 = n_split, p, 64
        return lib.jatts_conv1d(C.byref(d), None)

    assert rc() == 0
    assert rc(n=64) == 0 and rc(k=3, b0=0) == 0 and rc(k=1, a0=2, b0=0) == 0      # the edges of what is allowed
    assert rc(n=0, a0=7, b0=-3, k=0) == 0                                         # no hint: the other fields are not read
    for bad in (dict(n=65), dict(n=-32), dict(k=0), dict(k=-1), dict(a0=-1), dict(b0=-1), dict(a0=2), dict(b0=2), dict(k=4, a0=0, b0=0),
                dict(a0=3, k=1), dict(b0=2 ** 31 - 1)):
        assert rc(**bad) == -1 and b"tap window" in lib.jatts_last_error(), bad
    assert rc(n_out=512, n_split=256, n=0) == 0                                   # two outputs without a hint: fine
    assert rc(n_out=512, n_split=256, n=256) == -1 and b"tap window" in lib.jatts_last_error()
