"""No GPU: the `const jatts_scratch* scratch` argument of the thirteen entry points that reduce across workgroups (include/jatts_hip.h:
jatts_scratch; csrc/det_reduce.h, csrc/api.hip: jatts_ws_need).  Where a call reduces, a scratch that is missing, misaligned or too small is
refused with JATTS_ERR_ARG by the argument checks, before anything is launched -- every pointer here is host memory that no kernel ever sees;
where nothing is launched at all, NULL is accepted.  The library keeps no scratch of its own: the registration call is gone."""
import ctypes as C
import os
import re

import pytest

from conftest import ROOT

TICKET_BYTES = 64 * 1024
ROWS, DIM = 513, 81
STFT_SAMPLES = [4000, 4800]          # hop 16: 251 and 301 frames


def _calls(_abi, rows, max_len, n_seq, reduce=True):
    """{entry point: f(lib, scratch) -> rc} at ROWS x DIM-sized shapes (rows = max_len = n_seq = 0: the empty launch).  reduce=False: the
    form of the call that does not reduce through the scratch, where the entry point has one."""
    host = (C.c_float * 64)()
    p = C.addressof(host)
    q = p if reduce else None                                  # the outputs whose presence makes the call reduce
    rg = _abi.Ragged(p, n_seq, max_len, 1, 0, None)
    ns = (C.c_int32 * 2)(*STFT_SAMPLES)
    rg_frames = _abi.Ragged(p, n_seq, 1 + max(STFT_SAMPLES) // 16 if n_seq else 0, 1, 0, None)
    kw = 7 if reduce else 3                                    # conv1d_wgrad: k_w = 7 is the VALU path, k_w = 3 the MFMA path (no db)
    r = C.byref(rg)
    return {
        "jatts_layernorm_bwd": lambda lib, sc: lib.jatts_layernorm_bwd(p, DIM, p, DIM, p, rows, DIM, 1e-5, p, DIM, q, q, sc, None),
        "jatts_groupnorm_bwd": lambda lib, sc: lib.jatts_groupnorm_bwd(r, p, p, 64, 8, p, p, p, p, q, q, sc, None),
        "jatts_snakebeta_bwd": lambda lib, sc: lib.jatts_snakebeta_bwd(p, p, rows, DIM, p, p, p, p, p, sc, None),
        "jatts_dwconv_wgrad": lambda lib, sc: lib.jatts_dwconv_wgrad(r, p, p, p, DIM, 7, 3, sc, None),
        "jatts_col_stats": lambda lib, sc: lib.jatts_col_stats(p, None, DIM, rows, DIM, None, None, 0, p, p, sc, None),
        "jatts_col_sum": lambda lib, sc: lib.jatts_col_sum(p, DIM, rows, DIM, p, sc, None),
        "jatts_col_wsum": lambda lib, sc: lib.jatts_col_wsum(p, DIM, p, rows, DIM, p, sc, None),
        "jatts_seq_sum": lambda lib, sc: lib.jatts_seq_sum(r, p, DIM, p, sc, None),
        "jatts_qkv_split_bwd": lambda lib, sc: lib.jatts_qkv_split_bwd(p, p, p, p, 2, 300, 3, 27, p, p, p, sc, None),
        "jatts_sumsq": lambda lib, sc: lib.jatts_sumsq(p, rows * DIM, p, sc, None),
        "jatts_conv1d_wgrad": lambda lib, sc: lib.jatts_conv1d_wgrad(r, p, DIM, p, DIM, DIM, DIM, kw, 1, 3 if reduce else 1, p, q, p, sc, None),
        "jatts_conv1d_wgrad_emul": lambda lib, sc: lib.jatts_conv1d_wgrad_emul(r, p, DIM, p, DIM, DIM, DIM, kw, 1, 3 if reduce else 1, _abi.F32E,
                                                                                 p, q, p, sc, None),
        "jatts_stft_mag": lambda lib, sc: lib.jatts_stft_mag(C.byref(rg_frames), p, ns, p, p, 64, 16, p, 33, q, sc, None),
    }


ENTRY_POINTS = ["jatts_layernorm_bwd", "jatts_groupnorm_bwd", "jatts_snakebeta_bwd", "jatts_dwconv_wgrad", "jatts_col_stats", "jatts_col_sum",
                "jatts_col_wsum", "jatts_seq_sum", "jatts_qkv_split_bwd", "jatts_sumsq", "jatts_conv1d_wgrad", "jatts_conv1d_wgrad_emul",
                "jatts_stft_mag"]
# the entry points with a form that does not reduce: dgamma = dbeta = NULL, pow_sum = NULL, the MFMA path without db.  (jatts_qkv_split_bwd with
# du = dv = NULL has one too, but no empty launch -- it refuses t_len = 0 -- so it cannot be called without a GPU.)
NON_REDUCING = ["jatts_layernorm_bwd", "jatts_groupnorm_bwd", "jatts_conv1d_wgrad", "jatts_conv1d_wgrad_emul", "jatts_stft_mag"]


def _aligned(n):
    """-> (keep-alive, 16-byte aligned host address with n bytes behind it)"""
    raw = (C.c_char * (n + 16))()
    return raw, (C.addressof(raw) + 15) & ~15


def test_the_table_names_the_thirteen_entry_points():
    from jatts_amd import _abi
    takes = sorted(n for n, (_, args) in _abi.PROTOTYPES.items() if C.POINTER(_abi.Scratch) in args)
    assert takes == sorted(ENTRY_POINTS) == sorted(_calls(_abi, ROWS, 300, 2)) and len(takes) == 13
    for n in takes:                                            # immediately in front of the stream
        assert _abi.PROTOTYPES[n][1][-2:] == [C.POINTER(_abi.Scratch), C.c_void_p], n


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_a_reducing_call_refuses_a_missing_misaligned_or_short_scratch(lib, name):
    from jatts_amd import _abi
    call = _calls(_abi, ROWS, 300, 2)[name]
    keep, addr = _aligned(64)
    big = 1 << 40
    assert call(lib, None) == -1 and b"jatts_scratch" in lib.jatts_last_error()                       # NULL scratch
    assert call(lib, C.byref(_abi.Scratch(None, big))) == -1                                            # NULL buf
    assert call(lib, C.byref(_abi.Scratch(addr + 4, big))) == -1 and b"aligned" in lib.jatts_last_error()
    assert call(lib, C.byref(_abi.Scratch(addr, 0))) == -1                                              # no bytes at all: the message names the need
    named = re.search(rb"(\d+) bytes of scratch", lib.jatts_last_error())
    assert named and int(named.group(1)) > 0 and int(named.group(1)) % 4 == 0, lib.jatts_last_error()
    need = int(named.group(1))
    assert call(lib, C.byref(_abi.Scratch(addr, TICKET_BYTES + need - 16))) == -1                       # 16 bytes short of that
    again = re.search(rb"(\d+) bytes of scratch", lib.jatts_last_error())
    assert again and int(again.group(1)) == need and b"jatts_scratch" in lib.jatts_last_error()
    del keep


@pytest.mark.parametrize("name", [n for n in ENTRY_POINTS if n != "jatts_qkv_split_bwd"])       # (t_len = 0 is bad geometry there: no empty launch)
def test_an_empty_launch_takes_a_null_scratch(lib, name):
    from jatts_amd import _abi
    assert _calls(_abi, 0, 0, 0)[name](lib, None) == 0, lib.jatts_last_error()


@pytest.mark.parametrize("name", NON_REDUCING)
def test_the_non_reducing_form_takes_a_null_scratch_on_an_empty_launch(lib, name):
    from jatts_amd import _abi
    assert _calls(_abi, 0, 0, 0, reduce=False)[name](lib, None) == 0, lib.jatts_last_error()


def test_the_registration_call_is_gone(lib):
    from jatts_amd import _abi
    hdr = open(os.path.join(ROOT, "include", "jatts_hip.h")).read()
    assert "jatts_set_workspace" not in hdr and "jatts_set_workspace" not in _abi.PROTOTYPES
    assert not hasattr(lib, "jatts_set_workspace")
