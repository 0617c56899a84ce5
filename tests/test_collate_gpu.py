"""GPU: jatts_collate (csrc/collate.hip) against a numpy restatement of its copy rule, bit for bit.  Every destination is pre-filled with NaN
(float32) or -1 (int64) and handed to ``hip.collate(out=...)``, so an element the kernel leaves unwritten shows.
Each case is the smallest that reaches a branch of the kernel: the 16-byte path and the word path (row starts off 16 bytes), the unit that
straddles an utterance's end, the slot's last partial unit, more than one workgroup per slot, several fields per launch."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def make_store(lens, dim, dtype, seed, lead=0):
    """All utterances one behind the other, ``lead`` unused rows in front (they shift every row start, and with it the alignment)."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    rows = int(lens.sum()) + lead
    if dtype == np.float32:
        flat = rng.standard_normal((rows, dim)).astype(np.float32)
    else:
        flat = rng.integers(-(1 << 40), 1 << 40, size=(rows, dim), dtype=np.int64)
    start = lead + np.concatenate([[0], np.cumsum(lens)[:-1]])
    return flat, start, lens


def restate(flat, start, lens, ids, t_max):
    """dst[b][t][c] = src[(row_start[u] + t) * dim + c] for t < row_len[u], all-zero bits behind."""
    out = np.zeros((len(ids), t_max, flat.shape[1]), dtype=flat.dtype)
    for b, u in enumerate(ids):
        out[b, :lens[u]] = flat[start[u]:start[u] + lens[u]]
    return out


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def run(cuda, stores, ids, t_maxs):
    from jatts_amd import hip
    srcs = [hip.CollateSource(torch.from_numpy(f).to(cuda), s, l) for f, s, l in stores]
    outs = []
    for (f, _, _), tm in zip(stores, t_maxs):
        dtype = torch.from_numpy(f[:0]).dtype
        outs.append(torch.full((len(ids), tm, f.shape[1]), float("nan") if dtype == torch.float32 else -1, dtype=dtype, device=cuda))
    got = hip.collate(srcs, ids, t_maxs, out=outs)
    assert all(g is o for g, o in zip(got, outs))
    for (f, s, l), tm, o in zip(stores, t_maxs, outs):
        want = torch.from_numpy(restate(f, s, l, ids, tm))
        assert o.shape == want.shape and o.dtype == want.dtype
        assert torch.equal(bits(o.cpu()), bits(want)), (f.shape, f.dtype, tm)
    return outs


def test_allocating_form_equals_the_prefilled_form(cuda):
    """``hip.collate`` without ``out`` (what the loader calls) allocates its destinations and writes the same bits."""
    from jatts_amd import hip
    stores = [make_store([3, 1, 5], 1, np.int64, seed=30), make_store([7, 1, 12], 80, np.float32, seed=31)]
    srcs = [hip.CollateSource(torch.from_numpy(f).to(cuda), s, l) for f, s, l in stores]
    for (f, s, l), o in zip(stores, hip.collate(srcs, [2, 0, 1])):
        assert torch.equal(bits(o.cpu()), bits(torch.from_numpy(restate(f, s, l, [2, 0, 1], int(l.max())))))
    with pytest.raises(ValueError, match="out"):
        hip.collate(srcs, [2, 0, 1], out=[torch.empty(3, 5, 1, dtype=torch.int64, device=cuda), torch.empty(3, 11, 80, device=cuda)])


@pytest.mark.parametrize("dim", [80, 1, 5, 6])
@pytest.mark.parametrize("t_max", [7, 9])
@pytest.mark.parametrize("lead", [0, 1])
def test_lengths_dims_and_alignment(cuda, dim, t_max, lead):
    """Lengths (1, 7, 4): t_max = 7 leaves no padding on the longest.  Rows of 1, 5 or 6 floats, and the leading row, put utterance starts off
    16 bytes (word path); dim 80 keeps every start on 16 bytes (vector path); slots of 7 * 5 or 9 * 1 words end in a partial 16-byte unit."""
    for dtype in (np.float32, np.int64):
        st = make_store([1, 7, 4], dim, dtype, seed=dim * 10 + t_max, lead=lead)
        run(cuda, [st], [0, 1, 2], [t_max])
        run(cuda, [st], [2, 0, 1], [t_max])


def test_single_utterance_batch_and_repeated_id(cuda):
    st = make_store([3, 5, 2], 80, np.float32, seed=1)
    run(cuda, [st], [1], [5])                       # B = 1
    run(cuda, [st], [2, 0, 2], [3])                 # the same id twice
    st = make_store([3, 5, 2], 1, np.int64, seed=2)
    run(cuda, [st], [1], [5])
    run(cuda, [st], [0, 0], [4])


def test_int64_above_2_32_negative_zero_and_nan_payload_survive(cuda):
    f, s, l = make_store([2, 3], 1, np.int64, seed=3)
    f[:, 0] = [(1 << 32) + 5, -(1 << 33) - 7, (1 << 62) + 1, 3, -1]
    out, = run(cuda, [(f, s, l)], [1, 0], [4])
    assert out[1, 0, 0].item() == (1 << 32) + 5 and out[0, 0, 0].item() == (1 << 62) + 1
    for dim in (4, 5):                              # vector path and word path
        f, s, l = make_store([2, 3], dim, np.float32, seed=4)
        w = f.view(np.uint32)
        f[0, 0] = -0.0
        w[3, 1] = 0x7FC12345                        # a quiet NaN with a payload
        w[3, 2] = 0xFF800001                        # a signalling NaN, sign set
        out, = run(cuda, [(f, s, l)], [0, 1], [3])
        got = out.cpu().numpy().view(np.uint32)
        assert got[0, 0, 0] == 0x80000000 and got[1, 1, 1] == 0x7FC12345 and got[1, 1, 2] == 0xFF800001


@pytest.mark.parametrize("dim", [4, 3, 80])
def test_nothing_behind_a_short_utterance_leaks_into_the_padding(cuda, dim):
    """A NaN-filled utterance that is not in the batch sits directly behind a short one that is: the padding is zero bits, not NaN (a padding
    that was loaded and multiplied by a mask would be NaN)."""
    f, s, l = make_store([1, 6, 2], dim, np.float32, seed=5)
    f[s[1]:s[1] + l[1]] = np.nan
    out, = run(cuda, [(f, s, l)], [0, 2], [6])
    assert not torch.isnan(out).any() and torch.equal(bits(out[:, 2:].cpu()), torch.zeros(2, 4, dim, dtype=torch.int32))


def test_three_fields_of_different_geometry_in_one_launch(cuda):
    lens_tok, lens_mel = [3, 1, 5], [7, 1, 12]
    stores = [make_store(lens_tok, 1, np.int64, seed=6), make_store(lens_mel, 80, np.float32, seed=7),
              make_store(lens_tok, 1, np.float32, seed=8, lead=1)]
    run(cuda, stores, [2, 0, 1], [5, 12, 6])


def test_max_fields_in_one_launch(cuda):
    from jatts_amd import _abi
    stores = [make_store([2, 4, 3], 1 + i, np.float32 if i % 2 else np.int64, seed=20 + i, lead=i % 3) for i in range(_abi.COLLATE_MAX_FIELDS)]
    run(cuda, stores, [1, 2, 0, 1], [4 + i % 2 for i in range(_abi.COLLATE_MAX_FIELDS)])


def test_more_rows_than_a_grid_dimension_holds(cuda):
    """n_batch * t_max = 90 000 > 65 535 at dim = 1, and 30 000 words a slot: eight workgroups per slot, the last one partial."""
    st = make_store([30000, 29999, 17], 1, np.float32, seed=9)
    run(cuda, [st], [0, 1, 2], [30000])
    st = make_store([4100, 3], 3, np.int64, seed=10)        # int64 rows across a workgroup's edge (4096 words), word path and vector path
    run(cuda, [st], [1, 0], [4100])


def test_argument_errors_raise_before_any_launch(cuda):
    from jatts_amd import _abi, hip
    f, s, l = make_store([1, 7, 4], 5, np.float32, seed=11)
    src = hip.CollateSource(torch.from_numpy(f).to(cuda), s, l)
    with pytest.raises(ValueError, match="t_max"):
        hip.collate([src], [0, 1], [6])
    with pytest.raises(ValueError, match="id"):
        hip.collate([src], [0, 3], [7])
    with pytest.raises(ValueError, match="id"):
        hip.collate([src], [-1], [7])
    with pytest.raises(ValueError, match="dim"):
        hip.collate([hip.CollateSource(torch.empty(12, 0, device=cuda), s, l)], [0], [7])
    with pytest.raises(ValueError, match="fields"):
        hip.collate([src] * (_abi.COLLATE_MAX_FIELDS + 1), [0], [7] * (_abi.COLLATE_MAX_FIELDS + 1))
    with pytest.raises(ValueError, match="elem_bytes"):
        hip.collate([hip.CollateSource(torch.zeros(12, 5, dtype=torch.int16, device=cuda), s, l)], [0], [7])
    # the library's own checks (the wrapper's are in front of them): JATTS_ERR_ARG, nothing launched
    lib = _abi.load()
    dst = torch.empty(1, 7, 5, device=cuda)
    utt = torch.zeros(1, dtype=torch.int32, device=cuda)
    good = (src.src.data_ptr(), src.row_start.data_ptr(), src.row_len.data_ptr(), dst.data_ptr(), 4, 5, 7)
    for bad in ((4, 2), (5, 0), (6, 0), (0, None), (3, None)):
        a = list(good)
        a[bad[0]] = bad[1]
        tab = (_abi.CollateField * 1)(_abi.CollateField(*a))
        assert lib.jatts_collate(tab, 1, utt.data_ptr(), 1, None) == -1, bad
    tab = (_abi.CollateField * 9)(*[_abi.CollateField(*good)] * 9)
    assert lib.jatts_collate(tab, 9, utt.data_ptr(), 1, None) == -1 and lib.jatts_collate(tab, 0, utt.data_ptr(), 1, None) == -1
    assert lib.jatts_collate(tab, 1, utt.data_ptr(), 0, None) == -1 and lib.jatts_collate(tab, 1, None, 1, None) == -1
