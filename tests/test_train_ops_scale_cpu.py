"""The exactness precondition of tests/test_train_ops_scale_gpu.py, proven from the inputs alone: for every integer case the sum of the
absolute values of the terms of each output element (plus the start pattern of an accumulating output) stays below 2**24 -- 2**53 for
the double accumulator of sumsq -- so every partial sum a kernel can form, in any order and with or without FMA, is an integer that f32
holds exactly, and the int64 reference is the expected value to the last bit."""
import pytest
import torch

import train_ops_scale_cases as K


@pytest.mark.parametrize("kc", K.ALL_INT, ids=K.case_id)
def test_every_partial_sum_of_the_integer_cases_is_exact(kc):
    kernel, case = kc
    inp = K.make(kernel, case)
    for name, t in inp.items():
        if torch.is_tensor(t) and t.dtype == torch.float32 and name != "mul":
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 4, (name, "inputs are integers, |x| <= 4")
    if "dy" in inp:
        assert float(inp["dy"].abs().max()) <= 3
    for name, (want, bound, acc) in K.reference(kernel, inp).items():
        assert want.dtype == torch.float64 and want.shape == bound.shape
        assert bool((want.abs() <= bound).all()), name
        worst = float(bound.max()) + (K.PATTERN_MAX if acc else 0)
        assert worst < K.limit(kernel, name), (name, worst)


def test_the_case_table_crosses_every_launcher_threshold():
    """Both sides of each size threshold of the launchers in csrc/train_ops.hip (and the exact boundary) have a case."""
    rows = {r for r, _ in K.COL}
    assert {1, 256, 257, 24576, 65536} <= rows and any(r > 65536 for r in rows)                       # gridDim.y: 1, 2, 96, 256, capped
    assert {1, 63, 64, 65, 81, 384, 1536} <= {d for _, d in K.COL}
    ln = {r for r, _ in K.LN}
    assert {1, 511, 512, 513, 8176, 8192, 8208, 24576} <= ln and any(d % 2 for _, d in K.LN) and any(d == 1536 for _, d in K.LN)
    qr = {b * t for b, t, _, _ in K.QKV}
    assert {16384, 16416, 24576} <= qr and any((h * d) % 2 for _, _, h, d in K.QKV)
    assert {512, 513, 768} <= {max(l) for l, _, k in K.DWCONV if k in (7, 31)}
    assert {7, 31} <= {k for _, _, k in K.DWCONV} and any(max(l) > 4096 and k not in (7, 31) for l, _, k in K.DWCONV)
    assert any(max(l) == 1024 for l, _ in K.SEQ_SUM) and any(max(l) == 1025 for l, _ in K.SEQ_SUM)
    assert {1, 4096, 4097, 4194304 + 3} <= set(K.SUMSQ)
    assert any(r > 1024 for r, _, _, _ in K.INDEX_ADD)
    assert any(t * d < 65536 for _, t, d in K.MLOSS) and any(t * d > 65536 for _, t, d in K.MLOSS)
    for lens in [l for l, *_ in K.DWCONV + K.SEQ_SUM] + [K.RECIPE_FRAMES]:
        assert min(lens) >= 1
    assert min(K.RECIPE_FRAMES) == 1 and max(K.RECIPE_FRAMES) == 768 and len(K.RECIPE_FRAMES) == 32
