"""GPU: the sliding ("carried-halo") form of the emulated fused dilation unit (jatts_resunit_desc.variant = 2, csrc/resunit_emul16_impl.h) is bit-identical
to the windowed form (variant = 1) -- every output column's contractions run the same taps and K-steps in the same order in both.

The shapes cover every tile of resunit_emul16 (C = 32 / 64 / 128 / 256, k = 3 / 7 / 11, dilation 1 / 3 / 5, the channel-halves tile at C = 256, k = 11,
dilation 5), the residual-register tiles, both product counts and the MRF-mean store pass.  The ragged batches hold enough rows for several windows per
run, so runs start mid-sequence and cross sequence boundaries, with lengths off multiples of 16 and sequences shorter than one window and than the halo."""
import pytest
import torch

pytestmark = pytest.mark.gpu

RATES = {256: 8, 128: 64, 64: 128, 32: 256}     # HiFi-GAN v1 22.05 kHz stage rates (bench.py: 64 utterances x 768 frames)
PATTERN = [1, 7, 33, 129, 1000, 2, 4001, 50, 12345, 3, 777, 16, 5]


def _ragged_lens(C):
    """~4 sliding windows per run (one run per resident workgroup: CUs x 1 at C >= 128 or k = 11, CUs x 2 below)."""
    target = {256: 4 * 256 * 64, 128: 4 * 256 * 128, 64: 4 * 512 * 128, 32: 4 * 512 * 256}[C]
    lens = []
    while sum(lens) < target:
        lens += PATTERN
    return lens


def _unit(cuda, C, k, seed):
    from jatts_amd import hip
    g = torch.Generator(device=cuda).manual_seed(seed)
    w1 = torch.randn(C, C, k, generator=g, device=cuda) / (C * k) ** 0.5
    w2 = torch.randn(C, C, k, generator=g, device=cuda) / (C * k) ** 0.5
    b1, b2 = torch.randn(C, generator=g, device=cuda) * 0.1, torch.randn(C, generator=g, device=cuda) * 0.1
    return hip.pack_unit_weight_bf16x3_k32(w1), b1, hip.pack_unit_weight_bf16x3_k32(w2), b2, g


def _both(cuda, rb, rate, C, k, d, seed, code=None, n_add=0):
    """(windowed, sliding) outputs of one unit launch on the same inputs."""
    from jatts_amd import hip
    code = hip.F32E if code is None else code
    p1, b1, p2, b2, g = _unit(cuda, C, k, seed)
    rows = rb.total * rate
    x = torch.randn(rows, C, generator=g, device=cuda)
    add = [torch.randn(rows, C, generator=g, device=cuda) for _ in range(n_add)] or None
    out = []
    for variant in (1, 2):
        y = torch.full_like(x, float("nan"))
        hip.hifigan_resunit(rb, rate, x, y, p1, b1, p2, b2, C, k, d, 0.1, code, add=add, out_scale=1.0 / 3.0 if add else 1.0, w_layout=1,
                            variant=variant)
        out.append(y)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("d", [1, 3, 5])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_sliding_equals_windowed_ragged(cuda, lib, C, k, d):
    from jatts_amd import hip
    rb = hip.RaggedBatch(_ragged_lens(C), cuda)
    yw, ys = _both(cuda, rb, 1, C, k, d, seed=C * 100 + k * 10 + d)
    assert torch.isfinite(yw).all(), "windowed: unwritten outputs"
    assert torch.equal(ys, yw), f"C={C} k={k} d={d}: sliding != windowed at {int((ys != yw).sum())} elements"


@pytest.mark.parametrize("n_add", [1, 2])
@pytest.mark.parametrize("C,k,d", [(32, 7, 3), (64, 11, 5), (64, 3, 1), (128, 11, 3), (256, 11, 5), (256, 7, 1)])
def test_sliding_equals_windowed_mrf_mean(cuda, lib, C, k, d, n_add):
    """The MRF-mean store pass (y = (unit(x) + add0 [+ add1]) * out_scale)."""
    from jatts_amd import hip
    rb = hip.RaggedBatch(_ragged_lens(C), cuda)
    yw, ys = _both(cuda, rb, 1, C, k, d, seed=7 + C + k + d, n_add=n_add)
    assert torch.isfinite(yw).all()
    assert torch.equal(ys, yw)


@pytest.mark.parametrize("C,k,d", [(32, 11, 5), (64, 7, 3), (128, 11, 1), (128, 3, 5), (256, 11, 5), (256, 11, 3)])
def test_sliding_equals_windowed_six_products(cuda, lib, C, k, d):
    from jatts_amd import hip
    rb = hip.RaggedBatch(_ragged_lens(C), cuda)
    yw, ys = _both(cuda, rb, 1, C, k, d, seed=3 * C + k + d, code=hip.F32E6)
    assert torch.isfinite(yw).all()
    assert torch.equal(ys, yw)


@pytest.mark.parametrize("C,k,d", [(32, 11, 5), (64, 11, 3), (64, 7, 1), (128, 11, 5), (128, 3, 1), (256, 11, 5), (256, 7, 3)])
def test_sliding_equals_windowed_bench_size(cuda, lib, C, k, d):
    """64 utterances x 768 frames at the stage rate (a uniform batch: the rectangular geometry, no host lengths)."""
    from jatts_amd import hip
    rb = hip.RaggedBatch([768] * 64, cuda)
    yw, ys = _both(cuda, rb, RATES[C], C, k, d, seed=11 * C + k + d)
    assert torch.isfinite(yw).all()
    assert torch.equal(ys, yw)


@pytest.mark.parametrize("lens", [[768], [200001], [5], [1]])
@pytest.mark.parametrize("C,k,d", [(128, 11, 5), (256, 11, 5), (64, 7, 3), (32, 3, 1)])
def test_sliding_equals_windowed_single_utterance(cuda, lib, C, k, d, lens):
    """One utterance: the B = 1 stage rows (fewer windows than runs), a long one (several windows per run), shorter than the halo."""
    from jatts_amd import hip
    rate = RATES[C] if lens == [768] else 1
    rb = hip.RaggedBatch(lens, cuda)
    yw, ys = _both(cuda, rb, rate, C, k, d, seed=C + k + d + lens[0])
    assert torch.isfinite(yw).all()
    assert torch.equal(ys, yw)


@pytest.mark.parametrize("C", [32, 64, 128, 256])
def test_library_picks_sliding_at_bench_size_windowed_at_b1(cuda, lib, C):
    """variant = 0: the sliding form for the bench-size launches of the C >= 128 tiles (the residual-register tiles stay windowed), the windowed form
    for a B = 1 utterance; variant 1 / 2 are taken as given."""
    from jatts_amd import hip
    p1, b1, p2, b2, _ = _unit(cuda, C, 11, 0)
    for B, want in ((64, 2 if C >= 128 else 1), (1, 1)):
        rb = hip.RaggedBatch([768] * B, cuda)
        x = torch.empty(rb.total * RATES[C], C, device=cuda)
        y = torch.empty_like(x)
        for variant, expect in ((0, want), (1, 1), (2, 2)):
            got = hip.resunit_variant(rb, RATES[C], x, y, p1, b1, p2, b2, C, 11, 1, 0.1, hip.F32E, w_layout=1, variant=variant)
            assert got == expect, (C, B, variant, got)
