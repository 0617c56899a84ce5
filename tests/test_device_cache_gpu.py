"""hip.DeviceCache on the GPU: a hit on another stream is ordered behind the build, a new entry during a graph capture is refused cleanly for
every cache the package owns, and a tensor lives in one cache under one spelling of its device.  (Bounds, eviction and keep(): tests/test_device_cache_cpu.py.)"""
import pytest
import torch

from jatts_amd.synthetic import FS2_SMALL

pytestmark = pytest.mark.gpu


def _cache(name):
    from jatts_amd import hip
    (c,) = [c for c in hip.device_caches() if c.name == name]
    return c


# ---- another stream sees a finished upload

def _private(cuda, m):
    from jatts_amd import hip
    c = hip.DeviceCache("private", max_entries=2)
    return lambda: c.get("k", cuda, lambda: torch.arange(1000, dtype=torch.int32, device=cuda) * m), [m * i for i in range(1000)]


def _h2d(cuda, m):
    from jatts_amd import hip
    vals = [70001 + m * i for i in range(32)]
    return lambda: hip.h2d(vals, torch.int32, cuda), vals


def _ragged(cuda, m):
    from jatts_amd import hip
    return lambda: hip.RaggedBatch([31, 10 + m], cuda).cu, [0, 31, 41 + m]


@pytest.mark.parametrize("user", [_private, _h2d, _ragged], ids=["private", "h2d", "RaggedBatch"])
def test_another_stream_sees_a_finished_upload(cuda, lib, user):
    """Stream A has milliseconds of fills queued in front of the build; stream B hits the entry at once and copies it out.  Only B is
    synchronised: the values are the built ones because B waited for the entry's event.  (The same exchange with other values and one
    fill runs first: a first pinned allocation, a first launch of a kernel or a first use of a stream may stall the host until the fills
    are through, and then there is nothing left to wait for -- the last line asserts that A was still busy when B had its copy queued.)"""
    from jatts_amd import hip
    hip.clear_device_caches()
    a, b = torch.cuda.Stream(cuda), torch.cuda.Stream(cuda)
    big = torch.empty(1 << 27, dtype=torch.float32, device=cuda)          # 512 MiB a fill
    for m, fills in ((3, 1), (7, 64)):                                    # the first pass only warms the streams, the allocators and the kernels
        get, expect = user(cuda, m)
        host = torch.full((len(expect),), -1, dtype=torch.int32).pin_memory()
        torch.cuda.synchronize()
        with torch.cuda.stream(a):
            for _ in range(fills):
                big.fill_(float(m))
            built = get()
            behind = torch.cuda.Event()
            behind.record(a)
        with torch.cuda.stream(b):
            hit = get()
            host.copy_(hit, non_blocking=True)
            in_flight = not behind.query()
        b.synchronize()
        assert hit is built and host.tolist() == expect, m
        torch.cuda.synchronize()
    assert in_flight, "stream A was through before stream B had its copy queued: nothing was ordered here"


# ---- a miss under capture

def _fs2(cuda):
    from helpers import golden_state, load_golden
    from jatts_amd.models import FastSpeech2
    _, keys = load_golden("fs2_small.npz")
    m = FastSpeech2(idim=20, **FS2_SMALL)
    m.load_state_dict(golden_state(keys, 0))
    return m.to(cuda).set_precision("fp32")


def _case_h2d(cuda):
    from jatts_amd import hip
    return _cache("hip.h2d"), lambda t: t + hip.h2d([3.0, 1.0, 4.0], torch.float32, cuda), 3


def _case_ragged(cuda):
    from jatts_amd import hip
    return _cache("RaggedBatch geometry"), lambda t: t + hip.RaggedBatch([5, 7], cuda).cu[1:].float(), 2


def _case_selection(cuda):
    from jatts_amd.alignments import frame_token_indices
    return _cache("alignments.frame_token_indices"), lambda t: t.index_select(0, frame_token_indices([2, 1], [3, 2], 2, 3, cuda)[1]) * 2, 6


def _case_pos_table(cuda):
    from jatts_amd.models import fastspeech2_train as ft
    return ft._POS_TABLES, lambda t: t + ft._pos_table("legacy", 8, 4, cuda).reshape(-1)[:8], 8


def _case_prior(cuda):
    from jatts_amd.models import matchatts_train as mt
    return mt._PRIOR_DEV, lambda t: t + mt.beta_binomial_prior_dev([3, 2], [5, 4], cuda)[0, 0], 3


def _case_conformer(cuda):
    enc = _fs2(cuda)._prepare()["enc"]

    def body(t):
        cap, per_layer = enc._pos(9)                                      # cap 128: the projections of 128 positions, per layer
        assert cap == 128
        return t + [p for p in per_layer if p is not None][0][1][0, :8].float()
    return enc._pos_cache, body, 8


@pytest.mark.parametrize("case", [_case_h2d, _case_ragged, _case_selection, _case_pos_table, _case_prior, _case_conformer],
                         ids=["h2d", "RaggedBatch", "frame_token_indices", "pos_table", "prior", "ConformerRunner"])
def test_a_miss_under_capture_is_refused_and_answered_eagerly(cuda, lib, case):
    """The entry is dropped between a signature's first (eager) and second (capturing) sight, so the capture meets a miss: the cache raises
    JattsHipError in Python before anything is recorded, builds and inserts nothing, GraphCache answers by eager launches and keeps the
    signature eager-only, nothing stays pinned, and another signature captures and replays as ever."""
    from jatts_amd import hip
    from jatts_amd._abi import JattsHipError
    from jatts_amd.graphs import GraphCache
    cache, body, n = case(cuda)
    x = torch.arange(n, dtype=torch.float32, device=cuda) + 0.5
    ref = body(x).clone()
    refused = []

    def fn(t):
        if not torch.cuda.is_current_stream_capturing():
            return body(t)
        try:
            return body(t)
        except JattsHipError as e:
            refused.append((len(cache), str(e)))
            raise
    gc = GraphCache(max_graphs=2)
    assert torch.equal(gc.run("a", fn, (x,)), ref) and gc.stats["eager"] == 1
    cache.clear()
    assert torch.equal(gc.run("a", fn, (x,)), ref)                         # the capturing sight
    assert gc.stats["failed"] == 1 and gc.stats["captured"] == 0 and gc._g["a"].get("eager_only") and len(gc) == 0, gc.stats
    assert hip._KEEP[0] is None
    assert len(refused) == 1 and refused[0][0] == 0, refused              # the cache did not grow during the failed capture
    assert cache.name in refused[0][1] and "outside the capture" in refused[0][1], refused
    assert len(cache) >= 1                                                # (the eager answer filled it again)
    assert torch.equal(gc.run("a", fn, (x,)), ref) and gc.stats["eager"] == 2 and gc.stats["failed"] == 1
    for _ in range(3):                                                    # eager, capture (all hits), replay
        assert torch.equal(gc.run("b", fn, (x,)), ref)
    assert gc.stats == dict(eager=3, captured=1, replayed=1, failed=1) and len(gc) == 1 and len(refused) == 1


# ---- one tensor, one cache

def test_one_tensor_lives_in_one_cache_under_one_spelling_of_its_device(cuda, lib):
    from jatts_amd import hip
    from jatts_amd.alignments import frame_token_indices
    hip.clear_device_caches()
    hip.h2d([1, 2, 3], torch.int32, cuda)
    uploads, geometry, selections = _cache("hip.h2d"), _cache("RaggedBatch geometry"), _cache("alignments.frame_token_indices")
    spelled = torch.device("cuda", torch.cuda.current_device())
    assert len(uploads) == 1
    a, b = hip.RaggedBatch([29, 31], "cuda"), hip.RaggedBatch([29, 31], spelled)
    assert a.cu is b.cu and a.cu.tolist() == [0, 29, 60] and len(geometry) == 1
    s, t = frame_token_indices([2, 1], [31, 30], 2, 32, "cuda"), frame_token_indices([2, 1], [31, 30], 2, 32, spelled)
    assert s[0] is t[0] and s[1] is t[1] and len(selections) == 1
    assert s[0].tolist() == [0, 1, 2] and s[1].tolist() == list(range(31)) + list(range(32, 62))
    assert len(uploads) == 1                                              # the geometry and the selection lists are not held twice
    assert hip.h2d([1, 2, 3], torch.int32, "cuda") is hip.h2d([1, 2, 3], torch.int32, spelled) and len(uploads) == 1
