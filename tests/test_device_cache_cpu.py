"""hip.DeviceCache, the one bounded cache of small device constants, on CPU tensors: eviction orders, the byte bound, the device key, one
build per key, and keep() on everything handed out.  (The stream ordering and the refusal under a capture need a GPU: tests/test_device_cache_gpu.py.)"""
import torch

from jatts_amd import hip


def _t(n, fill=0):
    return torch.full((n,), fill, dtype=torch.int32)          # 4 n bytes


def _fill(cache, keys, n=1):
    for k in keys:
        cache.get(k, "cpu", lambda: _t(n))


def _keys(cache):
    return [k for k, _ in cache._entries]


def test_oldest_first_eviction_ignores_hits():
    c = hip.DeviceCache("t", max_entries=3)
    _fill(c, "abc")
    _fill(c, "a")                    # a hit does not make "a" young
    _fill(c, "d")
    assert _keys(c) == ["b", "c", "d"] and len(c) == 3
    _fill(c, "ef")
    assert _keys(c) == ["d", "e", "f"]


def test_lru_eviction_keeps_what_was_hit():
    c = hip.DeviceCache("t", max_entries=3, lru=True)
    _fill(c, "abc")
    _fill(c, "a")
    _fill(c, "d")
    assert _keys(c) == ["c", "a", "d"]
    _fill(c, "c")
    _fill(c, "e")
    assert _keys(c) == ["d", "c", "e"] and len(c) == 3


def test_byte_bound_counts_every_tensor_of_a_value():
    c = hip.DeviceCache("t", max_bytes=400, lru=True)
    c.get("a", "cpu", lambda: _t(25))                             # 100 bytes
    c.get("b", "cpu", lambda: (_t(25), [_t(25), None, 7]))        # 200
    c.get("c", "cpu", lambda: _t(25))                             # 100: 400 in all, the bound holds
    assert _keys(c) == ["a", "b", "c"] and c._bytes == 400
    c.get("d", "cpu", lambda: _t(1))                              # 404: "a" goes
    assert _keys(c) == ["b", "c", "d"] and c._bytes == 304
    c.get("b", "cpu", None)                                       # young again
    c.get("e", "cpu", lambda: _t(50))                             # 504: "c" and "d" go, 400 left
    assert _keys(c) == ["b", "e"] and c._bytes == 400


def test_both_bounds_hold_together():
    c = hip.DeviceCache("t", max_entries=2, max_bytes=100)
    _fill(c, "ab", n=5)
    _fill(c, "c", n=5)
    assert _keys(c) == ["b", "c"]                                 # the entry bound
    _fill(c, "d", n=24)
    assert _keys(c) == ["d"] and c._bytes == 96                   # the byte bound: 20 + 96 > 100


def test_the_newest_entry_survives_alone_above_the_bound():
    c = hip.DeviceCache("t", max_bytes=100)
    _fill(c, "ab")
    big = c.get("big", "cpu", lambda: _t(100))
    assert _keys(c) == ["big"] and len(c) == 1 and c._bytes == 400
    assert c.get("big", "cpu", None) is big
    _fill(c, "c")
    assert _keys(c) == ["c"] and c._bytes == 4


def test_clear_and_len():
    c = hip.DeviceCache("t", max_entries=4, max_bytes=1000)
    assert len(c) == 0
    _fill(c, "abc")
    assert len(c) == 3 and c._bytes == 12
    c.clear()
    assert len(c) == 0 and c._bytes == 0
    _fill(c, "a")
    assert len(c) == 1 and c._bytes == 4


def test_build_runs_once_per_key_while_the_entry_lives():
    c = hip.DeviceCache("t", max_entries=2)
    calls = []

    def build(k):
        def f():
            calls.append(k)
            return _t(3, len(calls))
        return f
    a = c.get("a", "cpu", build("a"))
    assert all(c.get("a", "cpu", build("a")) is a for _ in range(5))
    c.get("b", "cpu", build("b"))
    assert c.get("a", "cpu", build("a")) is a and calls == ["a", "b"]
    c.get("c", "cpu", build("c"))                                 # evicts "a" (oldest first)
    a2 = c.get("a", "cpu", build("a"))
    assert calls == ["a", "b", "c", "a"] and a2 is not a and a.tolist() == [1] * 3 and a2.tolist() == [4] * 3


def test_a_build_that_raises_inserts_nothing():
    c = hip.DeviceCache("t", max_entries=2)

    def build():
        raise ValueError("no table")
    try:
        c.get("a", "cpu", build)
    except ValueError:
        pass
    else:
        raise AssertionError("the build's exception was swallowed")
    assert len(c) == 0
    assert c.get("a", "cpu", lambda: _t(1)).tolist() == [0]


def test_two_spellings_of_one_device_share_an_entry_and_two_devices_do_not():
    c = hip.DeviceCache("t", max_entries=8)
    builds = []

    def build(dev):
        def f():
            builds.append(dev)
            return torch.zeros(2, device=dev)
        return f
    a = c.get("k", "cpu", build("cpu"))
    assert c.get("k", torch.device("cpu"), build("cpu")) is a and len(c) == 1
    m = c.get("k", "meta", build("meta"))
    assert m is not a and m.device.type == "meta" and len(c) == 2
    assert c.get("k", torch.device("meta"), build("meta")) is m and c.get("k", "cpu", build("cpu")) is a
    assert builds == ["cpu", "meta"]
    assert hip.canonical_device("cpu") == hip.canonical_device(torch.device("cpu")) == torch.device("cpu")


def test_hit_and_miss_record_every_tensor_of_a_nested_value_for_the_capture():
    c = hip.DeviceCache("t", max_entries=2)
    x, y, z = _t(1), _t(2), _t(3)
    value = [None, ([x, y], z), 5, "legacy"]
    quiet = c.get("q", "cpu", lambda: _t(4))                      # no capture in progress: nothing is recorded anywhere
    assert hip._KEEP[0] is None
    kept = hip.keep_begin()
    try:
        assert c.get("v", "cpu", lambda: value) is value          # a miss
        assert [id(t) for t in kept] == [id(x), id(y), id(z)]
        assert c.get("v", "cpu", None) is value                   # a hit
        assert [id(t) for t in kept] == [id(x), id(y), id(z)] * 2
        assert c.get("q", "cpu", None) is quiet and kept[-1] is quiet
    finally:
        hip.keep_end()
    n = len(kept)
    c.get("v", "cpu", None)
    c.get("w", "cpu", lambda: _t(1))
    assert len(kept) == n == 7 and hip._KEEP[0] is None


def test_only_the_module_level_caches_are_registered():
    import jatts_amd.alignments  # noqa: F401
    import jatts_amd.models.fastspeech2_train  # noqa: F401
    import jatts_amd.models.matchatts_train  # noqa: F401
    n = len(hip.device_caches())
    private = hip.DeviceCache("t", max_entries=2)
    names = [c.name for c in hip.device_caches()]
    assert len(names) == n == len(set(names)) and private not in hip.device_caches()
    bounds = {c.name: (c.max_entries, c.max_bytes, c.lru) for c in hip.device_caches()}
    assert bounds == {"hip.h2d": (None, 8 << 20, True), "RaggedBatch geometry": (512, None, False),
                      "alignments.frame_token_indices": (64, None, False), "fastspeech2_train._pos_table": (64, None, False),
                      "matchatts_train.beta_binomial_prior_dev": (16, None, False)}
    c = hip.DeviceCache("t2", max_entries=2, register=True)
    try:
        _fill(c, "ab")
        hip.clear_device_caches()
        assert len(c) == 0 and c in hip.device_caches()
    finally:
        hip._DEVICE_CACHES.remove(c)


def test_the_cpu_users_of_the_module_caches_go_through_them():
    """frame_token_indices on the CPU: one entry per lengths, the same tensors on a repeat, whatever the spelling of the device."""
    from jatts_amd.alignments import _SELECTIONS, frame_token_indices
    _SELECTIONS.clear()
    ts, fs = frame_token_indices([2, 1], [3, 2], 2, 3, "cpu")
    assert ts.tolist() == [0, 1, 2] and fs.tolist() == [0, 1, 2, 3, 4] and ts.dtype == torch.int64
    ts2, fs2 = frame_token_indices([2, 1], [3, 2], 2, 3, torch.device("cpu"))
    assert ts2 is ts and fs2 is fs and len(_SELECTIONS) == 1
    _SELECTIONS.clear()
