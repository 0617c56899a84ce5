"""The capture policy of jatts_amd/graphs.py as host-only bookkeeping (GraphPolicy: sightings, the once-seen bound, least-recently-used eviction,
sticky eager-only markers, limits read live), and the two facts the trainers' eager and replayed steps must agree on: the loss-schedule phase
(training.loss_phase) and the dropout base seed (hip.dropout_base_seed).  No GPU; every expected decision is written out by hand."""
import types

import torch

from jatts_amd.graphs import GraphPolicy

E, C, R = "eager", "capture", "replay"


def _policy(max_graphs, max_seen=64):
    """-> the policy and its owner's limits, which the owner hands over with every decision."""
    return GraphPolicy(), types.SimpleNamespace(max_graphs=max_graphs, max_seen=max_seen)


def _drive(p, lim, keys):
    """What a GraphCache or a trainer does with each decision: a capture that succeeds stores its graph in the state it was handed."""
    acts = []
    for k in keys:
        act, st = p.decide(k, lim.max_graphs, lim.max_seen)
        assert (st is None) == (act == E) and (st is None or st is p.states[k])
        if act == C:
            st["graph"] = object()
        acts.append(act)
    return acts


def _live(p):
    return {k for k, v in p.states.items() if v.get("graph") is not None}


def test_first_sight_eager_second_captures_later_replay_and_lru_eviction():
    p, lim = _policy(2)
    assert _drive(p, lim, "aaabbb") == [E, C, R] * 2 and _live(p) == {"a", "b"}
    assert _drive(p, lim, "ccc") == [E, C, R] and _live(p) == {"b", "c"}            # c's capture evicted a ...
    assert p.states["a"] == {"graph": None}                                   # ... back to a once-seen signature: no new eager sight
    assert _drive(p, lim, "aaa") == [C, R, R] and _live(p) == {"c", "a"}            # a's capture evicted b
    assert len(p.states) == 3                                                  # 4 captures in all: a, b, c, a


def test_eviction_follows_use_not_capture_time():
    p, lim = _policy(2)
    assert _drive(p, lim, "aabb" + "a" + "cc") == [E, C, E, C, R, E, C]
    assert _live(p) == {"a", "c"} and p.states["b"] == {"graph": None}


def test_once_seen_signatures_are_bounded_and_the_purge_spares_graphs_and_eager_only():
    n = 8
    p, lim = _policy(2, max_seen=n)
    assert _drive(p, lim, ["g", "g", "bad", "bad"]) == [E, C, E, C]
    p.fail("bad")                                    # what capture() does when an exception leaves the body
    once = [f"s{i}" for i in range(2 * n)]
    for i, k in enumerate(once):
        assert _drive(p, lim, [k]) == [E]
        assert len(p.states) <= n
        if i == n - 3:                               # g, bad + n - 2 once-seen signatures: full, nothing purged yet
            assert list(p.states) == ["g", "bad"] + once[: n - 2]
        if i == n - 2:                               # the next first sight dropped the n // 2 oldest once-seen ones
            assert list(p.states) == ["g", "bad"] + once[n // 2: n - 1]
    assert _live(p) == {"g"} and p.states["bad"] == {"graph": None, "eager_only": True}
    assert once[0] not in p.states and once[-1] in p.states
    assert _drive(p, lim, ["g", "bad", once[0]]) == [R, E, E]      # (a purged signature starts over)


def test_eager_only_is_sticky():
    n = 4
    p, lim = _policy(2, max_seen=n)
    assert _drive(p, lim, "xx") == [E, C]
    p.fail("x")
    assert p.states["x"] == {"graph": None, "eager_only": True} and _live(p) == set()
    for i in range(3 * n):                           # several purges later
        assert _drive(p, lim, [f"s{i}", "x"]) == [E, E]
    assert _drive(p, lim, "xxx") == [E, E, E] and p.states["x"].get("eager_only")


def test_limits_are_read_live():
    p, lim = _policy(2)
    assert _drive(p, lim, "aabb") == [E, C, E, C] and _live(p) == {"a", "b"}
    lim.max_graphs = 1
    assert _drive(p, lim, "cc") == [E, C] and _live(p) == {"c"}
    lim.max_seen = 2                                 # a, b (evicted: once-seen again) and c fill more than the new bound
    assert _drive(p, lim, "d") == [E] and list(p.states) == ["b", "c", "d"]


def test_graph_cache_is_freed_with_its_last_reference():
    import weakref
    from jatts_amd.graphs import GraphCache
    c = GraphCache(max_graphs=2)
    r = weakref.ref(c)
    del c
    assert r() is None            # no cycle through the policy: the graphs' device memory goes when the owner goes


def test_loss_phase_at_both_thresholds():
    from jatts_amd.training import loss_phase
    dp, bn = 5, 9
    want = {dp - 1: (False, True, False), dp: (False, False, False), dp + 1: (True, False, False),
            bn - 1: (True, False, False), bn: (True, False, False), bn + 1: (True, False, True)}
    for steps, flags in want.items():
        ph = loss_phase(steps, dp, bn)
        assert list(ph) == ["duration_loss", "forward_sum", "bin_loss"]        # (this order is the graph signature's)
        assert (ph["duration_loss"], ph["forward_sum"], ph["bin_loss"]) == flags, steps
    # the binarisation loss does not wait for the duration loss
    assert tuple(loss_phase(3, 9, 5).values()) == (False, True, False) and tuple(loss_phase(6, 9, 5).values()) == (False, True, True)


def test_dropout_base_seed_is_the_forward_contexts():
    from jatts_amd import hip
    from jatts_amd.models.fastspeech2_train import _Ctx
    for s in (0, 1, 2, 17, 4096, 123456789):
        assert hip.dropout_base_seed(s, 0) == _Ctx(torch.nn.Linear(1, 1), s).seed == s * 4099 * 1000003
        for rank in (1, 7):
            assert hip.dropout_base_seed(s, rank) - hip.dropout_base_seed(s, 0) == rank * 1000003
