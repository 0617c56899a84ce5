"""hipGraph replay of the B = 1 drop-in path (`model.inference(x)` / `vocoder.decode(mel)`, the calls of the reference's stage-4 loop,
jatts/bin/tts_decode.py:203-255), and the package's ONE capture policy: the trainers' graph mode (jatts_amd/training.py) runs on it too.

One 128-phoneme utterance is ~600 kernel launches of a few microseconds each: issued one by one from Python the GPU waits for the host
between most of them.  A segment of the path whose launch sequence depends only on its shape signature (T_text up to the length regulator,
T_feats behind it) is captured ONCE as a hipGraph -- through torch.cuda.graph, which supplies the capture stream and the graph's private
memory pool: plumbing, like the stream and the allocator everywhere else -- and replayed for every later utterance with that signature:
the same kernels in the same order on the same arithmetic, bit-identical to the eager launches (tests/test_graph_gpu.py).

Rules (tests/test_graph_policy_cpu.py):
  * a signature's FIRST sight runs eagerly -- it fills the bounded caches of device constants (hip.DeviceCache: uploads, ragged geometry,
    index lists, positional tables, priors), every one of which refuses a new entry during a capture -- its SECOND sight captures, later
    ones replay;
  * signatures seen once and never again are bounded: at `max_seen` entries the oldest never-captured ones are dropped;
  * least-recently-used graphs are dropped beyond `max_graphs` (each owns one call's activations); their next sight captures again;
  * every cached device tensor handed out during a capture is pinned by the graph's record (hip.keep_begin), the caches may evict.
    hip.DeviceCache.get is the one place that rule lives (with the bounds, the device key, the ordering behind an upload made on another
    stream and the refusal above); a new cache is an instance of it.  Only what is handed out DURING the capture is pinned: a tensor the
    caller looked up BEFORE the call is not recorded and is freed under the graph once the bounded caches drop it, so a captured function
    builds its own ragged geometry from the lengths (RaggedBatch(lens, dev) inside `fn`: a cache hit, recorded);
  * the key holds everything the launch sequence and its cached operands depend on -- besides the shapes, the positional table length of
    the conformer stacks (ConformerRunner.table_len), which regrows for good after a longer input and changes the table's values;
  * whatever leaves a capture as an exception marks the signature eager-only for good.  GraphCache logs it and answers the call by eager
    launches; the trainer lets it propagate;
  * GraphCache copies inputs into the graph's static buffers (stream-ordered) and hands outputs out as stream-ordered CLONES: a caller who
    keeps the mel of utterance n while utterance n + 1 replays the same graph sees its own values.
JATTS_INFER_GRAPH=0 switches the B = 1 mechanism off (every call eager)."""
import collections
import contextlib
import logging
import os

import torch

from . import hip

ENABLED = os.environ.get("JATTS_INFER_GRAPH", "1") != "0"


class GraphPolicy:
    """The rules as host-only bookkeeping: `states` maps key -> state dict, least recently used first.  The two limits are the owner's and
    come with every decision (no copies here, no reference back to the owner): it may change them on a live object."""

    def __init__(self):
        self.states = collections.OrderedDict()

    def decide(self, key, max_graphs, max_seen):
        """-> ("eager", None) | ("capture", state) | ("replay", state): what this sight of `key` does."""
        st = self.states.get(key)
        if st is None:
            if len(self.states) >= max_seen:            # (eager-only markers and graphs stay)
                for k in [k for k, v in self.states.items() if v.get("graph") is None and not v.get("eager_only")][: max_seen // 2]:
                    del self.states[k]
            self.states[key] = {"graph": None}
        if st is None or st.get("eager_only"):
            return "eager", None
        self.states.move_to_end(key)
        if st["graph"] is not None:
            return "replay", st
        live = [k for k, v in self.states.items() if v.get("graph") is not None]
        for k in live[: max(0, len(live) - max_graphs + 1)]:
            self.states[k] = {"graph": None}
        return "capture", st

    def fail(self, key):
        self.states[key] = {"graph": None, "eager_only": True}


@contextlib.contextmanager
def capture(policy, key, st):
    """The body's launches become st["graph"]; st["keep"] pins every cached device tensor the body is handed.  Any exception leaving the
    body, a KeyboardInterrupt too, marks `key` eager-only and goes on to the caller."""
    g = torch.cuda.CUDAGraph()
    st["keep"] = hip.keep_begin()
    try:
        torch.cuda.synchronize()
        with torch.cuda.graph(g):
            yield
    except BaseException:
        policy.fail(key)
        raise
    finally:
        hip.keep_end()
    st["graph"] = g


class GraphCache:
    def __init__(self, max_graphs=24, max_seen=4096):
        self.max_graphs, self.max_seen = int(max_graphs), int(max_seen)
        self.policy = GraphPolicy()
        self._g = self.policy.states                    # key -> state dict
        self.stats = dict(eager=0, captured=0, replayed=0, failed=0)

    def clear(self):
        self._g.clear()

    def __len__(self):
        return sum(1 for v in self._g.values() if v.get("graph") is not None)

    def run(self, key, fn, inputs):
        """outputs = fn(*inputs) for a launch sequence that depends on `key` only.  inputs: tuple of device tensors (contiguous); fn returns a
        tensor or a tuple of tensors / None.  -> the same structure, eagerly computed or replayed (clones of the graph's static outputs)."""
        act = "eager"
        if ENABLED and hip._PROF is None and not torch.cuda.is_current_stream_capturing():
            act, st = self.policy.decide(key, self.max_graphs, self.max_seen)
        if act == "eager":
            self.stats["eager"] += 1
            return fn(*inputs)
        if act == "capture":
            st["in"] = tuple(t.clone() for t in inputs)
            try:
                with capture(self.policy, key, st):
                    st["out"] = fn(*st["in"])
            except Exception as e:      # a capture that cannot be made (an upload the caches had evicted, a launch the runtime refuses to record):
                self.stats["failed"] += 1       # the same kernels, launched one by one; never a wrong result
                logging.warning("jatts_amd.graphs: capture of %r failed (%s: %s); this signature stays on eager launches", key, type(e).__name__, e)
                torch.cuda.synchronize()
                return fn(*inputs)
        self.stats["captured" if act == "capture" else "replayed"] += 1
        for dst, src in zip(st["in"], inputs):
            if dst.shape != src.shape or dst.dtype != src.dtype:
                raise ValueError(f"graph signature {key!r}: input {tuple(src.shape)} {src.dtype} does not match the captured {tuple(dst.shape)} {dst.dtype}")
            dst.copy_(src, non_blocking=True)
        st["graph"].replay()
        out = st["out"]
        if torch.is_tensor(out):
            return out.clone()
        return tuple(None if o is None else o.clone() for o in out)
