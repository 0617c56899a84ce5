"""Tensor-level wrappers over the C ABI (jatts_amd/_abi.py).

PyTorch is used here only as plumbing: device memory (torch tensors), the current
HIP stream and dtype bookkeeping.  Every wrapper validates shapes, fills the POD
descriptor and launches asynchronously on ``torch.cuda.current_stream()``.
"""
import collections
import contextlib
import ctypes as C

import torch

from . import _abi
from . import precision as _precision
from ._abi import ACT_MISH, ACT_NONE, ACT_RELU, ACT_SWISH, ACT_TANH, F16, F32, F32E, F32E6, F32S  # noqa: F401
from .precision import EMUL, PRECISIONS  # noqa: F401  (EMUL: f32 tensors, three exact bf16 terms per operand, seven / six partial products: include/jatts_hip.h)

_TORCH = {F32: torch.float32, F16: torch.float16, F32S: torch.float32, F32E: torch.float32, F32E6: torch.float32}


def torch_dtype(code):
    return _TORCH[code]


def code_of(t):
    if t.dtype == torch.float32:
        return F32
    if t.dtype == torch.float16:
        return F16
    raise TypeError(f"unsupported dtype {t.dtype}")


# ---- optional live kernel timing (HIP events on the launch stream); used by bench.py only
_PROF = None


def profile_begin():
    global _PROF
    _PROF = []


def profile_end():
    """-> list of (tag, meta, milliseconds); synchronises the device."""
    global _PROF
    recs, _PROF = _PROF or [], None
    torch.cuda.synchronize()
    return [(tag, meta, a.elapsed_time(b)) for tag, meta, a, b in recs]


# ---- optional dense-FLOP tally of the MFMA launches (conv forward / dgrad / wgrad, attention); bench.py's training lines
_FLOPS = None


def flops_begin():
    global _FLOPS
    _FLOPS = 0.0


def flops_end():
    global _FLOPS
    v, _FLOPS = _FLOPS or 0.0, None
    return v


def _count(flops):
    global _FLOPS
    if _FLOPS is not None:
        _FLOPS += flops


# ---- zero pool for the training step: the small accumulators the reduction kernels add into (column sums, LayerNorm / GroupNorm
# parameter gradients, per-sequence sums ...) used to be one torch.zeros() each = one fill launch each (~550 of a FastSpeech2 step's
# 2 960 launches).  A trainer opens the pool at the top of a step: ONE fill zeroes the region the previous step used, and every
# accumulator is a 64-byte-aligned slice of it; slices are never handed out twice within a step, and nothing taken from the pool
# outlives the step (gradients are accumulated into the flat gradient buffer, saved statistics die with the graph).
class _ZeroPool:
    def __init__(self, device, floats=1 << 20):
        self.buf = torch.zeros(floats, dtype=torch.float32, device=device)
        self.off, self.high, self.misses = 0, 0, 0
        self.active = False
        self._retired = []        # outgrown buffers stay alive: captured graphs may still write into them

    def begin(self):
        """Zero everything any step has used so far (the high-water mark: a few hundred KB) and start handing out from the front.  Never
        allocates: safe inside a graph capture."""
        self.high = max(self.high, self.off)
        if self.high:
            self.buf[:self.high].zero_()
        self.off = 0

    def end(self):
        self.high = max(self.high, self.off)
        if self.misses:           # the step ran out (its overflow used torch.zeros): grow now, outside any capture
            self._retired.append(self.buf)
            self.buf = torch.zeros(max(2 * self.buf.numel(), 2 * (self.high + self.misses)), dtype=torch.float32, device=self.buf.device)
            self.misses = 0

    def take(self, numel):
        n = (numel + 15) & ~15
        if self.off + n > self.buf.numel():
            self.misses += n
            return None
        t = self.buf[self.off:self.off + numel]
        self.off += n
        return t


_ZPOOL = None


def zero_pool_begin(device):
    """Open (or re-arm) the device's zero pool: call at the top of a training step.  Pair with zero_pool_end()."""
    global _ZPOOL
    dev = torch.device(device)
    if dev.index is None:
        dev = torch.device(dev.type, torch.cuda.current_device())
    if _ZPOOL is None or _ZPOOL.buf.device != dev:
        _ZPOOL = _ZeroPool(dev)
    _ZPOOL.begin()
    _ZPOOL.active = True


def zero_pool_end():
    if _ZPOOL is not None:
        _ZPOOL.active = False
        if not torch.cuda.is_current_stream_capturing():
            _ZPOOL.end()


def _zeros(shape, device):
    """Zero-initialised f32 accumulator: a slice of the step's zero pool when one is open on ``device``, else torch.zeros."""
    shape = (shape,) if isinstance(shape, int) else tuple(shape)
    if _ZPOOL is not None and getattr(_ZPOOL, "active", False) and _ZPOOL.buf.device == device:
        n = 1
        for v in shape:
            n *= v
        t = _ZPOOL.take(n)
        if t is not None:
            return t.view(shape)
    return torch.zeros(shape, dtype=torch.float32, device=device)


class _Timed:
    def __init__(self, tag, meta):
        self.tag, self.meta = tag, meta

    def __enter__(self):
        if _PROF is not None:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if _PROF is not None:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            _PROF.append((self.tag, self.meta, self.a, b))


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


_WS = {}               # str(device) -> the zero-initialised scratch of the deterministic reductions (include/jatts_hip.h: jatts_scratch)
_WS_OWNER = {}         # str(device) -> (stream handle, event recorded behind that stream's last reduction launch)
WS_BYTES = 64 * 1024 + 96 * 1024 * 1024


@contextlib.contextmanager
def _scratch(device):
    """(Graph replays: a captured step bakes the scratch in and is ordered against other users only on the stream it was CAPTURED on -- replay a trainer's
    graph on its capture stream, which is what jatts_amd.training does; ownership is not tracked for replays on other streams.)
    Around a kernel that reduces across workgroups (LayerNorm / GroupNorm / SnakeBeta parameter gradients, column sums, depthwise-conv
    weights, the gradient norm): yields this device's jatts_scratch, by reference, for the call's `scratch` argument.  The buffer is
    allocated once, outside any graph capture (the trainers' first step of a signature runs eagerly), and kept alive for the life of the
    process -- a captured step bakes its address in."""
    key = str(device)
    capturing = torch.cuda.is_current_stream_capturing()
    buf = _WS.get(key)
    if buf is None:
        if capturing:
            raise _abi.JattsHipError("the reduction scratch must exist before a graph capture: run one eager step first")
        buf = _WS[key] = torch.zeros(WS_BYTES, dtype=torch.uint8, device=device)
        torch.cuda.current_stream(device).synchronize()
    # ONE scratch (tickets + slabs) per device: two streams reducing concurrently would corrupt each other's tickets silently.
    # The stream that used it last owns it; another stream first waits for that stream's last reduction (an event, no host sync).  During a
    # graph capture the scratch belongs to the capturing stream for the graph's whole life (the trainers capture on one stream).
    cur = None if capturing else torch.cuda.current_stream(device)
    if cur is not None:
        own = _WS_OWNER.get(key)
        if own is None or own[0] != cur.cuda_stream:
            if own is not None and not own[1].query():
                cur.wait_event(own[1])
            own = _WS_OWNER[key] = (cur.cuda_stream, torch.cuda.Event())
    try:
        yield C.byref(_abi.Scratch(buf.data_ptr(), buf.numel()))
    finally:          # launched or refused: how far the owning stream has got with the scratch (what another stream would wait for)
        if cur is not None:
            own[1].record(cur)


def _ptr(t, col0=0):
    if t is None:
        return None
    return t.data_ptr() + col0 * t.element_size()


def _dev(t):
    if not t.is_cuda:
        raise _abi.JattsHipError("jatts_amd kernels need device tensors (no CPU fallback)")
    return t


_KEEP = [None]        # while a graph is being captured (graphs.capture): every cached device tensor handed out (the graph bakes their addresses in)


def keep_begin():
    """Start recording the cached device tensors handed out from here on (every DeviceCache: uploads, ragged geometry, the models' per-length
    tables): a captured graph reads them at their addresses for as long as it is replayed, while the caches are bounded and evict -- the
    capture's owner keeps the returned list alive next to the graph (jatts_amd.graphs.capture, the only caller)."""
    _KEEP[0] = []
    return _KEEP[0]


def keep_end():
    _KEEP[0] = None


def keep(t):
    """Record t for the capture in progress, if there is one; returns t.  DeviceCache.get calls it for everything it hands out."""
    if _KEEP[0] is not None and t is not None:
        _KEEP[0].append(t)
    return t


_DEVICES = {}         # a spelling that names its index ("cuda:0", torch.device("cuda", 0), "cpu") -> the torch.device


def canonical_device(device):
    """The ONE spelling of a device: a torch.device that carries its index on the GPU ("cuda" and torch.device("cuda") mean the current
    device, now)."""
    dev = _DEVICES.get(device)
    if dev is None:
        dev = torch.device(device)
        if dev.type == "cuda" and dev.index is None:
            return torch.device("cuda", torch.cuda.current_device())
        _DEVICES[device] = dev
    return dev


_DEVICE_CACHES = []


class DeviceCache:
    """A bounded cache of small device constants that depend only on lengths (uploads, ragged offsets, index lists, positional tables,
    priors), and the one place the rules for such tensors live (jatts_amd/graphs.py relies on them):
      * the key holds the device, spelled one way (canonical_device);
      * bounded by entries and / or device bytes; the old end is evicted, never the entry just inserted; `lru` moves a hit to the young end;
      * an entry remembers the stream it was built on and an event behind the build: another stream that hits it first waits for the event;
      * a miss while the current stream is capturing raises -- nothing may be uploaded or built into a graph;
      * everything handed out, hit or miss, goes through keep(): a capture pins what it reads, the cache may evict it.
    On a device that is not a GPU only the bounds and keep() apply."""

    def __init__(self, name, max_entries=None, max_bytes=None, lru=False, register=False):
        self.name, self.max_entries, self.max_bytes, self.lru = name, max_entries, max_bytes, lru
        self._entries = collections.OrderedDict()     # (key, device) -> [value, its tensors, their bytes, event or None once complete, stream handle]; old end first
        self._bytes = 0
        if register:                                  # the module-level caches (device_caches); one owned by an object dies with it
            _DEVICE_CACHES.append(self)

    def __len__(self):
        return len(self._entries)

    def clear(self):
        self._entries.clear()
        self._bytes = 0

    def get(self, key, device, build):
        """The value of (key, device); build() makes it on a miss: a tensor, or nested tuples / lists of tensors, None, plain values and
        objects that own tensors."""
        dev = canonical_device(device)
        key = (key, dev)
        e = self._entries.get(key)
        if e is not None:
            if self.lru:
                self._entries.move_to_end(key)
            if e[3] is not None and not torch.cuda.is_current_stream_capturing():
                if e[3].query():
                    e[3] = None                       # complete: every stream may read it from now on
                elif e[4] != torch.cuda.current_stream(dev).cuda_stream:
                    torch.cuda.current_stream(dev).wait_event(e[3])
        else:
            cuda = dev.type == "cuda"
            if cuda and torch.cuda.is_current_stream_capturing():
                raise _abi.JattsHipError(f"{self.name}: a new entry while a graph is being captured: run the step once outside the capture first")
            value = build()
            leaves = _leaves(value, [])
            e = [value, leaves, sum(t.numel() * t.element_size() for t in leaves if torch.is_tensor(t)), None, None]
            if cuda:
                stream = torch.cuda.current_stream(dev)
                e[3], e[4] = torch.cuda.Event(), stream.cuda_stream
                e[3].record(stream)
            self._entries[key] = e
            self._bytes += e[2]
            while len(self._entries) > 1 and ((self.max_entries is not None and len(self._entries) > self.max_entries)
                                              or (self.max_bytes is not None and self._bytes > self.max_bytes)):
                self._bytes -= self._entries.popitem(last=False)[1][2]
        if _KEEP[0] is not None:
            for t in e[1]:
                keep(t)
        return e[0]


def _leaves(value, out):
    """Everything in a cached value that can own device memory (tensors, prepared operands), depth first."""
    if isinstance(value, (list, tuple)):
        for v in value:
            _leaves(v, out)
    elif value is not None and not isinstance(value, (int, float, str)):
        out.append(value)
    return out


def device_caches():
    """The package's module-level DeviceCaches."""
    return list(_DEVICE_CACHES)


def clear_device_caches():
    for c in _DEVICE_CACHES:
        c.clear()


def upload(values, dtype, device):
    """Host values -> a NEW device tensor WITHOUT stalling the host: staged through pinned memory and copied asynchronously on the
    current stream.  torch.tensor(values, device=...) copies from pageable memory, which blocks the host until everything already
    queued on the stream has run -- one pipeline drain per call in the middle of a forward pass.  Refused under a graph capture: the
    graph would hold a copy from a host buffer that is gone."""
    dev = canonical_device(device)
    if dev.type != "cuda":
        return torch.tensor(values, dtype=dtype, device=dev)
    if torch.cuda.is_current_stream_capturing():
        raise _abi.JattsHipError("h2d of new values while a graph is being captured: run the step once outside the capture first")
    return torch.tensor(values, dtype=dtype).pin_memory().to(dev, non_blocking=True)


def h2d(values, dtype, device):
    """upload() behind a cache.  Small length-derived lists repeat from step to step (same bucket of lengths): cached per (values, dtype,
    device), which also makes a training step capturable -- a hit issues no copy.  LRU, bounded by BYTES: a long decode run produces a
    new key per batch.  Anything else (long lists, arrays, tensors) is uploaded afresh."""
    dev = canonical_device(device)
    if dev.type == "cuda" and isinstance(values, (list, tuple)) and len(values) <= 65536 and all(isinstance(v, (int, float, bool)) for v in values[:1] + values[-1:]):
        return _UPLOADS.get((tuple(values), dtype), dev, lambda: upload(values, dtype, dev))
    return keep(upload(values, dtype, dev))


_UPLOADS = DeviceCache("hip.h2d", max_bytes=8 << 20, lru=True, register=True)      # device bytes; the host-side key tuples cost about 8x that
_GEOMETRY = DeviceCache("RaggedBatch geometry", max_entries=512, register=True)


def exclusive_scan(lens):
    """[0, l0, l0 + l1, ..., sum(lens)]: the offsets of a packed ragged batch (``RaggedBatch.cu_host``, ``features.PackedWaves.cu_host``)."""
    cu = [0]
    for v in lens:
        cu.append(cu[-1] + v)
    return cu


class RaggedBatch:
    """Packed ragged batch geometry: sequence b owns rows cu[b]..cu[b+1]-1.

    The device copy of ``cu`` is cached per (lengths, device): a forward / training step builds the same handful of geometries
    (``[T] * B`` padded forms, the valid-length forms) dozens of times, and every upload is a launch plus a pinned staging copy."""

    def __init__(self, lens, device):
        self.lens = [int(v) for v in lens]
        self.cu_host = cu = exclusive_scan(self.lens)
        self.total = cu[-1]
        self.n_seq = len(self.lens)
        self.max_len = max(self.lens) if self.lens else 0
        self.device = device
        dev = canonical_device(device)
        if dev.type != "cuda":
            self.cu = upload(cu, torch.int32, dev)
        else:
            self.cu = _GEOMETRY.get(tuple(self.lens), dev, lambda: upload(cu, torch.int32, dev))

    def struct(self, len_mul=1):
        if _RAGGED_1D and self.n_seq > 1 and min(self.lens) != self.max_len:     # a ragged batch: 1-D grids over its real tiles (jatts_ragged.host_lens)
            if not hasattr(self, "_lens_c"):
                self._lens_c = (C.c_int32 * self.n_seq)(*self.lens)               # (kept alive with the batch; read by the launchers only)
            return _abi.Ragged(self.cu.data_ptr(), self.n_seq, self.max_len, len_mul, self.total, C.addressof(self._lens_c))
        return _abi.Ragged(self.cu.data_ptr(), self.n_seq, self.max_len, len_mul, 0, None)

    def vt_layout(self):
        """(col0 int32 device tensor, ld): V^T column layout with every sequence starting on a multiple of 8 columns
        and 8 columns of slack at the end (jatts_relattn_desc.vt_col0)."""
        if not hasattr(self, "_vt"):
            col, c = [], 0
            for v in self.lens:
                col.append(c)
                c += round_up(v, 8)
            self._vt = (h2d(col or [0], torch.int32, self.device), c + 8)
        return self._vt


# 1-D grids over the real tiles of a ragged batch (jatts_ragged.total_rows); False: the rectangular grids (tests compare the two)
_RAGGED_1D = True


def round_up(v, m):
    return (v + m - 1) // m * m


def pack_conv_weight(w, dtype_code, c_mult=64):
    """(n_out, c_in, k) -> MFMA fragment order [tap][c/16][n/32][lane][8] (include/jatts_hip.h).

    c_in is zero-padded to a multiple of ``c_mult`` (64 for jatts_conv1d, whose LDS chunks are 64
    channels; 32 for the fused HiFi-GAN unit, which takes c_in == channels) and n_out to a
    multiple of 32.  Pure permutation + cast: done once per checkpoint at prepare time.
    """
    n, c, k = w.shape
    n_pad, c_pad = round_up(n, 32), round_up(c, c_mult)
    wp = torch.zeros(n_pad, c_pad, k, dtype=torch.float32, device=w.device)
    wp[:n, :c] = w.float()
    wp = wp.permute(2, 0, 1).reshape(k, n_pad // 32, 32, c_pad // 16, 2, 8)
    wp = wp.permute(0, 3, 1, 4, 2, 5).contiguous().reshape(-1)
    return wp.to(torch_dtype(dtype_code))


def pack_conv_weight_split(w, c_mult=32):
    """(n_out, c_in, k) f32 -> the JATTS_F32S operand of the fused HiFi-GAN unit: per output channel n a power-of-two scale
    2^s[n] puts max |w[n]| in [2^14, 2^15) (so that the lo halves stay normal f16 numbers over 18 binary orders of magnitude
    below the channel's largest weight); ws = w * 2^s[n] travels as hi = f16(ws), lo = f16(ws - hi) in the fragment order of
    pack_conv_weight with the two halves of a lane's 8 elements side by side: [tap][c/16][n/32][lane][hi x8 | lo x8].
    -> (packed f16 tensor, inverse scales 2^-s[n] as f32 (n_pad,)).  Pure scaling by powers of two, one rounding per half."""
    n, c, k = w.shape
    w = w.detach().float()
    n_pad = round_up(n, 32)
    amax = w.abs().reshape(n, -1).amax(dim=1)
    e = torch.frexp(amax)[1]                               # amax = m 2^e, m in [0.5, 1)
    s = torch.where(amax > 0, 15 - e, torch.zeros_like(e)).clamp(-60, 60).to(torch.int32)
    # 2^s and 2^-s assembled from their bit patterns: torch.ldexp goes through pow() on the GPU and is an ulp off for some exponents -- the
    # scales must be EXACT powers of two (tests/test_training_gpu.py::test_split_weight_packer_on_the_device_equals_the_host_packing)
    scale = ((127 + s) << 23).view(torch.float32)
    ws = w * scale.view(-1, 1, 1)
    hi = ws.half()
    lo = (ws - hi.float()).half()
    ph = pack_conv_weight(hi.float(), F16, c_mult).view(-1, 8)
    pl = pack_conv_weight(lo.float(), F16, c_mult).view(-1, 8)
    inv = torch.ones(n_pad, dtype=torch.float32, device=w.device)
    inv[:n] = ((127 - s) << 23).view(torch.float32)
    return torch.stack([ph, pl], dim=1).reshape(-1).contiguous(), inv.contiguous()


def bf16x3_terms(w):
    """f32 tensor -> (b0, b1, b2) bfloat16 tensors with b0 + b1 + b2 == w exactly (round-to-nearest-even at every step; both
    differences are exact in f32): 3 x 8 significand bits = f32's 24, f32's exponent range.  Holds for every finite value whose last
    bit lies at or above bf16's smallest subnormal (|w| >= 2^-110)."""
    w = w.detach().float()
    b0 = w.bfloat16()
    r1 = w - b0.float()
    b1 = r1.bfloat16()
    b2 = (r1 - b1.float()).bfloat16()
    return b0, b1, b2


def pack_conv_weight_bf16x3(w, c_mult=32):
    """(n_out, c_in, k) f32 -> the JATTS_F32E / JATTS_F32E6 operand: the three bf16 terms of every weight (bf16x3_terms: exact, no scales) in the
    fragment order of pack_conv_weight with a lane's 8 elements of each term side by side: [tap][c/16][n/32][lane][b0 x8 | b1 x8 | b2 x8]."""
    planes = [pack_conv_weight(t.float(), F32, c_mult).view(-1, 8).bfloat16() for t in bf16x3_terms(w)]   # bf16 -> f32 -> bf16 is exact
    return torch.stack(planes, dim=1).reshape(-1).contiguous()


def pack_unit_weight_bf16x3_k32(w):
    """(C, C, k) f32 -> the JATTS_F32E / JATTS_F32E6 fused-unit operand in the fragment order of the v_mfma_f32_16x16x32_bf16 kernels
    (jatts_resunit_desc.w_layout = 1, csrc/resunit_emul16_impl.h): [tap][c / 32][n / 16][lane = 16 ((c % 32) / 8) + n % 16][b0 x8 | b1 x8 | b2 x8] over c % 8."""
    n_out, c_in, k = w.shape
    if n_out % 16 or c_in % 32:
        raise ValueError("pack_unit_weight_bf16x3_k32: channels must be a multiple of 32")
    planes = []
    for t in bf16x3_terms(w):
        # (n, c, k) -> [k][c / 32][c % 32 / 8][c % 8][n / 16][n % 16] -> [k][c / 32][n / 16][c % 32 / 8][n % 16][c % 8]
        v = t.permute(2, 1, 0).reshape(k, c_in // 32, 4, 8, n_out // 16, 16).permute(0, 1, 4, 2, 5, 3)
        planes.append(v.reshape(-1, 8))
    return torch.stack(planes, dim=1).reshape(-1).contiguous()


def pack_conv_weight_bf16x3_k32(w, c_mult=64):
    """(n_out, c_in, k) f32 -> the JATTS_F32E / JATTS_F32E6 conv operand in the fragment order of the v_mfma_f32_16x16x32_bf16 kernels (jatts_conv_desc.w_layout = 1,
    csrc/conv1d_emul16.h): output channels zero-padded to 32, input channels to c_mult, then pack_unit_weight_bf16x3_k32's order."""
    n, c, k = w.shape
    n_pad, c_pad = round_up(n, 32), round_up(c, c_mult)
    wp = torch.zeros(n_pad, c_pad, k, dtype=torch.float32, device=w.device)
    wp[:n, :c] = w.detach().float()
    return pack_unit_weight_bf16x3_k32(wp)


class PreparedWeight:
    """A conv weight prepared for the kernel of dtype code ``code``: ``packed``, ``inv`` (the inverse scales of F32S, else None) and ``layout``
    (jatts_conv_desc.w_layout).  hip.conv1d recognises it in place of a packed f32 weight -- call sites stay `dtype=hip.F32` -- and takes that
    kernel; shapes it does not cover (conv_halo_fits) fall back, loudly never silently wrong, to the exact-f32 kernel on a lazily packed f32
    copy of the same weight."""
    inv, layout = None, 0

    def __init__(self, w, c_mult):
        self._src, self._c_mult, self._f32 = w.detach(), c_mult, None

    def f32(self):
        if self._f32 is None:
            self._f32 = pack_conv_weight(self._src, F32, self._c_mult)
        return self._f32


class SplitWeight(PreparedWeight):
    """A conv weight prepared for JATTS_F32S (the pair of pack_conv_weight_split)."""
    code = F32S

    def __init__(self, w, c_mult=64):
        super().__init__(w, c_mult)
        self.packed, self.inv = pack_conv_weight_split(w, c_mult)


class EmulWeight(PreparedWeight):
    """A conv weight prepared for JATTS_F32E / JATTS_F32E6 (pack_conv_weight_bf16x3: the three bf16 terms of every weight, exact; ``code`` picks
    seven or six partial products)."""

    def __init__(self, w, c_mult=64, code=F32E, layout=None):
        super().__init__(w, c_mult)
        self.code = code
        self.layout = (1 if c_mult % 64 == 0 else 0) if layout is None else layout      # jatts_conv_desc.w_layout
        self.packed = pack_conv_weight_bf16x3_k32(w, c_mult) if self.layout else pack_conv_weight_bf16x3(w, c_mult)


def conv_halo_fits(k_w, dil):
    """The ONE fallback rule of the split and emulated conv kernels: they stage a halo of at most 32 rows; a wider conv takes the exact-f32
    kernel on the same weight."""
    return (k_w - 1) * dil <= 32


_OPERAND = [F32]     # the operand code of `dtype=F32` conv call sites: F32 (packed exact f32), F32S (SplitWeight) or F32E / F32E6 (EmulWeight)


@contextlib.contextmanager
def operands(precision):
    """Inside: PackedConv(..., dtype=F32) packs the operands of ``precision`` -- a name of PRECISIONS, a precision.Precision record, or None for
    exact f32 (the dtype=F32 call sites of an f16-tensor precision are exact f32 too).  Nests."""
    rec = None if precision is None else _precision.record(precision)
    prev, _OPERAND[0] = _OPERAND[0], rec.operand if rec is not None and rec.tensors == F32 else F32
    try:
        yield
    finally:
        _OPERAND[0] = prev


def operand_code():
    """The operand code `dtype=F32` call sites pack for right now (hip.operands)."""
    return _OPERAND[0]


# Self-attention arithmetic, a switch of its own (the models' set_precision(precision, attention=...)).  None: what the precision name has always meant
# (fp32_split: the split f16 attention; every other name: exact f32 / f16 with the tensors) -- bit for bit.  "fp32": exact f32.  "fp32_bf16x3": the
# seven-product bf16x3 kernel (JATTS_F32E of jatts_relpos_attention) wherever emul_attention_wins says so, exact f32 elsewhere.
ATTENTION_PRECISIONS = ("fp32", "fp32_bf16x3")
ATTENTION_F32_PRECISIONS = tuple(sorted(n for n, p in _precision.TABLE.items() if p.tensors == F32))     # the precisions whose activations are f32 tensors
_ATTENTION = [None]


def check_attention_precision(precision, attention):
    """The models' set_precision argument check: raises ValueError for an unknown name or for an attention choice under f16 tensors."""
    if precision not in PRECISIONS:
        raise ValueError(precision)
    if attention is None:
        return
    if attention not in ATTENTION_PRECISIONS:
        raise ValueError(f"attention={attention!r}: None (what the precision implies) or one of {ATTENTION_PRECISIONS}")
    if precision not in ATTENTION_F32_PRECISIONS:
        raise ValueError(f"attention={attention!r} needs f32 activations: precision one of {ATTENTION_F32_PRECISIONS}, not {precision!r}")


@contextlib.contextmanager
def attention_precision(attention):
    """Inside: ConformerRunner / Matcha's transformer blocks are built with this attention arithmetic (see ATTENTION_PRECISIONS).  Nests."""
    prev, _ATTENTION[0] = _ATTENTION[0], attention
    try:
        yield
    finally:
        _ATTENTION[0] = prev


def emul_attention_wins(n_heads, d_k, rel_mode):
    """The ONE routing rule of attention="fp32_bf16x3": does the bf16x3 kernel beat the exact-f32 one for this launch family?  A function of the
    head geometry and the bias mode only -- never of a length or a batch size, so an utterance alone, the same utterance inside a batch and a
    replayed graph all take the same kernel.  The C ABI always honours the dtype it is given.

    Round 8 (profiles/r08_attn_by_shape.txt, r08_notes.md): timed alternately against the exact-f32 kernel, the first bf16x3 kernel is SLOWER on every
    launch the BASELINE configs make -- d_k 192 (FastSpeech2) 0.66 - 0.93 x, d_k 256 (Matcha) 0.57 - 0.68 x, d_k 96 (VITS text encoder) inside the 1 - 2 % run-to-run
    spread at T = 128 and 0.71 x at T = 768; d_k 128 0.99 x.  Only d_k 64 at T = 768 came out ahead (1.12 x against a 10 % spread
    of the exact-f32 timings in that session), a shape no config launches.  A shape inside the spread or slower stays on exact f32, so nothing is
    routed yet: attention="fp32_bf16x3" is accepted, keyed and plumbed, and computes what attention="fp32" computes until a faster kernel earns a
    True here."""
    return False


def attention_dtype(dtype, split, attention, n_heads, d_k, rel_mode):
    """dtype code of one relpos_attention call of the inference path: `dtype` / `split` are the runner's tensors and fp32_split flag, `attention` its
    attention choice (None = as the precision implies)."""
    if attention is None or dtype != F32:
        return F32S if split else dtype
    if attention == "fp32_bf16x3" and emul_attention_wins(n_heads, d_k, rel_mode):
        return F32E
    return F32


def operand(code, w, c_mult=64):
    """A conv weight prepared for operand code ``code``: SplitWeight (F32S), EmulWeight (F32E / F32E6) or the packed tensor of a plain dtype code."""
    return SplitWeight(w, c_mult) if code == F32S else EmulWeight(w, c_mult, code) if code in EMUL else pack_conv_weight(w, code, c_mult)


def f32_operand(w, c_mult=64):
    """A conv weight for `dtype=F32` call sites under the current hip.operands: packed exact f32, SplitWeight or EmulWeight."""
    return operand(_OPERAND[0], w, c_mult)


class PackedConv:
    """A Conv1d/Linear layer prepared for jatts_conv1d: the packed operand ``w``, the folded bias ``b``, the geometry (``c_in`` padded to c_mult,
    ``n_out``, ``k``) and the tensor dtype code it was packed for.  Calling it is the launch: ``layer(rb, xs, act=..., resid=..., out=...)``."""

    def __init__(self, w, b, dtype, device, scale=None, shift=None, c_mult=64):
        # w: (n, c, k) or (n, c); optional per-output-channel affine folded in (BatchNorm eval)
        w = w.detach().float()
        if w.dim() == 2:
            w = w.unsqueeze(-1)
        b = None if b is None else b.detach().float()
        if scale is not None:
            w = w * scale.view(-1, 1, 1)
            b = (b * scale if b is not None else torch.zeros_like(scale)) + shift
        self.dtype = dtype
        self.n_out, c, self.k = w.shape
        self.c_in = round_up(c, c_mult)
        # set_precision("fp32_split"): f32 tensors, split f16 hi/lo MFMA operands (hip.operands is on while the model prepares)
        # set_precision("fp32_bf16x3"): f32 tensors, three exact bf16 terms per operand, seven (fp32_bf16x3_6p: six) MFMA products (EmulWeight)
        self.w = f32_operand(w.to(device), c_mult) if dtype == F32 else pack_conv_weight(w.to(device), dtype, c_mult)
        self.b = None if b is None else b.to(device).contiguous()

    def __call__(self, rb, xs, **kw):
        """hip.conv1d on this layer: the keywords are the launch's own (inputs' layout, activation, residual, output placement); ``bias=`` overrides
        the folded bias (None: launch without one)."""
        kw.setdefault("bias", self.b)
        return conv1d(rb, xs, self.w, self.c_in, self.n_out, self.k, dtype=self.dtype, **kw)


def _pack_dev_args(w, c_mult, dgrad):
    """The shared opening of the device packers: -> (library, contiguous f32 device weight, its (n, c, k), padded n_out and c_in of the packed conv)."""
    lib = _abi.load()
    w = _dev(w)
    if w.dtype != torch.float32 or not w.is_contiguous():
        w = w.float().contiguous()
    n, c, k = w.shape
    pn, pc = (c, n) if dgrad else (n, c)
    return lib, w, (n, c, k), round_up(pn, 32), round_up(pc, c_mult)


def pack_conv_weight_dev(w, dtype_code, c_mult=64, dgrad=False):
    """pack_conv_weight as ONE HIP launch on a device f32 weight (n_out, c_in, k); dgrad=True packs the data-gradient operand
    W'[c][n][k-1-tap] directly (no permute / flip copies).  -> (packed, padded c_in of the packed conv)."""
    lib, w, (n, c, k), n_pad, c_pad = _pack_dev_args(w, c_mult, dgrad)
    out = torch.empty(k * n_pad * c_pad, dtype=torch_dtype(dtype_code), device=w.device)
    _abi.check(lib.jatts_pack_conv_weight(w.data_ptr(), n, c, k, c_mult, int(dgrad), dtype_code, out.data_ptr(), _stream()),
               "jatts_pack_conv_weight")
    return out, c_pad


def pack_conv_weight_split_dev(w, c_mult=64, dgrad=False):
    """pack_conv_weight_split on the device (two launches: per-row maxima, pack), for weights that change every step (training).
    -> (packed f16, inverse scales f32 (n_pad,), padded c_in of the packed conv)."""
    lib, w, (n, c, k), n_pad, c_pad = _pack_dev_args(w, c_mult, dgrad)
    out = torch.empty(2 * k * n_pad * c_pad, dtype=torch.float16, device=w.device)
    inv = torch.empty(n_pad, dtype=torch.float32, device=w.device)
    _abi.check(lib.jatts_pack_conv_weight_split(w.data_ptr(), n, c, k, c_mult, int(dgrad), out.data_ptr(), inv.data_ptr(), _stream()),
               "jatts_pack_conv_weight_split")
    return out, inv, c_pad


def pack_conv_weight_bf16x3_dev(w, c_mult=64, dgrad=False):
    """pack_conv_weight_bf16x3_k32 (the JATTS_F32E operand, jatts_conv_desc.w_layout = 1) as ONE HIP launch on a device f32 weight (n_out, c_in, k), for
    weights that change every step (training): bit for bit the host packing.  dgrad=True packs the data-gradient operand W'[c][n][k-1-tap] directly.
    -> (packed bf16, padded c_in of the packed conv)."""
    lib, w, (n, c, k), n_pad, c_pad = _pack_dev_args(w, c_mult, dgrad)
    out = torch.empty(3 * k * n_pad * c_pad, dtype=torch.bfloat16, device=w.device)
    _abi.check(lib.jatts_pack_conv_weight_bf16x3(w.data_ptr(), n, c, k, c_mult, int(dgrad), out.data_ptr(), _stream()), "jatts_pack_conv_weight_bf16x3")
    return out, c_pad


class TrainWeight(PreparedWeight):
    """A conv weight that changes every step (training): a device f32 weight (n_out, c_in, k) for operand code F32 / F32S / F32E, packed by the device
    packers above; dgrad=True: the data-gradient operand W'[c][n][k-1-tap].  ``c_in`` is the padded c_in of the packed conv.  Packs lazily and only
    the form hip.conv1d launches: ``packed`` / ``inv`` where the halo fits, f32() where it does not -- one packing per conv either way."""

    def __init__(self, w, code, dgrad=False, c_mult=64):
        if code not in (F32, F32S, F32E):
            raise ValueError(f"TrainWeight: operand code {code} (F32, F32S or F32E)")
        super().__init__(w, c_mult)
        self.code, self.layout, self._dgrad, self._pair = code, int(code == F32E), dgrad, None      # (jatts_conv_desc.w_layout 1: the F32E device packing)
        self.c_in = round_up(w.shape[0 if dgrad else 1], c_mult)

    def _pack(self):
        if self._pair is None:
            if self.code == F32S:
                self._pair = pack_conv_weight_split_dev(self._src, self._c_mult, self._dgrad)[:2]
            elif self.code == F32E:
                self._pair = (pack_conv_weight_bf16x3_dev(self._src, self._c_mult, self._dgrad)[0], None)
            else:
                self._pair = (self.f32(), None)
        return self._pair

    packed = property(lambda self: self._pack()[0])
    inv = property(lambda self: self._pack()[1])

    def f32(self):
        if self._f32 is None:
            self._f32 = pack_conv_weight_dev(self._src, F32, self._c_mult, self._dgrad)[0]
        return self._f32


def _polyphase_taps(K, stride, padding):
    """The (phase r, input offset q) pairs of ConvTranspose1d(K, stride, padding): output step j * stride + r takes w[..., stride * q + r + padding] from
    input row j - q.  -> (pairs, qmin, qmax); the polyphase conv holds the pair (r, q) at tap qmax - q."""
    qs = [(r, q) for r in range(stride) for q in range(-K, K + 1) if 0 <= stride * q + r + padding < K]
    return qs, min(q for _, q in qs), max(q for _, q in qs)


def convtranspose_tap_groups(K, stride, padding):
    """The tap windows of convtranspose_as_conv's weight, from its structure alone (never from weight values): the phases' real taps are a contiguous
    window each; when the phases 0 .. a - 1 share one window, the phases a .. stride - 1 another, and both are equally long,
    -> (a, first tap of group A, first tap of group B, taps per group) -- with c_out output channels per phase, jatts_conv_desc's tap_group_n = a * c_out,
    tap_a0, tap_b0, tap_k.  K = 2 stride: two taps each, {0, 1} then {1, 2}.  Any other pattern (one window for every phase, three windows, unequal
    lengths, holes) -> None."""
    qs, _, qmax = _polyphase_taps(K, stride, padding)
    wins = []
    for r in range(stride):
        taps = sorted(qmax - q for rr, q in qs if rr == r)
        if not taps or taps != list(range(taps[0], taps[-1] + 1)):
            return None
        wins.append((taps[0], len(taps)))
    a = next((r for r in range(stride) if wins[r] != wins[0]), stride)
    if a == stride or any(wn != wins[a] for wn in wins[a:]) or wins[0][1] != wins[a][1]:
        return None
    return a, wins[0][0], wins[a][0], wins[0][1]


def check_tap_window(wc, tap_window):
    """Raises ValueError unless the dense conv weight wc (n_out, c_in, k_w) is zero outside tap_window = (tap_group_n, tap_a0, tap_b0, tap_k): the promise
    jatts_conv_desc's hint makes (callers check ONCE, when they pack the weight)."""
    n, a0, b0, k = tap_window
    keep = torch.zeros(wc.shape[0], wc.shape[2], dtype=torch.bool, device=wc.device)
    keep[:n, a0:a0 + k] = True
    keep[n:, b0:b0 + k] = True
    if bool((wc != 0).any(1)[~keep].any()):
        raise ValueError(f"tap window {tuple(tap_window)}: the weight is not zero outside it")


def convtranspose_as_conv(w, stride, padding):
    """ConvTranspose1d weight (c_in, c_out, K) -> polyphase Conv1d weight
    (stride*c_out, c_in, taps) + input offset `pad`, such that the conv output row j,
    viewed as [stride][c_out], equals output steps j*stride .. j*stride+stride-1."""
    c_in, c_out, K = w.shape
    qs, qmin, qmax = _polyphase_taps(K, stride, padding)
    taps = qmax - qmin + 1
    wc = torch.zeros(stride * c_out, c_in, taps, dtype=w.dtype, device=w.device)
    for r, q in qs:
        kk = stride * q + r + padding
        wc[r * c_out:(r + 1) * c_out, :, qmax - q] = w[:, :, kk].t()
    return wc, qmax


def conv1d(rb, xs, w_packed, c_in, n_out, k_w, *, dtype, dil=1, pad=None, bias=None, act=ACT_NONE,
           alpha=1.0, resid=None, out=None, out_f32=False, transposed=False, pre_lrelu=None,
           in_scale=1.0, ldx=None, x_col0=0, len_mul=1, out_ld=None, out_col0=0, out_rows=None, resid_col0=0,
           y_seq_col0=None, reflect=False, variant=0, w_inv=None, snake=None, split=None, w_layout=0, tap_window=None):
    """See jatts_conv1d in include/jatts_hip.h.  ``xs`` is a tensor or list of <=3 tensors.  dtype F32S: f32 tensors, ``w_packed`` / ``w_inv``
    from pack_conv_weight_split (c_mult 64).  ``snake`` = (exp(alpha), 1 / (exp(beta) + 1e-9)) f32 vectors of n_out: the SnakeBeta
    activation (the ``snakebeta`` op) applied in the epilogue instead of ``act``.  ``split`` = (n_split, ld2, seq_col0): TWO outputs from one launch
    (the Q | K | V projection): channels < n_split row-major as usual, channels >= n_split transposed into a (n_out - n_split, ld2) matrix with the V^T
    column layout ``seq_col0`` (RaggedBatch.vt_layout); returns (out, out2), fresh buffers or the caller's ``out=(out, out2)``.  ``pad`` (default: the "same" offset (k_w - 1) // 2 * dil) must lie in
    [0, (k_w - 1) * dil]; the library refuses anything else.  ``tap_window`` = (tap_group_n, tap_a0, tap_b0, tap_k): the caller's PROMISE that the weight
    is zero outside those taps (jatts_conv_desc.tap_group_n: a hint, same result with or without; check_tap_window verifies a dense weight)."""
    lib = _abi.load()
    if isinstance(xs, torch.Tensor):
        xs = [xs]
    if isinstance(w_packed, PreparedWeight):
        if dtype != F32:
            raise ValueError(f"conv1d: a {type(w_packed).__name__} goes with dtype F32 tensors")
        if conv_halo_fits(k_w, dil):
            dtype, w_inv, w_layout, w_packed, out_f32 = w_packed.code, w_packed.inv, w_packed.layout, w_packed.packed, True
        else:                                  # outside the split / emulated kernel's tiles: the exact-f32 kernel on the same weight
            w_packed = w_packed.f32()
    x0 = _dev(xs[0])
    rows = rb.total * len_mul
    tdt = torch_dtype(dtype)
    for x in xs:
        if x.dtype != tdt or not x.is_contiguous():
            raise ValueError(f"conv1d: inputs must be contiguous {tdt}")
    ldx = ldx if ldx is not None else x0.shape[-1]
    if x0.numel() < rows * ldx or max(x_col0 if isinstance(x_col0, (list, tuple)) else [x_col0]) + c_in > ldx:
        raise ValueError("conv1d: input too small for the ragged geometry")
    if pad is None:
        pad = (k_w - 1) // 2 * dil
    n_pad = round_up(n_out, 32)
    if dtype == F32S:
        if w_packed.dtype != torch.float16 or w_packed.numel() != 2 * n_pad * c_in * k_w or w_inv is None or w_inv.numel() != n_pad:
            raise ValueError("conv1d: F32S takes the (packed, inverse scales) pair of pack_conv_weight_split")
    elif dtype in EMUL:
        if w_packed.dtype != torch.bfloat16 or w_packed.numel() != 3 * n_pad * c_in * k_w:
            raise ValueError("conv1d: F32E / F32E6 take the packed bf16 terms of pack_conv_weight_bf16x3")
        out_f32 = True
    elif w_packed.dtype != tdt or w_packed.numel() != n_pad * c_in * k_w:
        raise ValueError("conv1d: packed weight has wrong dtype/size")
    odt = torch.float32 if out_f32 else tdt
    out2 = None
    if split is not None:
        n_split, ld2, col2 = split
        pair = isinstance(out, (tuple, list))              # out=(out, out2): the caller's own buffers (the store tests prefill both with canaries)
        if transposed or (out is not None and not pair) or resid is not None or n_split % 256 or not 0 < n_split < n_out:
            raise ValueError("conv1d: split takes a fresh row-major output (or the pair out=(out, out2)), no residual, n_split a multiple of 256 below n_out")
        if pair:
            out, out2 = out
            if out2.dtype != odt or not out2.is_contiguous() or out2.numel() < (n_out - n_split) * ld2:
                raise ValueError("conv1d: split: out2 must be a contiguous (n_out - n_split, ld2) buffer of the output dtype")
            if not out.is_contiguous() or out.numel() < rows * (out_ld or out.shape[-1]) or out_col0 + n_split > (out_ld or out.shape[-1]):
                raise ValueError("conv1d: split: out must hold rows x out_ld elements with the n_split-wide window inside a row")
        else:
            out = torch.empty(rows, out_ld or n_split, dtype=odt, device=x0.device)
            out2 = torch.empty(n_out - n_split, ld2, dtype=odt, device=x0.device)
    if out is None:
        if transposed:
            # slack columns of an aligned V^T layout stay uninitialised: the attention kernel masks every element
            # outside [0, T) after loading it (tests fill them with NaN)
            out = torch.empty(n_out, rows if out_ld is None else out_ld, dtype=odt, device=x0.device)
        else:
            out = torch.empty(rows if out_rows is None else out_rows, out_ld or n_out, dtype=odt, device=x0.device)
    if out.dtype != odt:
        raise ValueError("conv1d: output dtype mismatch")
    ldy = out.shape[-1] if out_ld is None else out_ld
    d = _abi.ConvDesc()
    d.rg = rb.struct(len_mul)
    d.dtype, d.n_in = dtype, len(xs)
    cols = x_col0 if isinstance(x_col0, (list, tuple)) else [x_col0] * len(xs)   # per-input first column (views into wider rows)
    for i, x in enumerate(xs):
        d.x[i] = _ptr(x, cols[i])
    d.pad_mode = _abi.PAD_REFLECT if reflect else _abi.PAD_ZERO
    d.variant = variant
    d.ldx, d.in_scale = ldx, in_scale
    d.pre_act = _abi.PRE_LRELU if pre_lrelu is not None else _abi.PRE_NONE
    d.pre_slope = pre_lrelu or 0.0
    d.w, d.c_in, d.n_out, d.k_w, d.dil, d.pad = w_packed.data_ptr(), c_in, n_out, k_w, dil, pad
    d.bias = _ptr(bias)
    d.act, d.alpha = act, alpha
    if snake is not None:
        if act != ACT_NONE or any(v.dtype != torch.float32 or v.numel() != n_out or not v.is_contiguous() for v in snake):
            raise ValueError("conv1d: snake takes two contiguous f32 vectors of n_out and replaces act")
        d.act, d.act_a, d.act_b = _abi.ACT_SNAKEBETA, snake[0].data_ptr(), snake[1].data_ptr()
    if resid is not None:
        if resid.dtype != torch.float32:
            raise ValueError("conv1d: residual must be f32")
        d.resid, d.ldr = _ptr(resid, resid_col0), resid.shape[-1]
    d.y, d.ldy = _ptr(out, out_col0), ldy
    d.y_is_f32, d.y_transposed = int(odt == torch.float32), int(transposed)
    d.y_seq_col0 = _ptr(y_seq_col0) if transposed else None
    d.w_inv = _ptr(w_inv) if dtype == F32S else None
    d.w_layout = w_layout if dtype in EMUL else 0
    if out2 is not None:
        d.n_split, d.ldy2, d.y2, d.y2_seq_col0 = split[0], split[1], out2.data_ptr(), _ptr(split[2])
    if tap_window is not None:
        d.tap_group_n, d.tap_a0, d.tap_b0, d.tap_k = tap_window
    _count(2.0 * c_in * n_out * k_w * rows)
    with _Timed("conv1d", (c_in, n_out, k_w, rows)):
        _abi.check(lib.jatts_conv1d(C.byref(d), _stream()), "jatts_conv1d")
    return out if out2 is None else (out, out2)


def _check_unit_weights(who, dtype, channels, k_w, *ws):
    """The packed operand a fused-unit dtype expects, element for element: the C entry point sees only a pointer, and an f32-packed weight (4 B per
    element) handed to an emulated kernel (three bf16 planes: 6 B) would be read out of bounds on the device."""
    n = channels * channels * k_w
    want = {F32: (torch.float32, n), F16: (torch.float16, n), F32S: (torch.float16, 2 * n), F32E: (torch.bfloat16, 3 * n), F32E6: (torch.bfloat16, 3 * n)}[dtype]
    for w in ws:
        if w.dtype != want[0] or w.numel() != want[1] or not w.is_cuda:
            raise ValueError(f"{who}: dtype code {dtype} needs packed weights of {want[1]} x {want[0]} on the GPU (pack_conv_weight / pack_conv_weight_split / "
                             f"pack_conv_weight_bf16x3 with c_mult=32), got {w.numel()} x {w.dtype}")


def _resunit_desc(rb, len_mul, x, y, w1, b1, w2, b2, channels, k_w, dil, slope, dtype, add, out_scale, ws, w_layout, variant):
    d = _abi.ResUnitDesc()
    d.w_layout, d.variant = w_layout, variant
    d.rg = rb.struct(len_mul)
    d.dtype, d.channels, d.k_w, d.dil, d.slope = dtype, channels, k_w, dil, slope
    rows = rb.total * len_mul
    if x.numel() != rows * channels or y.numel() != rows * channels or x.dtype != torch_dtype(dtype):
        raise ValueError("hifigan_resunit: bad buffer size/dtype")
    d.x, d.y = _dev(x).data_ptr(), y.data_ptr()
    # w2 None: the single-conv unit (use_additional_convs=False) -- w2 / b2 / ws2 go down as NULL and the library checks that they agree
    _check_unit_weights("hifigan_resunit", dtype, channels, k_w, *((w1,) if w2 is None else (w1, w2)))
    d.w1, d.b1, d.w2, d.b2 = w1.data_ptr(), b1.data_ptr(), _ptr(w2), _ptr(b2)
    if dtype == F32S:
        need = ws[:1] if ws is not None and w2 is None else ws      # (the single-conv unit has no F32S kernel: the library refuses it)
        if need is None or any(v is None or v.numel() < channels or v.dtype != torch.float32 for v in need):
            raise ValueError("hifigan_resunit: F32S needs the inverse weight scales (pack_conv_weight_split)")
        d.ws1, d.ws2 = ws[0].data_ptr(), _ptr(ws[1]) if len(ws) > 1 else None
    if add:
        for a in add:
            if a.numel() != rows * channels or a.dtype != x.dtype:
                raise ValueError("hifigan_resunit: bad mix buffer")
        d.add0 = add[0].data_ptr()
        d.add1 = add[1].data_ptr() if len(add) > 1 else None
    d.out_scale = out_scale
    return d


def hifigan_resunit(rb, len_mul, x, y, w1, b1, w2, b2, channels, k_w, dil, slope, dtype, add=None, out_scale=1.0, ws=None, w_layout=0, variant=0):
    """jatts_hifigan_resunit.  w2 = b2 = None: the single-conv unit y = x + conv_k,d(lrelu(x)) + b1 (F32, F16, F32E / F32E6 with w_layout 1).
    w_layout (F32E / F32E6): 0 = weights from pack_conv_weight_bf16x3(w, 32) (32 x 32 x 16 kernels), 1 = from
    pack_unit_weight_bf16x3_k32 (16 x 16 x 32 kernels).  variant (jatts_resunit_desc.variant): 0 = the library's choice, 1 = windowed, 2 = sliding."""
    lib = _abi.load()
    d = _resunit_desc(rb, len_mul, x, y, w1, b1, w2, b2, channels, k_w, dil, slope, dtype, add, out_scale, ws, w_layout, variant)
    with _Timed("resunit", (channels, k_w, dil, rb.total * len_mul, len(add) if add else 0)):
        _abi.check(lib.jatts_hifigan_resunit(C.byref(d), _stream()), "jatts_hifigan_resunit")
    return y


def resunit_variant(rb, len_mul, x, y, w1, b1, w2, b2, channels, k_w, dil, slope, dtype, add=None, out_scale=1.0, ws=None, w_layout=0, variant=0):
    """jatts_resunit_variant: the form hifigan_resunit with the same arguments would launch (1 = windowed, 2 = sliding); launches nothing."""
    lib = _abi.load()
    d = _resunit_desc(rb, len_mul, x, y, w1, b1, w2, b2, channels, k_w, dil, slope, dtype, add, out_scale, ws, w_layout, variant)
    rc = lib.jatts_resunit_variant(C.byref(d))
    _abi.check(min(rc, 0), "jatts_resunit_variant")
    return rc


def hifigan_resblock(rb, len_mul, x, y, units, channels, k_w, slope, dtype, add=None, out_scale=1.0, ws=None):
    """jatts_hifigan_resblock: ``units`` = [(w1, b1, w2, b2, dil), ...] (<= 3), all dilation units of one ResBlock in one launch.
    dtype F32S: ``ws`` = [(inverse scales of w1, of w2), ...] per unit (pack_conv_weight_split)."""
    lib = _abi.load()
    d = _abi.ResBlockDesc()
    d.rg = rb.struct(len_mul)
    d.dtype, d.channels, d.k_w, d.n_units, d.slope = dtype, channels, k_w, len(units), slope
    rows = rb.total * len_mul
    if x.numel() != rows * channels or y.numel() != rows * channels or x.dtype != torch_dtype(dtype):
        raise ValueError("hifigan_resblock: bad buffer size/dtype")
    d.x, d.y = _dev(x).data_ptr(), y.data_ptr()
    for i, (w1, b1, w2, b2, dil) in enumerate(units):
        _check_unit_weights("hifigan_resblock", dtype, channels, k_w, w1, w2)
        d.w1[i], d.b1[i], d.w2[i], d.b2[i], d.dil[i] = w1.data_ptr(), b1.data_ptr(), w2.data_ptr(), b2.data_ptr(), dil
    if dtype == F32S:
        if ws is None or len(ws) != len(units):
            raise ValueError("hifigan_resblock: F32S needs the inverse weight scales of every unit")
        for i, (a, b) in enumerate(ws):
            d.ws1[i], d.ws2[i] = a.data_ptr(), b.data_ptr()
    if add:
        for a in add:
            if a.numel() != rows * channels or a.dtype != x.dtype:
                raise ValueError("hifigan_resblock: bad mix buffer")
        d.add0 = add[0].data_ptr()
        d.add1 = add[1].data_ptr() if len(add) > 1 else None
    d.out_scale = out_scale
    with _Timed("resblock", (channels, k_w, tuple(u[4] for u in units), rows, len(add) if add else 0)):
        _abi.check(lib.jatts_hifigan_resblock(C.byref(d), _stream()), "jatts_hifigan_resblock")
    return y


def hifigan_output(rb, len_mul, xs, in_scale, slope, c_in, k_w, w, bias, dtype):
    lib = _abi.load()
    rows = rb.total * len_mul
    y = torch.empty(rows, dtype=torch.float32, device=xs[0].device)
    arr = (C.c_void_p * len(xs))(*[_dev(x).data_ptr() for x in xs])
    rg = rb.struct(len_mul)
    _abi.check(lib.jatts_hifigan_output(C.byref(rg), dtype, arr, len(xs), in_scale, slope, c_in, k_w,
                                        w.data_ptr(), float(bias), y.data_ptr(), _stream()),
               "jatts_hifigan_output")
    return y


def relpos_attention(rb, q, ldq, k, ldk, vt, ldvt, g, ldg, ku, scale, n_heads, d_k, dtype,
                     q_col0=0, k_col0=0, rel_mode=1, rel_center=0, vt_col0=None, kv_len=None):
    lib = _abi.load()
    out = torch.empty(rb.total, n_heads * d_k, dtype=torch_dtype(dtype), device=q.device)
    d = _abi.RelAttnDesc()
    d.rg = rb.struct()
    d.dtype, d.n_heads, d.d_k = dtype, n_heads, d_k
    d.q, d.ldq = _ptr(_dev(q), q_col0), ldq
    d.k, d.ldk = _ptr(k, k_col0), ldk
    d.vt, d.ldvt = vt.data_ptr(), ldvt
    d.g, d.ldg = _ptr(g), ldg
    d.ku = _ptr(ku)
    d.scale = scale
    d.out, d.ldo = out.data_ptr(), n_heads * d_k
    d.rel_mode, d.rel_center = rel_mode, rel_center
    d.vt_col0 = _ptr(vt_col0)
    d.kv_len = _ptr(kv_len)
    with _Timed("relattn", (n_heads, d_k, rb.total, sum(v * v for v in rb.lens))):
        _abi.check(lib.jatts_relpos_attention(C.byref(d), _stream()), "jatts_relpos_attention")
    return out


def rowdot(x, ldx, rows, n_heads, d_k, vec, col0=0):
    lib = _abi.load()
    out = torch.empty(rows, n_heads, dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_rowdot(code_of(x), _ptr(_dev(x), col0), ldx, rows, n_heads, d_k, vec.data_ptr(),
                                out.data_ptr(), _stream()), "jatts_rowdot")
    return out


_BAD_IDS = {}      # device index -> int64 (1,) counter of out-of-range embedding ids seen by launches that passed no counter of their own


def _bad_counter(dev):
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _BAD_IDS.get(key)
    if t is None:
        t = _BAD_IDS[key] = torch.zeros(1, dtype=torch.int64, device=dev)
    return t


def embed_scale(ids, table, scale, n_bad=None):
    """rows = table[ids] * scale.  The kernel ALWAYS bounds-checks: an id outside the table yields a zero row (never a read outside
    the table) and is counted -- in ``n_bad`` (int64 (1,) device counter zeroed by the caller, read at the caller's next host
    synchronisation: lr_sizes(..., check=n_bad)) or, when none is passed, in the device's shared counter, which
    check_bad_ids() / bad_ids_async() turn into the IndexError torch.nn.Embedding would have raised."""
    lib = _abi.load()
    if n_bad is None:
        n_bad = _bad_counter(_dev(ids).device)
    out = torch.empty(ids.numel(), table.shape[1], dtype=torch.float32, device=ids.device)
    _abi.check(lib.jatts_embed_scale(_dev(ids).data_ptr(), ids.numel(), table.data_ptr(), table.shape[1],
                                     float(scale), out.data_ptr(), table.shape[0], _ptr(n_bad), _stream()), "jatts_embed_scale")
    return out


def check_bad_ids(device):
    """Read the device's shared bad-id counter (a host synchronisation: call it right after one the caller needs anyway) and raise
    IndexError like torch.nn.Embedding if a launch since the last check saw an id outside its table."""
    t = _BAD_IDS.get(torch.device(device).index if torch.device(device).index is not None else torch.cuda.current_device())
    if t is None:
        return
    n = int(t)
    if n:
        t.zero_()
        raise IndexError(f"index out of range in self ({n} token ids outside the embedding table)")


def bad_ids_async(device):
    """Stream-ordered snapshot of the shared counter into pinned memory, no host wait.  -> resolve() which raises IndexError once the
    copy has landed and the count is non-zero (returns False while the copy is still in flight)."""
    dev = torch.device(device)
    t = _BAD_IDS.get(dev.index if dev.index is not None else torch.cuda.current_device())
    if t is None:
        return lambda wait=False: True
    host = torch.zeros(1, dtype=torch.int64).pin_memory()
    host.copy_(t, non_blocking=True)
    t.zero_()
    ev = torch.cuda.Event()
    ev.record()

    def resolve(wait=False):
        if wait:
            ev.synchronize()
        elif not ev.query():
            return False
        if int(host):
            n = int(host)
            host.zero_()
            raise IndexError(f"index out of range in self ({n} token ids outside the embedding table in an earlier training step)")
        return True
    return resolve


def layernorm(x, gamma, beta, out_dtype, eps=1e-12, out=None):
    lib = _abi.load()
    rows, dim = x.shape
    if out is None:
        out = torch.empty(rows, dim, dtype=torch_dtype(out_dtype), device=x.device)
    _abi.check(lib.jatts_layernorm(_dev(x).data_ptr(), code_of(x), dim, out.data_ptr(), out_dtype, dim, rows,
                                   dim, gamma.data_ptr(), beta.data_ptr(), eps, _stream()), "jatts_layernorm")
    return out


def affine_cast(x, out_dtype, scale=None, shift=None, ldy=None, x_col0=0, dim=None, out=None, out_col0=0):
    """y = x * scale + shift -> out_dtype.  ``x_col0`` / ``dim`` select a column slice of x; ``out`` / ``out_col0`` write into
    a column slice of an existing matrix (row stride out.shape[1]) instead of a fresh (rows, ldy) one."""
    lib = _abi.load()
    rows, ldx = x.shape
    dim = dim if dim is not None else ldx - x_col0
    fresh = out is None
    if fresh:
        ldy = ldy or dim
        out = torch.empty(rows, ldy, dtype=torch_dtype(out_dtype), device=x.device)
        dim_w = dim
    else:
        ldy, dim_w = out.shape[1], dim
        if out.dtype != torch_dtype(out_dtype) or out.shape[0] != rows or out_col0 + dim > ldy:
            raise ValueError("affine_cast: bad output slice")
    fn = lib.jatts_affine_cast if fresh else lib.jatts_affine_slice   # a slice writes exactly dim columns, no zero fill
    _abi.check(fn(_ptr(_dev(x), x_col0), ldx, _ptr(out, out_col0), out_dtype, ldy, rows, dim_w,
                  _ptr(scale), _ptr(shift), _stream()), "jatts_affine_cast")
    return out


def glu_dwconv_bn_swish(rb, x, channels, k_w, w_dw, bn_scale, bn_shift, dtype):
    lib = _abi.load()
    y = torch.empty(rb.total, channels, dtype=torch_dtype(dtype), device=x.device)
    rg = rb.struct()
    _abi.check(lib.jatts_glu_dwconv_bn_swish(C.byref(rg), dtype, _dev(x).data_ptr(), y.data_ptr(), channels,
                                             k_w, w_dw.data_ptr(), bn_scale.data_ptr(), bn_shift.data_ptr(),
                                             _stream()), "jatts_glu_dwconv_bn_swish")
    return y


def predictor_head(x, w, b, want_duration=False, offset=1.0):
    lib = _abi.load()
    rows, dim = x.shape
    v = torch.empty(rows, dtype=torch.float32, device=x.device)
    dur = torch.empty(rows, dtype=torch.int64, device=x.device) if want_duration else None
    _abi.check(lib.jatts_predictor_head(code_of(x), _dev(x).data_ptr(), dim, rows, dim, w.data_ptr(), float(b),
                                        v.data_ptr(), _ptr(dur), offset, _stream()), "jatts_predictor_head")
    return (v, dur) if want_duration else v


def variance_embed_add(rb, hs, p, wp, bp, e, we, be):
    lib = _abi.load()
    rg = rb.struct()
    _abi.check(lib.jatts_variance_embed_add(C.byref(rg), _dev(hs).data_ptr(), hs.shape[1], p.data_ptr(),
                                            wp.data_ptr(), bp.data_ptr(), wp.shape[-1], e.data_ptr(),
                                            we.data_ptr(), be.data_ptr(), we.shape[-1], _stream()),
               "jatts_variance_embed_add")
    return hs


def gated_tanh_sigmoid(rb, x, gseq, channels, dtype):
    lib = _abi.load()
    y = torch.empty(rb.total, channels, dtype=torch_dtype(dtype), device=x.device)
    rg = rb.struct()
    _abi.check(lib.jatts_gated_tanh_sigmoid(C.byref(rg), dtype, _dev(x).data_ptr(), _ptr(gseq), y.data_ptr(),
                                            channels, _stream()), "jatts_gated_tanh_sigmoid")
    return y


def groupnorm_mish(rb, x, channels, groups, gamma, beta, out_dtype, eps=1e-5, addvec=None, time_split=True):
    lib = _abi.load()
    y = torch.empty(rb.total, channels, dtype=torch_dtype(out_dtype), device=x.device)
    rg = rb.struct()
    ws = None
    if time_split:  # chunk statistics of the two-launch form (include/jatts_hip.h)
        ws = torch.empty(rb.n_seq * groups * ((rb.max_len + 63) // 64) * 3, dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_groupnorm_mish(C.byref(rg), _dev(x).data_ptr(), code_of(x), y.data_ptr(), out_dtype, channels,
                                        groups, gamma.data_ptr(), beta.data_ptr(), eps, _ptr(addvec), _ptr(ws), _stream()),
               "jatts_groupnorm_mish")
    return y


def snakebeta(x, alpha, inv_beta):
    lib = _abi.load()
    y = torch.empty_like(x)
    _abi.check(lib.jatts_snakebeta(code_of(x), _dev(x).data_ptr(), y.data_ptr(), x.shape[0], x.shape[1],
                                   alpha.data_ptr(), inv_beta.data_ptr(), _stream()), "jatts_snakebeta")
    return y


def l2_normalize(x, out_dtype, ldy=None, eps=1e-12):
    """F.normalize(x, dim=1) (eps 1e-12) -> out_dtype, zero-padded to ldy columns."""
    lib = _abi.load()
    rows, dim = x.shape
    ldy = ldy or dim
    y = torch.empty(rows, ldy, dtype=torch_dtype(out_dtype), device=x.device)
    _abi.check(lib.jatts_l2_normalize(_dev(x).data_ptr(), dim, y.data_ptr(), out_dtype, ldy, rows, dim, eps,
                                      _stream()), "jatts_l2_normalize")
    return y


def gaussian_sample(stats, noise, noise_scale):
    lib = _abi.load()
    rows, c2 = stats.shape
    z = torch.empty(rows, c2 // 2, dtype=torch.float32, device=stats.device)
    _abi.check(lib.jatts_gaussian_sample(_dev(stats).data_ptr(), noise.data_ptr(), z.data_ptr(), rows, c2 // 2,
                                         float(noise_scale), _stream()), "jatts_gaussian_sample")
    return z


def flip_channels(x):
    lib = _abi.load()
    y = torch.empty_like(x)
    _abi.check(lib.jatts_flip_channels(_dev(x).data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], _stream()),
               "jatts_flip_channels")
    return y


def add_seq_vector(rb, hs, vec):
    lib = _abi.load()
    rg = rb.struct()
    _abi.check(lib.jatts_add_seq_vector(C.byref(rg), _dev(hs).data_ptr(), hs.shape[1], vec.data_ptr(),
                                        _stream()), "jatts_add_seq_vector")
    return hs


def lr_durations(rb, d, alpha=1.0, zero_rule=2):
    """-> (d_eff, cum, olens int64 (n_seq,), fallback int64 (n_seq,) or None).  zero_rule 2 (default): an utterance whose
    durations sum to 0 gets all ones, as the reference's B=1 inference() does; ``fallback`` marks those utterances."""
    lib = _abi.load()
    d_eff = torch.empty_like(d)
    cum = torch.empty_like(d)
    buf = torch.empty(2 * rb.n_seq, dtype=torch.int64, device=d.device)
    rg = rb.struct()
    _abi.check(lib.jatts_lr_durations(C.byref(rg), _dev(d).data_ptr(), float(alpha), int(zero_rule),
                                      d_eff.data_ptr(), cum.data_ptr(), buf.data_ptr(), _stream()),
               "jatts_lr_durations")
    return d_eff, cum, buf[:rb.n_seq], (buf[rb.n_seq:] if zero_rule == 2 else None)


def lr_sizes_dev(rb, d, alpha=1.0, check=None):
    """The device half of lr_sizes (capturable: no host access): -> (d_eff, cum, sizes) with sizes = int64 [olens (n_seq) | all-zero
    fallback flags (n_seq) | the bad-id counter `check` (1, when given)], read by lr_sizes_host."""
    d_eff, cum, olens, fb = lr_durations(rb, d, alpha)
    return d_eff, cum, torch.cat([olens, fb] + ([check.view(-1)] if check is not None else []))


def lr_sizes_host(rb, sizes, checked):
    """The one host sync of the path: sizes (lr_sizes_dev) -> olens list.  Logs the reference's warning (length_regulator.py:87-90) for
    utterances that took the all-zero fallback; a non-zero bad-id counter raises IndexError like torch.nn.Embedding."""
    host = sizes.tolist()
    if checked and host[2 * rb.n_seq]:
        raise IndexError("token id out of range")
    olens_h, fb_h = host[:rb.n_seq], host[rb.n_seq:2 * rb.n_seq]
    if any(fb_h):
        import logging
        logging.warning("predicted durations includes all 0 sequences. fill the first element with 1.")
    return olens_h


def lr_sizes(rb, d, alpha=1.0, check=None):
    """lr_durations + the one host sync of the path: -> (d_eff, cum, olens list).  ``check``: the embed_scale bad-id counter, read in
    the same transfer."""
    d_eff, cum, sizes = lr_sizes_dev(rb, d, alpha, check)
    return d_eff, cum, lr_sizes_host(rb, sizes, check is not None)


def zero_pad_rows(rb, x, valid_len, len_mul=1):
    """x: f32 / f16 (rb.total, dim) or (rb.total,); zero the rows t >= valid_len[b] of every sequence, in place."""
    lib = _abi.load()
    dim = x.shape[1] if x.dim() == 2 else 1
    rg = rb.struct(len_mul)
    _abi.check(lib.jatts_zero_pad_rows(C.byref(rg), _dev(x).data_ptr(), code_of(x), dim, dim, valid_len.data_ptr(), _stream()),
               "jatts_zero_pad_rows")
    return x


def cfm_mix(rb, x1, z, t, sigma_min):
    lib = _abi.load()
    y, u = torch.empty_like(x1), torch.empty_like(x1)
    rg = rb.struct()
    _abi.check(lib.jatts_cfm_mix(C.byref(rg), _dev(x1).data_ptr(), z.data_ptr(), t.data_ptr(), float(sigma_min), x1.shape[1],
                                 y.data_ptr(), u.data_ptr(), _stream()), "jatts_cfm_mix")
    return y, u


def sq_err_sum(a, b, scale=1.0):
    """scale * sum((a - b)^2) -> f32 scalar tensor on the GPU (double accumulation, deterministic order)."""
    lib = _abi.load()
    out = torch.empty((), dtype=torch.float32, device=a.device)
    ws = torch.empty(256, dtype=torch.float64, device=a.device)
    _abi.check(lib.jatts_sq_err_sum(_dev(a).data_ptr(), b.data_ptr(), a.numel(), float(scale), out.data_ptr(), ws.data_ptr(),
                                    _stream()), "jatts_sq_err_sum")
    return out


def lr_gather(rb_in, cum, rb_out, x, want_index=False):
    lib = _abi.load()
    dim = x.shape[1]
    out = torch.empty(rb_out.total, dim, dtype=torch.float32, device=x.device)
    idx = torch.empty(rb_out.total, dtype=torch.int64, device=x.device) if want_index else None
    rg = rb_in.struct()
    _abi.check(lib.jatts_lr_gather(C.byref(rg), cum.data_ptr(), rb_out.cu.data_ptr(), rb_out.max_len,
                                   _dev(x).data_ptr(), dim, out.data_ptr(), _ptr(idx), _stream()),
               "jatts_lr_gather")
    return (out, idx) if want_index else out


def gaussian_upsample(rb_in, d, rb_out, hs, delta=0.1):
    lib = _abi.load()
    dim = hs.shape[1]
    out = torch.empty(rb_out.total, dim, dtype=torch.float32, device=hs.device)
    rg = rb_in.struct()
    _abi.check(lib.jatts_gaussian_upsample(C.byref(rg), _dev(d).data_ptr(), rb_out.cu.data_ptr(),
                                           rb_out.max_len, hs.data_ptr(), dim, delta, out.data_ptr(),
                                           _stream()), "jatts_gaussian_upsample")
    return out


def alignment_logp(rb_f, rb_t, feats, text, adim):
    """jatts_alignment_logp: f32 (frame rows, ld) log-probabilities, ld = round_up(max text length, 8)."""
    lib = _abi.load()
    ld = round_up(max(rb_t.max_len, 1), 8)
    out = torch.empty(rb_f.total, ld, dtype=torch.float32, device=feats.device)
    rg = rb_f.struct()
    _abi.check(lib.jatts_alignment_logp(C.byref(rg), rb_t.cu.data_ptr(), rb_t.max_len, _dev(feats).data_ptr(),
                                        _dev(text).data_ptr(), adim, out.data_ptr(), ld, _stream()), "jatts_alignment_logp")
    return out


def alignment_logp_bwd(rb_f, rb_t, feats, text, log_p, dlog_p):
    """jatts_alignment_logp_bwd: the gradient of alignment_logp in f32, two fixed-order passes.  feats (frame rows, A), text (valid-packed token rows,
    A), log_p / dlog_p (frame rows, >= max text length) f32 -> (d_feats (frame rows, A), d_text (token rows, A))."""
    lib = _abi.load()
    for v in (feats, text, log_p, dlog_p):
        if _dev(v).dtype != torch.float32 or not v.is_contiguous():
            raise ValueError("alignment_logp_bwd: contiguous float32 tensors expected")
    adim = feats.shape[1]
    lp2, dl2 = log_p.reshape(rb_f.total, -1), dlog_p.reshape(rb_f.total, -1)
    if feats.shape[0] != rb_f.total or text.shape != (rb_t.total, adim):
        raise ValueError("alignment_logp_bwd: feats / text do not match the batch geometry")
    w = torch.empty_like(lp2)
    d_feats = torch.empty_like(feats)
    d_text = torch.empty_like(text)
    rg = rb_f.struct()
    _abi.check(lib.jatts_alignment_logp_bwd(C.byref(rg), rb_t.cu.data_ptr(), rb_t.max_len, feats.data_ptr(), text.data_ptr(), adim, lp2.data_ptr(),
                                            lp2.shape[1], dl2.data_ptr(), dl2.shape[1], w.data_ptr(), d_feats.data_ptr(), d_text.data_ptr(),
                                            _stream()), "jatts_alignment_logp_bwd")
    return d_feats, d_text


def _gauss_args(what, ds, x, kv, kvo, B, Tm, To, rows):
    if _dev(x).dtype != torch.float32 or not x.is_contiguous() or x.dim() != 2 or x.shape[0] != B * rows:
        raise ValueError(f"{what}: contiguous float32 (B * {rows}, C) expected")
    if _dev(ds).dtype != torch.float32 or not ds.is_contiguous() or ds.numel() != B * Tm:
        raise ValueError(f"{what}: ds must be contiguous float32 (B, Tm)")
    for v in (kv, kvo):
        if _dev(v).dtype != torch.int32 or not v.is_contiguous() or v.numel() != B:
            raise ValueError(f"{what}: kv / kvo must be int32 (B,) device tensors")


def gaussian_upsample_fwd(ds, hs, kv, kvo, B, Tm, To, delta=0.1):
    """jatts_gaussian_upsample_fwd: masked Gaussian upsampling on the padded batch.  ds (B, Tm) f32 durations, hs (B * Tm, C) f32, kv / kvo int32 (B,)
    valid tokens / frames -> (out (B * To, C), stat (B * To, 2) = row maximum and 1 / denominator for the backward)."""
    lib = _abi.load()
    _gauss_args("gaussian_upsample_fwd", ds, hs, kv, kvo, B, Tm, To, Tm)
    Cc = hs.shape[1]
    out = torch.empty(B * To, Cc, dtype=torch.float32, device=hs.device)
    stat = torch.empty(B * To, 2, dtype=torch.float32, device=hs.device)
    _abi.check(lib.jatts_gaussian_upsample_fwd(hs.data_ptr(), ds.data_ptr(), kv.data_ptr(), kvo.data_ptr(), B, Tm, To, Cc, float(delta),
                                               out.data_ptr(), stat.data_ptr(), _stream()), "jatts_gaussian_upsample_fwd")
    return out, stat


def gaussian_upsample_bwd(ds, stat, g, kv, kvo, B, Tm, To, delta=0.1):
    """jatts_gaussian_upsample_bwd: g (B * To, C) f32 -> d_hs (B * Tm, C), exact zeros at padded tokens; the weights are recomputed from ds and stat."""
    lib = _abi.load()
    _gauss_args("gaussian_upsample_bwd", ds, g, kv, kvo, B, Tm, To, To)
    if _dev(stat).dtype != torch.float32 or not stat.is_contiguous() or stat.numel() != 2 * B * To:
        raise ValueError("gaussian_upsample_bwd: stat must be the forward's (B * To, 2) float32 tensor")
    Cc = g.shape[1]
    d_hs = torch.empty(B * Tm, Cc, dtype=torch.float32, device=g.device)
    _abi.check(lib.jatts_gaussian_upsample_bwd(g.data_ptr(), ds.data_ptr(), stat.data_ptr(), kv.data_ptr(), kvo.data_ptr(), B, Tm, To, Cc,
                                               float(delta), d_hs.data_ptr(), _stream()), "jatts_gaussian_upsample_bwd")
    return d_hs


def mas_viterbi(rb_f, rb_t, log_p):
    """jatts_mas_viterbi -> (path int64 (frame rows,), dur int64 (token rows,), score f64 (n_seq,))."""
    lib = _abi.load()
    dev = log_p.device
    path = torch.empty(rb_f.total, dtype=torch.int64, device=dev)
    dur = torch.empty(rb_t.total, dtype=torch.int64, device=dev)
    score = torch.empty(rb_f.n_seq, dtype=torch.float64, device=dev)
    rg = rb_f.struct()
    if log_p.dtype != torch.float32 or not log_p.is_contiguous():
        raise ValueError("mas_viterbi: log_p must be contiguous float32")
    _abi.check(lib.jatts_mas_viterbi(C.byref(rg), rb_t.cu.data_ptr(), _dev(log_p).data_ptr(), log_p.shape[1], rb_t.max_len,
                                     path.data_ptr(), dur.data_ptr(), score.data_ptr(), _stream()), "jatts_mas_viterbi")
    return path, dur, score


def pcm16(y, out=None):
    """jatts_pcm16: f32 waveform (n,) on the GPU -> int16 PCM (n,) on the GPU."""
    lib = _abi.load()
    y = _dev(y)
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("pcm16: contiguous float32 expected")
    if out is None:
        out = torch.empty(y.numel(), dtype=torch.int16, device=y.device)
    _abi.check(lib.jatts_pcm16(y.data_ptr(), y.numel(), out.data_ptr(), _stream()), "jatts_pcm16")
    return out


# ---- speaker-embedding front end (csrc/spkemb.hip)
def frame_signal(rb_frames, cu_samples, x, window, n_fft, hop, ldo):
    lib = _abi.load()
    out = torch.empty(rb_frames.total, ldo, dtype=torch.float32, device=x.device)
    rg = rb_frames.struct()
    _abi.check(lib.jatts_frame_signal(C.byref(rg), cu_samples.data_ptr(), _dev(x).data_ptr(), window.data_ptr(), n_fft, hop,
                                      out.data_ptr(), ldo, _stream()), "jatts_frame_signal")
    return out


def power_spectrum(x, n_bins, ldo):
    lib = _abi.load()
    out = torch.empty(x.shape[0], ldo, dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_power_spectrum(_dev(x).data_ptr(), x.shape[1], n_bins, x.shape[0], out.data_ptr(), ldo, _stream()),
               "jatts_power_spectrum")
    return out


def fbank_post(rb, p, n_mels, ldo, amin=1e-10, top_db=80.0):
    lib = _abi.load()
    out = torch.empty(rb.total, ldo, dtype=torch.float32, device=p.device)
    rg = rb.struct()
    _abi.check(lib.jatts_fbank_post(C.byref(rg), _dev(p).data_ptr(), p.shape[1], n_mels, amin, top_db, out.data_ptr(), ldo,
                                    _stream()), "jatts_fbank_post")
    return out


def seq_mean_std(rb, x, dim, logits=None, want_std=True, eps=1e-12):
    """-> (n_seq, 2*dim) f32 [mean | std] (or (n_seq, dim) means when want_std is False)."""
    lib = _abi.load()
    ld = 2 * dim if want_std else dim
    out = torch.empty(rb.n_seq, ld, dtype=torch.float32, device=x.device)
    rg = rb.struct()
    _abi.check(lib.jatts_seq_mean_std(C.byref(rg), _dev(x).data_ptr(), x.shape[1], dim, _ptr(logits),
                                      logits.shape[1] if logits is not None else 0, out.data_ptr(),
                                      _ptr(out, dim) if want_std else None, ld, eps, _stream()), "jatts_seq_mean_std")
    return out


def seq_affine_act(rb, x, dim, out_dtype, seq_vec=None, pre_act=ACT_NONE, scale=None, shift=None, post_act=ACT_NONE, ldy=None):
    lib = _abi.load()
    ldy = ldy or dim
    y = torch.empty(rb.total, ldy, dtype=torch_dtype(out_dtype), device=x.device)
    rg = rb.struct()
    _abi.check(lib.jatts_seq_affine_act(C.byref(rg), _dev(x).data_ptr(), x.shape[1], dim, _ptr(seq_vec), pre_act, _ptr(scale),
                                        _ptr(shift), post_act, y.data_ptr(), out_dtype, ldy, _stream()), "jatts_seq_affine_act")
    return y


def se_scale_add(rb, x, s, resid=None, out=None, out_col0=0):
    """y = x * sigmoid(s[b]) + resid; ``out`` / ``out_col0``: write into a column slice of a wider matrix."""
    lib = _abi.load()
    y = torch.empty_like(x) if out is None else out
    rg = rb.struct()
    _abi.check(lib.jatts_se_scale_add(C.byref(rg), _dev(x).data_ptr(), x.shape[1], s.data_ptr(), _ptr(resid), _ptr(y, out_col0),
                                      y.shape[1], _stream()), "jatts_se_scale_add")
    return y


# ---- stage-1 features (csrc/features.hip; host layer: jatts_amd/features/stft.py)
def _f32d(name, what, *ts, dims=None, numel=0):
    """Stage-1 operand check: all on the device (JattsHipError), then float32, contiguous, ``dims[i]``-dimensional where given and of at
    least ``numel`` elements (ValueError)."""
    ts = [_dev(t) for t in ts]
    if any(t.dtype != torch.float32 or not t.is_contiguous() or d not in (None, t.dim()) or t.numel() < numel
           for t, d in zip(ts, dims or [None] * len(ts))):
        raise ValueError(f"{name}: {what} expected")


def stft_mag(rb_frames, cu_samples, n_samples, x, table, n_fft, hop, ldo, want_pow=False):
    """jatts_stft_mag: packed f32 waveforms -> (mag f32 (rows, ldo), pow_sum f32 (rows,) or None).  ``n_samples``: host list of the
    utterance lengths, ``cu_samples``: their exclusive scan on the device, ``table``: features.dft_table.  Geometry the library
    refuses (n_fft, hop, ldo, short utterances) goes through to it for its message."""
    lib = _abi.load()
    _f32d("stft_mag", "contiguous float32 samples and table", x, table)
    if len(n_samples) != rb_frames.n_seq or cu_samples.numel() != rb_frames.n_seq + 1 or x.numel() < sum(n_samples):
        raise ValueError("stft_mag: sample geometry does not match the frame geometry")
    if 64 <= n_fft <= 2048 and table.numel() != n_fft * 2 * round_up(n_fft // 2 + 1, 32):
        raise ValueError("stft_mag: table is not (n_fft, 2 * round_up(n_bins, 32))")
    out = torch.empty(rb_frames.total, max(ldo, 1), dtype=torch.float32, device=x.device)
    pw = torch.empty(rb_frames.total, dtype=torch.float32, device=x.device) if want_pow else None
    ns = (C.c_int32 * len(n_samples))(*[int(v) for v in n_samples])
    rg = rb_frames.struct()
    with _scratch(x.device) if want_pow else contextlib.nullcontext() as sc:      # only the energy sum reduces: NULL without it
        _abi.check(lib.jatts_stft_mag(C.byref(rg), _dev(cu_samples).data_ptr(), ns, x.data_ptr(), table.data_ptr(), n_fft, hop,
                                      out.data_ptr(), ldo, _ptr(pw), sc, _stream()), "jatts_stft_mag")
    _count(2.0 * n_fft * table.shape[-1] * rb_frames.total)
    return out, pw


def logmel_post(mel, n_mels, ldo, eps=1e-10, log_base=10):
    """log_b(max(eps, mel)) with b = e (log_base 0), 2 or 10; columns n_mels .. ldo - 1 zero."""
    lib = _abi.load()
    out = torch.empty(mel.shape[0], ldo, dtype=torch.float32, device=mel.device)
    _abi.check(lib.jatts_logmel_post(_dev(mel).data_ptr(), mel.shape[1], n_mels, mel.shape[0], eps, log_base, out.data_ptr(), ldo,
                                     _stream()), "jatts_logmel_post")
    return out


def energy_frames(pow_sum):
    lib = _abi.load()
    e = torch.empty_like(pow_sum)
    _abi.check(lib.jatts_energy_frames(_dev(pow_sum).data_ptr(), pow_sum.numel(), e.data_ptr(), _stream()), "jatts_energy_frames")
    return e


def energy_adjust(rb_in, rb_out, e):
    """Per utterance truncate / zero-pad from rb_in's lengths to rb_out's."""
    lib = _abi.load()
    out = torch.empty(rb_out.total, dtype=torch.float32, device=e.device)
    rgi, rgo = rb_in.struct(), rb_out.struct()
    _abi.check(lib.jatts_energy_adjust(C.byref(rgi), C.byref(rgo), _dev(e).data_ptr(), out.data_ptr(), _stream()), "jatts_energy_adjust")
    return out


def token_average(rb_tokens, rb_frames, cum, e):
    """Mean of the strictly positive frame values per token span; ``cum``: per-utterance inclusive scan of the durations (device int32)."""
    lib = _abi.load()
    out = torch.empty(rb_tokens.total, dtype=torch.float32, device=e.device)
    rgt, rgf = rb_tokens.struct(), rb_frames.struct()
    _abi.check(lib.jatts_token_average(C.byref(rgt), C.byref(rgf), _dev(cum).data_ptr(), _dev(e).data_ptr(), out.data_ptr(), _stream()),
               "jatts_token_average")
    return out


# ---- stage-1 audio reading (csrc/resample.hip; host layer: jatts_amd/features/audio.py)
def resample(cu_in, cu_out, n_in, n_out, x, table, up, down, half_len, out=None):
    """jatts_resample: packed f32 waveforms -> packed f32 waveforms at up / down times the rate.  ``n_in`` / ``n_out``: host lists of the
    utterance lengths (n_out = ceil(n_in * up / down)), ``cu_in`` / ``cu_out``: their exclusive scans on the device, ``table``:
    features.resample_table (K, Nbp).  ``out``: a device buffer of at least sum(n_out) floats to write into (default: a new one)."""
    lib = _abi.load()
    _f32d("resample", "contiguous float32 samples and a (K, Nbp) float32 table", x, table, dims=(None, 2))
    n_in, n_out = [int(v) for v in n_in], [int(v) for v in n_out]
    if len(n_out) != len(n_in) or cu_in.numel() != len(n_in) + 1 or cu_out.numel() != len(n_in) + 1 or x.numel() < sum(n_in):
        raise ValueError("resample: sample geometry does not match the lengths")
    if any(o != -(-n * up // down) for n, o in zip(n_in, n_out)):
        raise ValueError("resample: n_out is not ceil(n_in * up / down)")
    nb = up * (-(-32 // up) if up < 32 else 1)
    if table.shape[1] != round_up(nb, 32):
        raise ValueError("resample: table is not (K, round_up(up * r, 32))")
    total = sum(n_out)
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=x.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < total:
        raise ValueError("resample: out must be a contiguous float32 device buffer of at least sum(n_out) elements")
    ns = (C.c_int32 * max(len(n_in), 1))(*n_in)
    _abi.check(lib.jatts_resample(len(n_in), _dev(cu_in).data_ptr(), _dev(cu_out).data_ptr(), ns, x.data_ptr(), table.data_ptr(), up, down,
                                  half_len, table.shape[0], out.data_ptr(), _stream()), "jatts_resample")
    _count(2.0 * table.shape[0] * table.shape[1] * sum(-(-o // nb) for o in n_out))
    return out


def wave_gain_peak(cu, n_seq, y, gain):
    """jatts_wave_gain_peak: y_b *= gain in place (one f32 multiply) -> f32 (n_seq, 2): max |y_b| before | after the gain."""
    lib = _abi.load()
    y = _dev(y)
    if y.dtype != torch.float32 or not y.is_contiguous() or cu.numel() != n_seq + 1:
        raise ValueError("wave_gain_peak: contiguous float32 samples and n_seq + 1 offsets expected")
    peak = torch.empty(n_seq, 2, dtype=torch.float32, device=y.device)
    _abi.check(lib.jatts_wave_gain_peak(n_seq, _dev(cu).data_ptr(), y.data_ptr(), float(gain), peak.data_ptr(), _stream()),
               "jatts_wave_gain_peak")
    return peak


# ---- Griffin-Lim (csrc/griffinlim.hip; host layer: jatts_amd/vocoder/griffin_lim.py)
def _gl_frames(name, rb):
    if rb.n_seq and min(rb.lens) < 1:
        raise ValueError(f"{name}: every utterance needs at least one frame")
    return (C.c_int32 * max(rb.n_seq, 1))(*rb.lens)


def gl_stft_project(rb, x, table, n_fft, hop, S, beta, c_prev, x_next):
    """jatts_gl_stft_project: one half-iteration, in place on ``c_prev`` and ``x_next`` (both f32 (rows, 2 * nbp)).  ``x``: f32 of at least
    rows * hop samples in the frame layout (utterance b at cu[b] * hop), ``table``: features.dft_table, ``S``: f32 (rows, lds >= n_bins)."""
    lib = _abi.load()
    _f32d("gl_stft_project", "contiguous float32 device buffers", x, table, S, c_prev, x_next, dims=(1, 2, 2, 2, 2))
    nbp = round_up(n_fft // 2 + 1, 32)
    if (x.numel() < rb.total * hop or S.shape[0] < rb.total or c_prev.shape[0] < rb.total or x_next.shape[0] < rb.total
            or c_prev.shape[1] != x_next.shape[1]):
        raise ValueError("gl_stft_project: a buffer is smaller than the frame geometry")
    if 64 <= n_fft <= 2048 and table.numel() != n_fft * 2 * nbp:
        raise ValueError("gl_stft_project: table is not (n_fft, 2 * round_up(n_bins, 32))")
    ns, rg = _gl_frames("gl_stft_project", rb), rb.struct()
    _abi.check(lib.jatts_gl_stft_project(C.byref(rg), ns, x.data_ptr(), table.data_ptr(), n_fft, hop, S.data_ptr(), S.shape[1], float(beta),
                                         c_prev.data_ptr(), x_next.data_ptr(), x_next.shape[1], _stream()), "jatts_gl_stft_project")
    _count(2.0 * n_fft * 2 * nbp * rb.total)


def gl_istft(rb, X, table, renv, n_fft, hop, y, packed=False):
    """jatts_gl_istft: ``X`` f32 (rows, 2 * nbp) -> ``y`` (f32, in place): utterance b's (T_b - 1) * hop samples at cu[b] * hop (the frame
    layout, at least rows * hop floats) or, ``packed``, back to back (at least (rows - n_seq) * hop floats).  ``table`` / ``renv``:
    vocoder.griffin_lim.istft_table / istft_envelope."""
    lib = _abi.load()
    _f32d("gl_istft", "contiguous float32 device buffers", X, table, renv, y, dims=(2, 2, 3, 1))
    if X.shape[0] < rb.total or y.numel() < (rb.total - (rb.n_seq if packed else 0)) * hop:
        raise ValueError("gl_istft: a buffer is smaller than the frame geometry")
    j = -(-n_fft // max(hop, 1))
    if hop >= 1 and tuple(renv.shape) != (j, j, table.shape[1]):
        raise ValueError("gl_istft: the envelope is not (J, J, round_up(hop, 32))")
    ns, rg = _gl_frames("gl_istft", rb), rb.struct()
    _abi.check(lib.jatts_gl_istft(C.byref(rg), ns, X.data_ptr(), X.shape[1], table.data_ptr(), table.shape[0], table.shape[1], renv.data_ptr(),
                                  n_fft, hop, int(bool(packed)), y.data_ptr(), _stream()), "jatts_gl_istft")
    _count(2.0 * table.shape[0] * table.shape[1] * max(rb.total - rb.n_seq, 0))
    return y


def gl_exp(c, n_mels, scale, mean, log_base, ldo):
    """jatts_gl_exp: base ** (c * scale + mean), f32 (rows, ldo), columns n_mels .. ldo - 1 zero.  ``log_base``: 0 (e), 2 or 10."""
    lib = _abi.load()
    _f32d("gl_exp", "contiguous float32 features (rows, >= n_mels) and statistics of n_mels", c, scale, mean, dims=(2, 1, 1))
    if c.shape[1] < n_mels or scale.numel() != n_mels or mean.numel() != n_mels:
        raise ValueError("gl_exp: contiguous float32 features (rows, >= n_mels) and statistics of n_mels expected")
    out = torch.empty(c.shape[0], ldo, dtype=torch.float32, device=c.device)
    _abi.check(lib.jatts_gl_exp(c.data_ptr(), c.shape[1], n_mels, c.shape[0], scale.data_ptr(), mean.data_ptr(), log_base, out.data_ptr(), ldo,
                                _stream()), "jatts_gl_exp")
    return out


def gl_floor(lin, n_bins, eps, ldo):
    """jatts_gl_floor: max(eps, lin), f32 (rows, ldo), columns n_bins .. ldo - 1 zero."""
    lib = _abi.load()
    _f32d("gl_floor", "a contiguous float32 (rows, >= n_bins) matrix", lin, dims=(2,))
    out = torch.empty(lin.shape[0], ldo, dtype=torch.float32, device=lin.device)
    _abi.check(lib.jatts_gl_floor(lin.data_ptr(), lin.shape[1], n_bins, lin.shape[0], float(eps), out.data_ptr(), ldo, _stream()), "jatts_gl_floor")
    return out


def gl_init(S, p0, n_fft, X):
    """jatts_gl_init: X_0 = S * P0 into ``X`` f32 (rows, 2 * nbp).  ``p0``: complex64 (rows, n_bins), contiguous."""
    lib = _abi.load()
    _f32d("gl_init", "contiguous float32 device buffers", S, X, dims=(2, 2))
    n_bins = n_fft // 2 + 1
    if _dev(p0).dtype != torch.complex64 or not p0.is_contiguous() or tuple(p0.shape) != (S.shape[0], n_bins) or X.shape[0] < S.shape[0]:
        raise ValueError("gl_init: contiguous complex64 phases (rows, n_bins) expected")
    _abi.check(lib.jatts_gl_init(S.data_ptr(), S.shape[1], p0.data_ptr(), n_fft, S.shape[0], X.data_ptr(), X.shape[1], _stream()), "jatts_gl_init")
    return X


# ---- stage-1 pitch (csrc/pitch.hip; host layer: jatts_amd/features/pitch.py)
def acf_from_mag(rb_frames, mag, table, out=None):
    """jatts_acf_from_mag: mag f32 (rows, ldm >= K) -> r f32 (rows, Lp), r[row][tau] = sum_k mag[row][k]^2 table[k][tau]; ``table``:
    features.acf_table (K, Lp).  ``out``: a device buffer of at least rows * Lp floats to write into (default: a new one)."""
    lib = _abi.load()
    _f32d("acf_from_mag", "contiguous float32 (rows, ldm) spectra and a (K, Lp) float32 table", mag, table, dims=(2, 2))
    if mag.shape[0] < rb_frames.total:
        raise ValueError("acf_from_mag: fewer spectrum rows than frames")
    k, lp = int(table.shape[0]), int(table.shape[1])
    if out is None:
        out = torch.empty(rb_frames.total, lp, dtype=torch.float32, device=mag.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < rb_frames.total * lp:
        raise ValueError("acf_from_mag: out must be a contiguous float32 device buffer of at least rows * Lp elements")
    rg = rb_frames.struct()
    _abi.check(lib.jatts_acf_from_mag(C.byref(rg), mag.data_ptr(), mag.shape[1], table.data_ptr(), k, lp, out.data_ptr(), _stream()),
               "jatts_acf_from_mag")
    _count(2.0 * k * lp * rb_frames.total)
    return out


def pitch_pick(rb_frames, r, peak, peak_stride, lo, hi, sr, f0min, sum_w2, voicing_threshold=0.45, silence_threshold=0.03,
               octave_cost=0.01):
    """jatts_pitch_pick: r f32 (rows, ldr) -> (f0 f32 (rows,), tau int32 (rows,)).  ``peak``: device f32 with max |x| of utterance b at
    element b * peak_stride (a view into hip.wave_gain_peak's result has stride 2)."""
    lib = _abi.load()
    r, peak = _dev(r), _dev(peak)
    if r.dtype != torch.float32 or peak.dtype != torch.float32 or r.dim() != 2 or not r.is_contiguous() or r.shape[0] < rb_frames.total:
        raise ValueError("pitch_pick: contiguous float32 (rows, ldr) autocorrelations and float32 peaks expected")
    if peak_stride < 1 or peak.numel() < (rb_frames.n_seq - 1) * peak_stride + 1:
        raise ValueError("pitch_pick: one peak per utterance expected")
    f0 = torch.empty(rb_frames.total, dtype=torch.float32, device=r.device)
    tau = torch.empty(rb_frames.total, dtype=torch.int32, device=r.device)
    rg = rb_frames.struct()
    _abi.check(lib.jatts_pitch_pick(C.byref(rg), r.data_ptr(), r.shape[1], peak.data_ptr(), int(peak_stride), int(lo), int(hi), float(sr),
                                    float(f0min), float(sum_w2), float(voicing_threshold), float(silence_threshold), float(octave_cost),
                                    f0.data_ptr(), tau.data_ptr(), _stream()), "jatts_pitch_pick")
    return f0, tau


def f0_continuous_log(rb_frames, f0, use_continuous=True, use_log=True):
    """jatts_f0_continuous_log: Dio._convert_to_continuous_f0 and the log of the non-zero values, per utterance -> f32 (rows,)."""
    lib = _abi.load()
    _f32d("f0_continuous_log", "a contiguous float32 track of the batch's frames", f0, dims=(1,), numel=rb_frames.total)
    out = torch.empty(rb_frames.total, dtype=torch.float32, device=f0.device)
    rg = rb_frames.struct()
    _abi.check(lib.jatts_f0_continuous_log(C.byref(rg), f0.data_ptr(), int(bool(use_continuous)), int(bool(use_log)), out.data_ptr(), _stream()),
               "jatts_f0_continuous_log")
    return out


# ---- stage-5 objective evaluation (csrc/evaluate.hip; host layer: jatts_amd/evaluate.py)
SELECT_MEAN, SELECT_POSITIVE, SELECT_MAX = 0, 1, 2


def frame_select(rb_frames, val, mode, factor=0.0, count=None):
    """jatts_frame_select over one f32 value per frame.  SELECT_MEAN: val > factor * mean (float64), SELECT_POSITIVE: val > 0 -> (count int32
    (n_seq,), idx int32 (rows,): the ascending local indices of utterance b at its frame offset).  SELECT_MAX: val > factor * max -> (int32
    (n_seq, 2): first and last selected frame, -1 when none; None).  ``count``: an int32 device buffer to write into (a slice of one the
    caller reads back once)."""
    lib = _abi.load()
    _f32d("frame_select", "a contiguous float32 value per frame", val, dims=(1,), numel=rb_frames.total)
    if mode not in (SELECT_MEAN, SELECT_POSITIVE, SELECT_MAX):
        raise ValueError(f"frame_select: unknown mode {mode}")
    n = rb_frames.n_seq * (2 if mode == SELECT_MAX else 1)
    if count is None:
        count = torch.empty(n, dtype=torch.int32, device=val.device)
    elif not count.is_cuda or count.dtype != torch.int32 or not count.is_contiguous() or count.numel() != n:
        raise ValueError(f"frame_select: count must be a contiguous int32 device buffer of {n} elements")
    idx = None if mode == SELECT_MAX else torch.empty(max(rb_frames.total, 1), dtype=torch.int32, device=val.device)
    rg = rb_frames.struct()
    with _Timed("frame_select", (mode, rb_frames.total)):
        _abi.check(lib.jatts_frame_select(C.byref(rg), val.data_ptr(), int(mode), float(factor), count.data_ptr(), _ptr(idx), _stream()),
                   "jatts_frame_select")
    return (count.view(-1, 2), None) if mode == SELECT_MAX else (count, idx)


def gather_rows(rb_src, idx, rb_out, src, dim=None):
    """jatts_gather_rows: out[rb_out.cu[b] + k] = src[rb_src.cu[b] + idx[rb_src.cu[b] + k]] -> f32 (rb_out.total, dim), or (rb_out.total,)
    for a 1-D ``src``.  ``idx``: what frame_select wrote for ``rb_src``; ``rb_out``: the geometry of its counts."""
    lib = _abi.load()
    _f32d("gather_rows", "contiguous float32 rows", src)
    idx = _dev(idx)
    flat = src.dim() == 1
    ld = 1 if flat else src.shape[1]
    dim = ld if dim is None else int(dim)
    if idx.dtype != torch.int32 or idx.numel() < rb_src.total or src.numel() < rb_src.total * ld or rb_out.n_seq != rb_src.n_seq \
            or any(o > s for o, s in zip(rb_out.lens, rb_src.lens)):
        raise ValueError("gather_rows: an int32 index per source row and at most as many output rows per utterance expected")
    out = torch.empty((rb_out.total,) if flat else (rb_out.total, dim), dtype=torch.float32, device=src.device)
    if rb_out.total == 0:
        return out
    rg = rb_out.struct()
    with _Timed("gather_rows", (rb_out.total, dim)):
        _abi.check(lib.jatts_gather_rows(C.byref(rg), rb_src.cu.data_ptr(), idx.data_ptr(), src.data_ptr(), ld, dim, out.data_ptr(), dim, _stream()),
                   "jatts_gather_rows")
    return out


def dtw_max_rows():
    return int(_abi.load().jatts_dtw_max_rows())


class PairGeometry:
    """Host geometry of a batch of (a, b) sequence pairs for the DTW kernels: pair p = rows ``a_row0[p] .. + n[p]`` of one packed matrix
    against rows ``b_row0[p] .. + m[p]`` of another.  Offsets of the per-pair cost matrices (floats), decision words (uint32) and path arrays
    (int32, capacity n + m - 1) are laid out back to back, ``gap`` elements apart (tests put poison there)."""

    def __init__(self, n, m, a_row0=None, b_row0=None, gap=0):
        self.n, self.m = [int(v) for v in n], [int(v) for v in m]
        if len(self.n) != len(self.m) or min(self.n + self.m, default=0) < 0:
            raise ValueError("PairGeometry: one non-negative (n, m) per pair")
        self.a_row0 = exclusive_scan(self.n)[:-1] if a_row0 is None else [int(v) for v in a_row0]
        self.b_row0 = exclusive_scan(self.m)[:-1] if b_row0 is None else [int(v) for v in b_row0]
        gap = int(gap)
        self.c_off, self.d_off, self.p_off = [], [], []
        c = d = p = gap
        for a, b in zip(self.n, self.m):
            self.c_off.append(c)
            self.d_off.append(d)
            self.p_off.append(p)
            c += a * b + gap
            d += a * ((b + 15) // 16) + gap
            p += max(a + b - 1, 0) + gap
        self.c_total, self.d_total, self.p_total = c, d, p
        self.n_pairs, self.max_n, self.max_m = len(self.n), max(self.n, default=0), max(self.m, default=0)

    def table(self, cols, device):
        rows = {"n": self.n, "m": self.m, "a": self.a_row0, "b": self.b_row0, "c": self.c_off, "d": self.d_off, "p": self.p_off}
        flat = [int(v) for vs in zip(*[rows[k] for k in cols]) for v in vs]
        return h2d(flat or [0], torch.int64, device)


def pairwise_dist(geo, a, b, dim=None, out=None):
    """jatts_pairwise_dist: per pair the (n, m) row-major f32 matrix of Euclidean distances between rows of ``a`` and of ``b`` (row pitch
    = their second dimension, ``dim`` <= 64 leading columns used), written at ``geo.c_off`` of one f32 buffer of ``geo.c_total``."""
    lib = _abi.load()
    _f32d("pairwise_dist", "contiguous float32 (rows, ld) matrices", a, b, dims=(2, 2))
    dim = a.shape[1] if dim is None else int(dim)
    if not 1 <= dim <= 64 or dim > a.shape[1] or dim > b.shape[1]:
        raise ValueError("pairwise_dist: 1 <= dim <= 64 and dim <= the row pitches expected")
    if any(r + n > a.shape[0] for r, n in zip(geo.a_row0, geo.n)) or any(r + m > b.shape[0] for r, m in zip(geo.b_row0, geo.m)):
        raise ValueError("pairwise_dist: a pair reaches past its matrix")
    if out is None:
        out = torch.empty(max(geo.c_total, 1), dtype=torch.float32, device=a.device)
    elif not out.is_cuda or out.dtype != torch.float32 or not out.is_contiguous() or out.numel() < geo.c_total:
        raise ValueError("pairwise_dist: out must be a contiguous float32 device buffer of geo.c_total elements")
    tab = geo.table("nmabc", a.device)
    with _Timed("pairwise_dist", (geo.n_pairs, sum(n * m for n, m in zip(geo.n, geo.m)))):
        _abi.check(lib.jatts_pairwise_dist(geo.n_pairs, tab.data_ptr(), geo.max_n, geo.max_m, a.data_ptr(), a.shape[1], b.data_ptr(), b.shape[1],
                                           dim, out.data_ptr(), _stream()), "jatts_pairwise_dist")
    return out


def dtw(geo, cost, bufs=None):
    """jatts_dtw on the cost matrices at ``geo.c_off`` of ``cost`` -> (path_len int32 (pairs,), path_i, path_j int32 (geo.p_total,): pair p's
    path at geo.p_off[p], total float64 (pairs,)).  ValueError, before any launch, for a pair of more than dtw_max_rows() rows.  ``bufs``:
    (decisions int32 (geo.d_total,), path_i, path_j, path_len, total) to write into (tests pass poisoned ones)."""
    lib = _abi.load()
    _f32d("dtw", "a contiguous float32 buffer of the pairs' cost matrices", cost, dims=(1,), numel=geo.c_total)
    cap = dtw_max_rows()
    if geo.max_n > cap:
        raise ValueError(f"dtw: a pair has {geo.max_n} rows, the kernel takes at most {cap} (rows are the first sequence's frames)")
    dev = cost.device
    if bufs is None:
        bufs = (torch.empty(max(geo.d_total, 1), dtype=torch.int32, device=dev), torch.empty(max(geo.p_total, 1), dtype=torch.int32, device=dev),
                torch.empty(max(geo.p_total, 1), dtype=torch.int32, device=dev), torch.empty(max(geo.n_pairs, 1), dtype=torch.int32, device=dev),
                torch.empty(max(geo.n_pairs, 1), dtype=torch.float64, device=dev))
    dec, pi, pj, plen, total = (_dev(t) for t in bufs)
    if dec.numel() < geo.d_total or min(pi.numel(), pj.numel()) < geo.p_total or min(plen.numel(), total.numel()) < geo.n_pairs \
            or any(t.dtype != torch.int32 or not t.is_contiguous() for t in (dec, pi, pj, plen)) or total.dtype != torch.float64:
        raise ValueError("dtw: workspace or output buffers too small or of the wrong type")
    tab = geo.table("nmcdp", dev)
    with _Timed("dtw", (geo.n_pairs, sum(n * m for n, m in zip(geo.n, geo.m)))):
        _abi.check(lib.jatts_dtw(geo.n_pairs, tab.data_ptr(), geo.max_n, cost.data_ptr(), dec.data_ptr(), pi.data_ptr(), pj.data_ptr(),
                                 plen.data_ptr(), total.data_ptr(), _stream()), "jatts_dtw")
    return plen, pi, pj, total


def dtw_path_stats(geo, path_len, path_i, path_j, a=None, b=None, dim=None, x=None, y=None, out=None):
    """jatts_dtw_path_stats -> float64 (pairs, 8): L, sum sqrt(2 sum_c (a - b)^2), sum x, sum y, sum x^2, sum y^2, sum x y, sum (x - y)^2
    along each pair's path; ``a`` / ``b``: the matrices the pairs index, ``x`` / ``y``: f32 tracks over the same rows."""
    lib = _abi.load()
    if (a is None) != (b is None) or (x is None) != (y is None) or (a is None and x is None):
        raise ValueError("dtw_path_stats: two matrices, two tracks or both expected")
    lda = ldb = d = 0
    if a is not None:
        _f32d("dtw_path_stats", "contiguous float32 (rows, ld) matrices", a, b, dims=(2, 2))
        lda, ldb = a.shape[1], b.shape[1]
        d = min(lda, ldb) if dim is None else int(dim)
    if x is not None:
        _f32d("dtw_path_stats", "contiguous float32 tracks", x, y, dims=(1, 1))
    dev = path_i.device
    if out is None:
        out = torch.empty(max(geo.n_pairs, 1), 8, dtype=torch.float64, device=dev)
    elif not out.is_cuda or out.dtype != torch.float64 or not out.is_contiguous() or out.numel() < 8 * geo.n_pairs:
        raise ValueError("dtw_path_stats: out must be a contiguous float64 device buffer of 8 values per pair")
    tab = geo.table("abp", dev)
    with _Timed("dtw_path_stats", (geo.n_pairs, d)):
        _abi.check(lib.jatts_dtw_path_stats(geo.n_pairs, tab.data_ptr(), _dev(path_i).data_ptr(), _dev(path_j).data_ptr(), _dev(path_len).data_ptr(),
                                            _ptr(a), lda, _ptr(b), ldb, d, _ptr(x), _ptr(y), out.data_ptr(), _stream()), "jatts_dtw_path_stats")
    return out


# ---- stage-1 statistics (csrc/stats.hip; host layer: jatts_amd/features/stats.py)
def col_moments_ws_doubles(rows, dim):
    """Doubles of workspace a col_moments call over ``rows`` rows needs: two sums per column and group of rows (include/jatts_hip.h)."""
    return -(-int(rows) // _abi.STATS_ROWS_PER_GROUP) * 2 * int(dim) if rows > 0 else 0


def col_moments(x, ld, dim, rows, state, ws):
    """jatts_col_moments: one partial_fit of the f32 matrix x[rows][ld] (first ``dim`` columns) into ``state`` (float64 (3, dim):
    n | mean | M2) through the caller's float64 workspace ``ws``.  Asynchronous, reads nothing back."""
    lib = _abi.load()
    _f32d("col_moments", "contiguous float32 (rows, ld)", x, numel=rows * ld)
    state, ws = _dev(state), _dev(ws)
    if state.dtype != torch.float64 or ws.dtype != torch.float64 or not state.is_contiguous() or state.numel() != 3 * dim:
        raise ValueError("col_moments: state is float64 (3, dim), the workspace float64")
    _abi.check(lib.jatts_col_moments(x.data_ptr(), ld, dim, rows, state.data_ptr(), ws.data_ptr(), ws.numel(), _stream()), "jatts_col_moments")
    return state


def col_moments_merge(state, other):
    """state <- state merged with other (both float64 (3, dim))."""
    lib = _abi.load()
    state, other = _dev(state), _dev(other)
    if state.dtype != torch.float64 or other.dtype != torch.float64 or state.shape != other.shape or state.dim() != 2 or state.shape[0] != 3:
        raise ValueError("col_moments_merge: two float64 (3, dim) states expected")
    if not state.is_contiguous() or not other.is_contiguous():
        raise ValueError("col_moments_merge: contiguous states expected")
    _abi.check(lib.jatts_col_moments_merge(state.data_ptr(), other.data_ptr(), state.shape[1], _stream()), "jatts_col_moments_merge")
    return state


def standardize(x, mean, scale, dim, ldy=None):
    """jatts_standardize: (x - mean) / scale on the first ``dim`` columns of f32 x (rows, ld), zeros up to ``ldy`` (default: x's ld)."""
    lib = _abi.load()
    _f32d("standardize", "contiguous float32 (rows, ld)", x, dims=(2,))
    mean, scale = _dev(mean), _dev(scale)
    if mean.dtype != torch.float32 or scale.dtype != torch.float32 or mean.numel() < dim or scale.numel() < dim \
            or not mean.is_contiguous() or not scale.is_contiguous():
        raise ValueError("standardize: mean / scale are contiguous float32 with at least dim elements")
    ldy = x.shape[1] if ldy is None else int(ldy)
    y = torch.empty(x.shape[0], ldy, dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_standardize(x.data_ptr(), x.shape[1], dim, x.shape[0], mean.data_ptr(), scale.data_ptr(), y.data_ptr(), ldy,
                                     _stream()), "jatts_standardize")
    return y


# ---- stage-3 batch assembly (csrc/collate.hip; host layer: jatts_amd/data.py)
class CollateSource:
    """One resident feature store for ``collate``: ``src`` (total_rows, dim) float32 or int64 on the device, contiguous, all utterances one behind
    the other; ``row_start`` / ``row_len``: the per-utterance index as numpy arrays (the host twin, what ``collate`` checks a batch against) and,
    uploaded once, as int64 / int32 device tensors (what the kernel reads)."""

    def __init__(self, src, row_start, row_len):
        import numpy as np
        self.src = _dev(src)
        self.row_start_host = np.ascontiguousarray(row_start, dtype=np.int64)
        self.row_len_host = np.ascontiguousarray(row_len, dtype=np.int32)
        if self.row_start_host.ndim != 1 or self.row_start_host.shape != self.row_len_host.shape:
            raise ValueError("CollateSource: row_start and row_len are 1-D and of one length")
        self.n_utt = int(self.row_len_host.shape[0])
        self.row_start = torch.from_numpy(self.row_start_host).to(src.device)
        self.row_len = torch.from_numpy(self.row_len_host).to(src.device)


def collate(sources, ids, t_max=None, utt=None, out=None):
    """jatts_collate: one launch that gathers the utterances ``ids`` (a host sequence of ints) out of every CollateSource of ``sources`` into
    freshly allocated padded batches -> list of (len(ids), t_max, dim) tensors, zero bits behind each utterance's rows.  ``t_max``: one value per
    source, default the longest member's rows.  ``utt``: ``ids`` as an int32 device tensor when the caller has staged it already.  ``out``: one destination per source to
    write into instead of allocating (contiguous, (len(ids), t_max, dim), the store's dtype and device; every element is overwritten).  Everything the
    kernel trusts is checked here against the host index, before any launch: ValueError."""
    import numpy as np
    lib = _abi.load()
    n_f = len(sources)
    if not 1 <= n_f <= _abi.COLLATE_MAX_FIELDS:
        raise ValueError(f"collate: {n_f} fields, 1..{_abi.COLLATE_MAX_FIELDS} (JATTS_COLLATE_MAX_FIELDS) go into one launch")
    idx = np.asarray(ids, dtype=np.int64)
    if idx.ndim != 1 or idx.size < 1:
        raise ValueError("collate: ids is a non-empty 1-D sequence of utterance numbers")
    B = int(idx.size)
    t_max = [None] * n_f if t_max is None else list(t_max)
    if len(t_max) != n_f:
        raise ValueError("collate: one t_max per source")
    if out is not None and len(out) != n_f:
        raise ValueError("collate: one out tensor per source")
    tab = (_abi.CollateField * n_f)()
    outs = []
    for i, s in enumerate(sources):
        src = s.src
        eb = {torch.float32: 4, torch.int64: 8}.get(src.dtype)
        if eb is None:
            raise ValueError(f"collate: a store of {src.dtype} (elem_bytes {src.element_size()}): float32 (4) or int64 (8)")
        if src.dim() != 2 or not src.is_contiguous():
            raise ValueError("collate: a store is a contiguous (total_rows, dim) tensor")
        dim = int(src.shape[1])
        if dim < 1:
            raise ValueError("collate: dim < 1")
        if int(idx.min()) < 0 or int(idx.max()) >= s.n_utt:
            raise ValueError(f"collate: utterance id outside 0..{s.n_utt - 1}")
        lens = s.row_len_host[idx]
        starts = s.row_start_host[idx]
        if int(lens.min()) < 0 or int(starts.min()) < 0 or int((starts + lens).max()) > src.shape[0]:
            raise ValueError("collate: the index points outside the store")
        tm = int(lens.max()) if t_max[i] is None else int(t_max[i])
        if tm < 1:
            raise ValueError("collate: t_max < 1")
        if tm < int(lens.max()):
            raise ValueError(f"collate: t_max {tm} below a member's {int(lens.max())} rows")
        if src.device != sources[0].src.device:
            raise ValueError("collate: stores on different devices")
        if out is None:
            dst = torch.empty(B, tm, dim, dtype=src.dtype, device=src.device)
        else:
            dst = out[i]
            if dst.dtype != src.dtype or dst.device != src.device or tuple(dst.shape) != (B, tm, dim) or not dst.is_contiguous():
                raise ValueError(f"collate: out[{i}] is not a contiguous {src.dtype} ({B}, {tm}, {dim}) tensor on the store's device")
        tab[i] = _abi.CollateField(src.data_ptr(), s.row_start.data_ptr(), s.row_len.data_ptr(), dst.data_ptr(), eb, dim, tm)
        outs.append(dst)
    if utt is None:
        utt = h2d([int(v) for v in idx], torch.int32, sources[0].src.device)
    elif utt.dtype != torch.int32 or utt.numel() != B or not utt.is_contiguous() or utt.device != sources[0].src.device:
        raise ValueError("collate: utt is ids as a contiguous int32 tensor on the stores' device")
    _abi.check(lib.jatts_collate(tab, n_f, utt.data_ptr(), B, _stream()), "jatts_collate")
    return outs


# ---- training side (csrc/training.hip)
def masked_loss(rb, a, b, valid_len, kind, scale, log_offset=-1.0):
    """scale * sum over valid rows of |a - b| (kind 0) or (a - b)^2 (kind 1); b -> log(b + log_offset) when log_offset >= 0."""
    lib = _abi.load()
    a2 = a if a.dim() == 2 else a.reshape(-1, 1)
    b2 = b if b.dim() == 2 else b.reshape(-1, 1)
    out = torch.empty((), dtype=torch.float32, device=a.device)
    ws = torch.empty(4 * rb.n_seq, dtype=torch.float64, device=a.device)
    rg = rb.struct()
    _abi.check(lib.jatts_masked_loss(C.byref(rg), _dev(a2).data_ptr(), a2.shape[1], b2.data_ptr(), b2.shape[1], a2.shape[1],
                                     _ptr(valid_len), kind, float(log_offset), float(scale), out.data_ptr(), ws.data_ptr(), _stream()),
               "jatts_masked_loss")
    return out


def conv1d_wgrad(rb, x, dy, c_in, n_out, k_w, dil, pad, len_mul=1, want_db=False, dtype=F32):
    """-> dw (n_out, c_in, k_w); with want_db -> (dw, db): the bias gradient comes out of the same launch (the kernel's dy tiles).
    dtype F32: the exact-f32 kernel; F32E: the emulated weight gradient (jatts_conv1d_wgrad_emul: k_w 1 / 3 / 5, halo <= 32 rows; any other geometry
    takes the exact-f32 kernel inside the entry point).  ``pad`` must lie in [0, (k_w - 1) * dil], as for conv1d; both entry points refuse anything else."""
    lib = _abi.load()
    if dtype not in (F32, F32E):
        raise ValueError("conv1d_wgrad: dtype F32 (exact) or F32E (three bf16 terms per operand, seven products)")
    dw = torch.empty(n_out, c_in, k_w, dtype=torch.float32, device=x.device)
    db = torch.empty(n_out, dtype=torch.float32, device=x.device) if want_db else None
    ws = torch.empty(rb.n_seq * (k_w * round_up(n_out, 64) * round_up(c_in, 64) + round_up(n_out, 64)), dtype=torch.float32,
                     device=x.device)                                                                                   # split-K partials
    rg = rb.struct(len_mul)
    _count(2.0 * c_in * n_out * k_w * rb.total * len_mul)
    with _scratch(x.device) as sc:
        if dtype == F32E:
            _abi.check(lib.jatts_conv1d_wgrad_emul(C.byref(rg), _dev(x).data_ptr(), x.shape[1], dy.data_ptr(), dy.shape[1], c_in, n_out, k_w, dil,
                                                    pad, dtype, dw.data_ptr(), _ptr(db), ws.data_ptr(), sc, _stream()), "jatts_conv1d_wgrad_emul")
        else:
            _abi.check(lib.jatts_conv1d_wgrad(C.byref(rg), _dev(x).data_ptr(), x.shape[1], dy.data_ptr(), dy.shape[1], c_in, n_out, k_w, dil,
                                               pad, dw.data_ptr(), _ptr(db), ws.data_ptr(), sc, _stream()), "jatts_conv1d_wgrad")
    return (dw, db) if want_db else dw


def col_sum(x, dim=None):
    lib = _abi.load()
    dim = dim or x.shape[1]
    out = _zeros((dim), x.device)
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_col_sum(_dev(x).data_ptr(), x.shape[1], x.shape[0], dim, out.data_ptr(), sc, _stream()), "jatts_col_sum")
    return out


# ------------------------------------------------------------------------------------------ training ops (train_ops.hip)
ACT_MODE = {"relu": 1, "tanh": 2, "swish": 3, "mish": 4}


def _f32c(t):
    t = _dev(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        raise ValueError("training ops take contiguous f32 device tensors")
    return t


def layernorm_bwd(x, dy, gamma, eps, need_dx=True, need_dparam=True):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    rows, dim = x.shape
    dx = torch.empty_like(x) if need_dx else None
    dg = _zeros((dim), x.device) if need_dparam else None
    db = _zeros((dim), x.device) if need_dparam else None
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_layernorm_bwd(x.data_ptr(), dim, dy.data_ptr(), dim, _f32c(gamma).data_ptr(), rows, dim, float(eps), _ptr(dx), dim,
                                            _ptr(dg), _ptr(db), sc, _stream()), "jatts_layernorm_bwd")
    return dx, dg, db


def act_fwd(x, mode):
    lib = _abi.load()
    x = _f32c(x)
    y = torch.empty_like(x)
    _abi.check(lib.jatts_act_fwd(ACT_MODE[mode], x.data_ptr(), y.data_ptr(), x.numel(), _stream()), "jatts_act_fwd")
    return y


def act_bwd(x, dy, mode):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    _abi.check(lib.jatts_act_bwd(ACT_MODE[mode], x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), _stream()), "jatts_act_bwd")
    return dx


def glu_fwd(x):
    lib = _abi.load()
    x = _f32c(x)
    rows, c2 = x.shape
    y = torch.empty(rows, c2 // 2, dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_glu_fwd(x.data_ptr(), y.data_ptr(), rows, c2 // 2, _stream()), "jatts_glu_fwd")
    return y


def glu_bwd(x, dy):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    _abi.check(lib.jatts_glu_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.shape[0], x.shape[1] // 2, _stream()), "jatts_glu_bwd")
    return dx


def dwconv(rb, x, w, bias, pad, flip=False):
    """depthwise conv on packed rows: w (C, K); flip=True is the data gradient (call with pad' = K - 1 - pad)."""
    lib = _abi.load()
    x, w = _f32c(x), _f32c(w)
    y = torch.empty_like(x)
    rg = rb.struct()
    _abi.check(lib.jatts_dwconv(C.byref(rg), x.data_ptr(), w.data_ptr(), _ptr(bias), y.data_ptr(), x.shape[1], w.shape[1], pad, int(flip),
                                _stream()), "jatts_dwconv")
    return y


def dwconv_wgrad(rb, x, dy, k_w, pad):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dw = _zeros((x.shape[1], k_w), x.device)
    rg = rb.struct()
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_dwconv_wgrad(C.byref(rg), x.data_ptr(), dy.data_ptr(), dw.data_ptr(), x.shape[1], k_w, pad, sc, _stream()),
                    "jatts_dwconv_wgrad")
    return dw


def col_stats(x, y2=None, shift=None, mul=None):
    """y2 None -> (sum (x - shift), sum (x - shift)^2); else (sum y2, sum y2 (x - shift) mul), per column."""
    lib = _abi.load()
    x = _f32c(x)
    rows, dim = x.shape
    o0 = _zeros((dim), x.device)
    o1 = _zeros((dim), x.device)
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_col_stats(x.data_ptr(), _ptr(y2), dim, rows, dim, _ptr(shift), _ptr(mul), 0 if y2 is None else 1, o0.data_ptr(),
                                        o1.data_ptr(), sc, _stream()), "jatts_col_stats")
    return o0, o1


def bn_bwd_apply(x, dy, mean, rstd, gamma, s_dy, s_dyx):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    _abi.check(lib.jatts_bn_bwd_apply(x.data_ptr(), dy.data_ptr(), x.shape[0], x.shape[1], mean.data_ptr(), rstd.data_ptr(),
                                      _f32c(gamma).data_ptr(), s_dy.data_ptr(), s_dyx.data_ptr(), dx.data_ptr(), _stream()), "jatts_bn_bwd_apply")
    return dx


def index_add_rows(src, idx, n_dst, scale=1.0, skip=-1):
    lib = _abi.load()
    src = _f32c(src)
    dst = _zeros((n_dst, src.shape[1]), src.device)
    _abi.check(lib.jatts_index_add_rows(src.data_ptr(), src.shape[1], _dev(idx).data_ptr(), src.shape[0], src.shape[1], float(scale), int(skip),
                                        n_dst, dst.data_ptr(), _stream()), "jatts_index_add_rows")
    return dst


def lr_segment_sum(rb_in, cum, rb_out, dy):
    lib = _abi.load()
    dy = _f32c(dy)
    dhs = torch.empty(rb_in.total, dy.shape[1], dtype=torch.float32, device=dy.device)
    rg = rb_in.struct()
    _abi.check(lib.jatts_lr_segment_sum(C.byref(rg), _dev(cum).data_ptr(), rb_out.cu.data_ptr(), dy.data_ptr(), dy.shape[1], dhs.data_ptr(),
                                        _stream()), "jatts_lr_segment_sum")
    return dhs


def shift_softmax_fwd(ac, bd, lens, scale, mode=1):
    """ac (B, H, T, T), bd (B, H, T, T) [mode 1, legacy rel_shift] or (B, H, T, 2T-1) [mode 2, new rel_shift] -> attention
    probabilities (bd None = plain attention)."""
    lib = _abi.load()
    ac = _f32c(ac)
    B, H, T, _ = ac.shape
    p = torch.empty_like(ac)
    _abi.check(lib.jatts_shift_softmax_fwd(ac.data_ptr(), _ptr(bd), B, H, T, _ptr(lens), float(scale), mode, p.data_ptr(), _stream()),
               "jatts_shift_softmax_fwd")
    return p


def shift_softmax_bwd(p, dp, scale, need_dbd=True, mode=1):
    lib = _abi.load()
    p, dp = _f32c(p), _f32c(dp)
    B, H, T, _ = p.shape
    ds = torch.empty_like(p)
    dbd = torch.empty(B, H, T, 2 * T - 1 if mode == 2 else T, dtype=torch.float32, device=p.device) if need_dbd else None
    _abi.check(lib.jatts_shift_softmax_bwd(p.data_ptr(), dp.data_ptr(), B, H, T, float(scale), mode, ds.data_ptr(), _ptr(dbd), _stream()),
               "jatts_shift_softmax_bwd")
    return ds, dbd


def gate_bwd(x, dy):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    _abi.check(lib.jatts_gate_bwd(x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.shape[0], x.shape[1] // 2, _stream()), "jatts_gate_bwd")
    return dx


def weight_norm_fwd(v, g):
    """-> (w, inv_norm): w = g v / ||v|| per output channel (v (n_out, ...), g (n_out, 1, ...))."""
    lib = _abi.load()
    v, g = _f32c(v), _f32c(g)
    n_out = v.shape[0]
    w = torch.empty_like(v)
    inv = torch.empty(n_out, dtype=torch.float32, device=v.device)
    _abi.check(lib.jatts_weight_norm_fwd(v.data_ptr(), g.data_ptr(), n_out, v.numel() // n_out, w.data_ptr(), inv.data_ptr(), _stream()),
               "jatts_weight_norm_fwd")
    return w, inv


def weight_norm_bwd(v, g, inv, dw):
    lib = _abi.load()
    v, g, dw = _f32c(v), _f32c(g), _f32c(dw)
    n_out = v.shape[0]
    dv, dg = torch.empty_like(v), torch.empty_like(g)
    _abi.check(lib.jatts_weight_norm_bwd(v.data_ptr(), g.data_ptr(), inv.data_ptr(), dw.data_ptr(), n_out, v.numel() // n_out,
                                         dv.data_ptr(), dg.data_ptr(), _stream()), "jatts_weight_norm_bwd")
    return dv, dg


def split_add(o, h, skip=None):
    """o (rows, 2 dim) = [res | skip part]; -> (h + res, skip + skip part)."""
    lib = _abi.load()
    o, h = _f32c(o), _f32c(h)
    rows, dim = h.shape
    if o.shape != (rows, 2 * dim):
        raise ValueError("split_add: o must be (rows, 2 dim)")
    h_out, s_out = torch.empty_like(h), torch.empty_like(h)
    _abi.check(lib.jatts_split_add(o.data_ptr(), h.data_ptr(), _ptr(_f32c(skip) if skip is not None else None), rows, dim,
                                   h_out.data_ptr(), s_out.data_ptr(), _stream()), "jatts_split_add")
    return h_out, s_out


def concat2(a, b, rows, dim, device):
    """-> (rows, 2 dim) = [a | b]; None = zeros."""
    lib = _abi.load()
    out = torch.empty(rows, 2 * dim, dtype=torch.float32, device=device)
    _abi.check(lib.jatts_concat2(_ptr(_f32c(a) if a is not None else None), _ptr(_f32c(b) if b is not None else None), rows, dim,
                                 out.data_ptr(), _stream()), "jatts_concat2")
    return out


def outer_rows(v, w, bias=None, out=None):
    lib = _abi.load()
    v, w = _f32c(v), _f32c(w)
    acc = out is not None
    if out is None:
        out = torch.empty(v.numel(), w.numel(), dtype=torch.float32, device=v.device)
    _abi.check(lib.jatts_outer_rows(v.data_ptr(), w.data_ptr(), _ptr(bias), v.numel(), w.numel(), int(acc), out.data_ptr(), _stream()),
               "jatts_outer_rows")
    return out


def col_wsum(x, v):
    lib = _abi.load()
    x, v = _f32c(x), _f32c(v)
    out = _zeros((x.shape[1]), x.device)
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_col_wsum(x.data_ptr(), x.shape[1], v.data_ptr(), x.shape[0], x.shape[1], out.data_ptr(), sc, _stream()), "jatts_col_wsum")
    return out


def row_dot(x, w, bias=None):
    lib = _abi.load()
    x, w = _f32c(x), _f32c(w)
    y = torch.empty(x.shape[0], dtype=torch.float32, device=x.device)
    _abi.check(lib.jatts_row_dot(x.data_ptr(), x.shape[1], w.data_ptr(), _ptr(bias), x.shape[0], x.shape[1], y.data_ptr(), _stream()),
               "jatts_row_dot")
    return y


def masked_loss_bwd(rb, a, b, valid_len, kind, scale, upstream=None, log_offset=-1.0):
    lib = _abi.load()
    a2 = _f32c(a if a.dim() == 2 else a.reshape(-1, 1))
    b2 = _f32c(b if b.dim() == 2 else b.reshape(-1, 1))
    da = torch.empty_like(a2)
    rg = rb.struct()
    _abi.check(lib.jatts_masked_loss_bwd(C.byref(rg), a2.data_ptr(), a2.shape[1], b2.data_ptr(), b2.shape[1], a2.shape[1], _ptr(valid_len), kind,
                                         float(log_offset), float(scale), _ptr(upstream), da.data_ptr(), a2.shape[1], _stream()),
               "jatts_masked_loss_bwd")
    return da.view_as(a)


def dropout_base_seed(seed, rank):
    """Base of one forward pass's dropout masks (site n draws from base + n): `seed` is the trainer's step / micro-batch counter, and
    data-parallel replicas draw different masks.  The eager forward bakes it into its launches, a replayed graph reads it from seed_dev."""
    return (int(seed) * 4099 + int(rank)) * 1000003


def dropout(x, p, seed, seed_dev=None):
    """seed_dev: optional int64 (1,) device tensor -- the mask seed is then *seed_dev + seed (graph mode: per-step base on the device)."""
    lib = _abi.load()
    x = _f32c(x)
    y = torch.empty_like(x)
    _abi.check(lib.jatts_dropout(x.data_ptr(), y.data_ptr(), x.numel(), float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(seed_dev), _stream()),
               "jatts_dropout")
    return y


def qkv_split(qkv, u, v, B, T, H):
    """qkv (B T, 3 A) -> (q + u, q + v, k, v) each (B, H, T, d_k) contiguous; u = v = None: (q, k, v)."""
    lib = _abi.load()
    qkv = _f32c(qkv)
    A3 = qkv.shape[1]
    dk = A3 // 3 // H
    if qkv.shape[0] != B * T or dk * H * 3 != A3 or (u is None) != (v is None):
        raise ValueError("qkv_split: shapes")
    if u is not None:
        u, v = _f32c(u), _f32c(v)
        if u.numel() != H * dk or v.numel() != H * dk:
            raise ValueError("qkv_split: bias shapes")
    outs = [torch.empty(B, H, T, dk, dtype=torch.float32, device=qkv.device) for _ in range(4 if u is not None else 3)]
    qu, qv, k, vv = outs if u is not None else (outs[0], None, outs[1], outs[2])
    _abi.check(lib.jatts_qkv_split(qkv.data_ptr(), _ptr(u), _ptr(v), B, T, H, dk, qu.data_ptr(), _ptr(qv), k.data_ptr(), vv.data_ptr(), _stream()),
               "jatts_qkv_split")
    return outs


def qkv_split_bwd(dqu, dqv, dk_, dvv):
    """-> (dqkv (B T, 3 A), du (A,), dv (A,)); dqv None (no position biases): du = dv = None."""
    lib = _abi.load()
    dqu, dk_, dvv = _f32c(dqu), _f32c(dk_), _f32c(dvv)
    B, H, T, dk = dqu.shape
    dqkv = torch.empty(B * T, 3 * H * dk, dtype=torch.float32, device=dqu.device)
    du = dv = None
    if dqv is not None:
        dqv = _f32c(dqv)
        du, dv = _zeros((H * dk), dqu.device), _zeros((H * dk), dqu.device)
    with _scratch(dqu.device) as sc:
        _abi.check(lib.jatts_qkv_split_bwd(dqu.data_ptr(), _ptr(dqv), dk_.data_ptr(), dvv.data_ptr(), B, T, H, dk, dqkv.data_ptr(), _ptr(du), _ptr(dv),
                                            sc, _stream()), "jatts_qkv_split_bwd")
    return dqkv, du, dv


def act_dropout(x, mode, p, seed, seed_dev=None, dy=None):
    """dropout(act(x)) in one pass; with dy: its backward dy * act'(x) * mask / (1 - p).  Same mask as dropout()."""
    lib = _abi.load()
    x = _f32c(x)
    out = torch.empty_like(x)
    _abi.check(lib.jatts_act_dropout(ACT_MODE[mode], x.data_ptr(), _ptr(_f32c(dy) if dy is not None else None), out.data_ptr(), x.numel(),
                                     float(p), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(seed_dev), _stream()), "jatts_act_dropout")
    return out


def dropout_add(x, resid, p, alpha, seed, seed_dev=None):
    """resid + alpha * dropout(x) (resid may be None); see jatts_dropout_add."""
    lib = _abi.load()
    x = _f32c(x)
    if resid is not None:
        resid = _f32c(resid)
        if resid.shape != x.shape:
            raise ValueError("dropout_add: shape mismatch")
    y = torch.empty_like(x)
    _abi.check(lib.jatts_dropout_add(x.data_ptr(), _ptr(resid), y.data_ptr(), x.numel(), float(p), float(alpha),
                                     int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(seed_dev), _stream()), "jatts_dropout_add")
    return y


def sumsq(x, out):
    """out (f64 scalar tensor on the device) += sum x^2"""
    lib = _abi.load()
    x = _f32c(x)
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_sumsq(x.data_ptr(), x.numel(), out.data_ptr(), sc, _stream()), "jatts_sumsq")
    return out


def gather_grads(grads, offsets, flat, accumulate=False):
    """grads: list of contiguous f32 device tensors, offsets: their element offsets in ``flat``; flat[off : off + numel] (+)= grad."""
    lib = _abi.load()
    n = len(grads)
    if n == 0:
        return
    for g in grads:
        if g.dtype != torch.float32 or not g.is_contiguous() or g.device != flat.device:
            raise ValueError("gather_grads takes contiguous f32 tensors on the flat buffer's device")
    src = (C.c_void_p * n)(*[g.data_ptr() for g in grads])
    num = (C.c_int64 * n)(*[g.numel() for g in grads])
    off = (C.c_int64 * n)(*[int(o) for o in offsets])
    _abi.check(lib.jatts_gather_grads(src, num, off, n, flat.data_ptr(), 1 if accumulate else 0, _stream()), "jatts_gather_grads")


def adam_hyper(lr, beta1, beta2, eps, weight_decay, step):
    """The 7 per-step scalars of jatts_adam_step's hyper_dev, computed in double like torch: [lr / bc1, 1 - b1, b2, 1 - b2, eps, wd, sqrt(bc2)]."""
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    return [lr / bc1, 1.0 - beta1, beta2, 1.0 - beta2, eps, weight_decay, bc2 ** 0.5]


def adam_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_sumsq=None, max_norm=0.0, hyper_dev=None):
    lib = _abi.load()
    _abi.check(lib.jatts_adam_step(_f32c(p).data_ptr(), _f32c(g).data_ptr(), _f32c(m).data_ptr(), _f32c(v).data_ptr(), p.numel(), float(lr),
                                   float(beta1), float(beta2), float(eps), float(weight_decay), int(step), _ptr(grad_sumsq), float(max_norm),
                                   _ptr(hyper_dev), _stream()), "jatts_adam_step")


def groupnorm_fwd(rb, x, groups, gamma, beta, eps):
    """-> (y, mean, rstd); mean / rstd (n_seq * groups,) for groupnorm_bwd."""
    lib = _abi.load()
    x = _f32c(x)
    y = torch.empty_like(x)
    mean = torch.empty(rb.n_seq * groups, dtype=torch.float32, device=x.device)
    rstd = torch.empty_like(mean)
    rg = rb.struct()
    _abi.check(lib.jatts_groupnorm_fwd(C.byref(rg), x.data_ptr(), x.shape[1], groups, _f32c(gamma).data_ptr(), _f32c(beta).data_ptr(), float(eps),
                                       y.data_ptr(), mean.data_ptr(), rstd.data_ptr(), _stream()), "jatts_groupnorm_fwd")
    return y, mean, rstd


def groupnorm_bwd(rb, x, dy, groups, gamma, mean, rstd, need_dx=True, need_dparam=True):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dim = x.shape[1]
    dx = torch.empty_like(x) if need_dx else None
    dg = _zeros((dim), x.device) if need_dparam else None
    db = _zeros((dim), x.device) if need_dparam else None
    rg = rb.struct()
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_groupnorm_bwd(C.byref(rg), x.data_ptr(), dy.data_ptr(), dim, groups, _f32c(gamma).data_ptr(), mean.data_ptr(),
                                            rstd.data_ptr(), _ptr(dx), _ptr(dg), _ptr(db), sc, _stream()), "jatts_groupnorm_bwd")
    return dx, dg, db


def snakebeta_fwd(x, alpha, beta):
    lib = _abi.load()
    x = _f32c(x)
    y = torch.empty_like(x)
    _abi.check(lib.jatts_snakebeta_fwd(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], _f32c(alpha).data_ptr(), _f32c(beta).data_ptr(),
                                       _stream()), "jatts_snakebeta_fwd")
    return y


def snakebeta_bwd(x, dy, alpha, beta):
    lib = _abi.load()
    x, dy = _f32c(x), _f32c(dy)
    dx = torch.empty_like(x)
    da = _zeros((x.shape[1]), x.device)
    db = _zeros((x.shape[1]), x.device)
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_snakebeta_bwd(x.data_ptr(), dy.data_ptr(), x.shape[0], x.shape[1], _f32c(alpha).data_ptr(), _f32c(beta).data_ptr(),
                                            dx.data_ptr(), da.data_ptr(), db.data_ptr(), sc, _stream()), "jatts_snakebeta_bwd")
    return dx, da, db


def ctc_forward_sum(log_p, ilens, olens, log_blank, want_grad=True, grad_scale=1.0):
    """log_p: (B, T, N) f32 (prior already added; entries beyond ilens / olens are ignored).  -> (nll (B,) = -log p / ilens, grad or None)."""
    lib = _abi.load()
    log_p = _f32c(log_p)
    B, T, ld = log_p.shape
    max_i = int(ilens.max())
    ws = torch.empty(2 * B * T * (2 * max_i + 1), dtype=torch.float32, device=log_p.device)
    nll = torch.empty(B, dtype=torch.float32, device=log_p.device)
    grad = torch.empty_like(log_p) if want_grad else None
    # (cached pinned uploads: .to(device) of a pageable CPU tensor blocks the host until everything queued so far -- the whole forward --
    # has run: 50 ms per VITS step)
    _up = lambda t: t.to(torch.int32).contiguous() if t.is_cuda else h2d([int(v) for v in t.tolist()], torch.int32, log_p.device)  # noqa: E731
    il, ol = _up(ilens), _up(olens)
    _abi.check(lib.jatts_ctc_forward_sum(log_p.data_ptr(), B, T, ld, il.data_ptr(), ol.data_ptr(), max_i, float(log_blank), ws.data_ptr(),
                                         nll.data_ptr(), _ptr(grad), float(grad_scale), _stream()), "jatts_ctc_forward_sum")
    return nll, grad


def seq_sum(rb, x):
    """-> (n_seq, dim) f32: per-sequence column sums."""
    lib = _abi.load()
    x = _f32c(x)
    out = _zeros((rb.n_seq, x.shape[1]), x.device)
    rg = rb.struct()
    with _scratch(x.device) as sc:
        _abi.check(lib.jatts_seq_sum(C.byref(rg), x.data_ptr(), x.shape[1], out.data_ptr(), sc, _stream()), "jatts_seq_sum")
    return out


def bgemm(a, b, trans_a=False, trans_b=False, alpha=1.0, out=None, dtype=F32, _tile=0):
    """jatts_bgemm: C[o][i] = alpha * op(a[o][i]) @ op(b[o][i]) on the exact-f32 matrix pipe (the training step's attention products), or with
    dtype=F32E jatts_bgemm_emul: the same product, f32 in and out, on three exact bf16 terms per operand and seven partial products (f32-equivalent).
    F32E6 has no batched GEMM and raises.  (_tile: tests only -- forces a tile of the emulated kernel, WNF | MF << 4.)
    a, b: f32 device tensors of 4 dims (O, I, rows, cols) -- any strides on the two batch dims, rows contiguous -- or 3 dims (I, rows, cols)
    = shared over O.  trans_a: a holds (k x m); trans_b: b holds (n x k).  -> (O, I, m, n) contiguous."""
    lib = _abi.load()
    a, b = _dev(a), _dev(b)

    def geom(t):
        if t.dtype != torch.float32 or t.dim() not in (3, 4) or t.stride(-1) != 1:
            raise ValueError("bgemm: f32 tensors of 3 / 4 dims with contiguous rows")
        if t.dim() == 3:
            return None, t.shape[0], 0, t.stride(0), t.stride(1)
        return t.shape[0], t.shape[1], t.stride(0), t.stride(1), t.stride(2)
    ao, ai, sao, sai, lda = geom(a)
    bo, bi, sbo, sbi, ldb = geom(b)
    O = ao if ao is not None else bo
    if O is None:
        O = 1
    if ai != bi or (ao is not None and ao != O) or (bo is not None and bo != O):
        raise ValueError("bgemm: batch dims differ")
    m, k = (a.shape[-1], a.shape[-2]) if trans_a else (a.shape[-2], a.shape[-1])
    n, kb = (b.shape[-2], b.shape[-1]) if trans_b else (b.shape[-1], b.shape[-2])
    if k != kb:
        raise ValueError("bgemm: contraction sizes differ")
    if out is None:
        out = torch.empty(O, ai, m, n, dtype=torch.float32, device=a.device)
    elif (not out.is_cuda or out.dtype != torch.float32 or out.dim() != 4 or tuple(out.shape) != (O, ai, m, n) or out.stride(3) != 1
          or out.device != a.device):
        raise ValueError(f"bgemm: out must be an f32 device tensor of shape {(O, ai, m, n)} with contiguous rows")
    _count(2.0 * O * ai * m * n * k)
    if dtype != F32:
        if dtype != F32E:
            raise ValueError("bgemm: dtype is F32 (exact f32) or F32E (seven-product bf16x3); the six-product F32E6 has no batched GEMM")
        with _Timed("bgemm_emul", (O * ai, m, n, k)):
            _abi.check(lib.jatts_bgemm_emul(a.data_ptr(), sao, sai, lda, int(trans_a), b.data_ptr(), sbo, sbi, ldb, int(trans_b), out.data_ptr(), out.stride(0),
                                            out.stride(1), out.stride(2), O, ai, m, n, k, float(alpha), 0, F32E | int(_tile) << 8, _stream()), "jatts_bgemm_emul")
        return out
    with _Timed("bgemm", (O * ai, m, n, k)):
        _abi.check(lib.jatts_bgemm(a.data_ptr(), sao, sai, lda, int(trans_a), b.data_ptr(), sbo, sbi, ldb, int(trans_b), out.data_ptr(), out.stride(0),
                                   out.stride(1), out.stride(2), O, ai, m, n, k, float(alpha), 0, _stream()), "jatts_bgemm")
    return out


def mfma_ceiling(dtype=F32E, feed=1, target_ms=60.0, device=None, seed=0):
    """jatts_mfma_probe: the matrix pipe's sustained rate on this part for `dtype` -- nothing but MFMAs (2 x 2 fragments per wave, two 4-wave workgroups per
    CU), operands re-read from LDS every K-step (feed=1) or held in registers (feed=0), on N(0, 1) operand bits in the form the kernels see them (bf16: the
    three exact terms of the emulated arithmetic in equal parts).  A calibration launch sizes the timed one to ~target_ms: long enough for the clock to
    settle at the power limit, short enough to sit in front of a bench run.  -> dict(tflops, ms, clock_ghz, iters, workgroups)."""
    lib = _abi.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(1 << 16, generator=g)
    if dtype in EMUL or dtype == 16 + F32E:
        ops = torch.cat([t.reshape(-1) for t in bf16x3_terms(v)])
    elif dtype in (F16, F32S, 16 + F16):
        ops = v.half()
    else:
        ops = v
    ops = ops.to(dev).contiguous()
    clocks = torch.zeros(2, dtype=torch.int64, device=dev)
    sink = torch.zeros(1, dtype=torch.float32, device=dev)
    wgs = 2 * torch.cuda.get_device_properties(dev).multi_processor_count

    def run(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        _abi.check(lib.jatts_mfma_probe(dtype, feed, ops.data_ptr(), ops.numel() * ops.element_size(), iters, wgs, clocks.data_ptr(), sink.data_ptr(),
                                        _stream()), "jatts_mfma_probe")
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    it = 2000
    ms = run(it)
    it = max(2000, min(int(it * target_ms / max(ms, 1e-3)) & ~1, 1 << 24))
    run(it)                              # settles the clock at the sustained level
    ms = run(it)
    c = clocks.tolist()
    return dict(tflops=lib.jatts_mfma_probe_flops(dtype, it, wgs) / ms / 1e9, ms=ms, clock_ghz=c[0] / (c[1] * 10.0) if c[1] else None, iters=it, workgroups=wgs,
                feed="lds" if feed else "registers")


_MARKER = {}


def mfma_marker(device=None):
    """One 1-workgroup, 2-K-step jatts_mfma_probe launch: a marker that tools (bench.py's B = 1 kernel-trace child) find by name in a rocprofv3 trace."""
    lib = _abi.load()
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    key = str(dev)
    if key not in _MARKER:
        _MARKER[key] = (torch.zeros(1 << 15, dtype=torch.bfloat16, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
    ops, sink = _MARKER[key]
    _abi.check(lib.jatts_mfma_probe(F32E, 0, ops.data_ptr(), ops.numel() * 2, 2, 1, None, sink.data_ptr(), _stream()), "jatts_mfma_probe")
