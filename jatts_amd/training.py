"""The trainers of the MI355X path (reference jatts/trainers/*.py `_train_step`, jatts/bin/tts_train.py) and stage 3 around them.

What is here: (1) the gradient exchange: `allreduce_gradients` / `allreduce_flat`, bucketed all-reduce over RCCL (what DistributedDataParallel does for
the reference), and its overlap with backward inside the trainers; (2) the learning-rate schedules (WarmupLR, StepLR); (3) `FastSpeech2Trainer`: the
whole `_train_step` -- forward in train() mode (models/*_train.py on the HIP forward / backward pairs of jatts_amd/autograd.py), the criterion,
backward, the gradient all-reduce, clip_grad_norm_ + Adam as HIP kernels on flat buffers, checkpoints in the reference's format, and the step captured
and replayed as a hipGraph per batch signature -- with `MatchaTTSTrainer` (tts1 and the MAS model) and `VITSTrainer` derived from it; (4) stage 3:
recipe config -> trainer (`trainer_kwargs`, refusals by name) and the training loop.  A trainer's arithmetic is one precision.TrainArithmetic record
(`precision=` / `attention=`), set around every step with autograd.arithmetic.  f32 tensors only.  No CPU fallback: CPU tensors raise.
"""
import torch
import torch.distributed as dist

from . import autograd, graphs, hip, precision as _precision
from .precision import TRAIN_ATTENTIONS, TRAIN_PRECISIONS  # noqa: F401  (read by the CLI under these names)


# ------------------------------------------------------------------------------------------ gradient exchange
def allreduce_gradients(params, group=None, bucket_bytes=64 << 20, average=True):
    """Sum (average) the .grad of ``params`` over the ranks: gradients are packed into flat buckets of ~bucket_bytes (one
    all-reduce each: 64 MiB buckets suit a ring over 7 xGMI links per GPU; FastSpeech2's 281 MB of f32 gradients = 5 collectives)
    and unpacked in place.  What DistributedDataParallel does for the reference (tts_train.py:355-363), minus the overlap with
    backward.  Works on any backend (RCCL on the GPUs, gloo in the CPU tests).  Returns the number of collectives issued."""
    world = dist.get_world_size(group)
    grads = [p.grad for p in params if p.grad is not None]
    if world == 1 or not grads:
        return 0
    n_coll, i = 0, 0
    while i < len(grads):
        j, size = i, 0
        while (j < len(grads) and (j == i or size + grads[j].numel() * grads[j].element_size() <= bucket_bytes)
               and grads[j].dtype == grads[i].dtype and grads[j].device == grads[i].device):
            size += grads[j].numel() * grads[j].element_size()
            j += 1
        flat = torch.cat([g.reshape(-1) for g in grads[i:j]])
        dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
        if average:
            flat /= world
        o = 0
        for g in grads[i:j]:
            g.copy_(flat[o:o + g.numel()].view_as(g))
            o += g.numel()
        n_coll += 1
        i = j
    return n_coll


def allreduce_flat(flat, group=None, bucket_bytes=64 << 20, average=True):
    """All-reduce a flat gradient buffer in place, bucket_bytes at a time (slices: no packing copies).  -> number of collectives."""
    world = dist.get_world_size(group)
    if world == 1:
        return 0
    per = max(1, bucket_bytes // flat.element_size())
    n = 0
    for o in range(0, flat.numel(), per):
        sl = flat[o:o + per]
        dist.all_reduce(sl, op=dist.ReduceOp.SUM, group=group)
        if average:
            sl /= world
        n += 1
    return n


# ------------------------------------------------------------------------------------------ _train_step
def warmup_lr(base_lr, step_num, warmup_steps):
    """jatts/schedulers/warmup_lr.py:55-62: lr * warmup^0.5 * min(step^-0.5, step * warmup^-1.5), step_num counts from 1."""
    return base_lr * warmup_steps ** 0.5 * min(step_num ** -0.5, step_num * warmup_steps ** -1.5)


def scheduled_lr(kind, base_lr, step_num, **params):
    """Learning rate of optimiser step ``step_num`` (1-based) under the recipes' schedulers: "warmuplr" (fastspeech2.v1 / vits.v1:
    jatts/schedulers/warmup_lr.py), "steplr" (the Matcha recipes: torch.optim.lr_scheduler.StepLR(step_size, gamma), stepped once
    per optimiser step) or None / "none" (constant)."""
    kind = (kind or "none").lower()
    if kind == "warmuplr":
        w = params.get("warmup_steps", 4000)
        return warmup_lr(base_lr, step_num, w) if w else base_lr
    if kind == "steplr":
        return base_lr * params.get("gamma", 0.1) ** ((step_num - 1) // params["step_size"])
    if kind == "none":
        return base_lr
    raise ValueError(f"unknown scheduler {kind!r} (warmuplr, steplr, none)")


class _ScalarRing:
    """A replayed graph's per-step scalars (dropout seed and Adam scalars in, gradient norm out) travel through a RING of pinned staging buffers, each
    guarded by an event recorded behind its copies: the host may run many steps ahead of the GPU, and one shared set would let step N's copy read step N + 1's."""

    def __init__(self, n):
        self.slots = [dict(seed=torch.zeros(1, dtype=torch.int64).pin_memory(), hyper=torch.zeros(7, dtype=torch.float32).pin_memory(),
                           gn=torch.zeros(1, dtype=torch.float64).pin_memory(), step=0, ev=None) for _ in range(n)]
        self.pos = 0

    def check(self, sanity):
        """Read the gradient norm of every finished slot and of the slot about to be recycled (waited for), so that no step's norm goes unread."""
        nxt = self.slots[self.pos % len(self.slots)]
        for sl in self.slots:
            if sl["ev"] is None or not sl["step"] or not (sl is nxt or sl["ev"].query()):
                continue                     # (never used, already read, or still in flight)
            if sl is nxt:
                sl["ev"].synchronize()       # (normally done long since)
            v = float(sl["gn"][0])
            sl["step"] = 0
            if not (v == v and abs(v) < sanity):
                raise FloatingPointError(f"gradient norm {v} at trainer step {sl['at']} (graph replay): a diverged run or a capture that does not replay correctly -- "
                                         "replay of this batch signature is disabled, later steps of it run eagerly; the parameters are suspect: resume from the last checkpoint")

    def take(self):
        """-> the next slot, its copies of len(slots) steps ago done; the caller fills it, replays, and records slot["ev"] behind its copies."""
        slot = self.slots[self.pos % len(self.slots)]
        self.pos += 1
        if slot["ev"] is not None:
            slot["ev"].synchronize()         # (already waited for by check() when it held a step's norm)
        return slot


class FastSpeech2Trainer:
    """`FastSpeech2Trainer._train_step` (jatts/trainers/fastspeech2.py:24-100) on one GPU of a data-parallel job:
    forward (train mode) -> MelLoss + DurationPredictorLoss + PitchLoss + EnergyLoss -> backward -> gradient all-reduce over
    the ranks (when torch.distributed is initialised) -> clip_grad_norm_(grad_norm) -> Adam -> WarmupLR.
    The optimiser state is one flat f32 pair (m, v) per parameter; clip + Adam run as HIP kernels (jatts_sumsq / jatts_adam_step),
    the clip coefficient is read on the device (no host sync in the step besides the loss values the caller asks for)."""

    def __init__(self, model, lr=0.0008, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, grad_norm=1.0, warmup_steps=4000, group=None,
                 bucket_bytes=64 << 20, overlap=True, gradient_accumulate_steps=1, scheduler="warmuplr", scheduler_params=None, capture_graph=False,
                 max_graphs=8, precision="fp32", attention=None):
        self.arith = _precision.train_arithmetic(precision, attention)      # (raises for an unknown name, before the model is touched)
        self.precision, self.attention = precision, attention               # the names, as given
        self.model, self.base_lr, self.betas, self.eps, self.wd = model, lr, betas, eps, weight_decay
        self.grad_norm, self.warmup_steps, self.group, self.bucket_bytes = grad_norm, warmup_steps, group, bucket_bytes
        self.overlap = overlap
        self.scheduler, self.scheduler_params = scheduler, dict(scheduler_params or {})      # e.g. "steplr", {"step_size": 10000, "gamma": 0.5}
        # trainers/base.py:64,135 / vits.py:113-121: `gradient_accumulate_steps` forward / backward passes (loss / G each) per optimiser
        # step; `steps` (and with it the loss schedules and WarmupLR) counts optimiser steps
        self.accumulate, self._micro = max(1, int(gradient_accumulate_steps)), 0
        model.train()   # (turns requires_grad on: the inference classes create frozen parameters)
        self.params = [p for p in model.parameters() if p.requires_grad]
        if not self.params or self.params[0].device.type != "cuda":
            raise hip._abi.JattsHipError("FastSpeech2Trainer needs the model on the GPU (no CPU fallback)")
        # one flat f32 buffer each for parameters, gradients and the two Adam moments; every parameter / .grad is a view into it:
        # zero_grad is one fill, the norm one reduction, Adam one launch, and the all-reduce runs on slices of the gradient
        # buffer with no packing copies (288 GB of HBM: the 4 x 281 MB of FastSpeech2 are nothing)
        n = sum(p.numel() for p in self.params)
        dev = self.params[0].device
        self.flat_p = torch.empty(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_m = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_v = torch.zeros(n, dtype=torch.float32, device=dev)
        o = 0
        self._grad_views, self._grad_offsets = [], []
        with torch.no_grad():
            for p in self.params:
                k = p.numel()
                self.flat_p[o:o + k].copy_(p.data.reshape(-1))
                p.data = self.flat_p[o:o + k].view(p.shape)
                p.grad = self.flat_g[o:o + k].view(p.shape)
                self._grad_views.append(p.grad)
                self._grad_offsets.append(o)
                o += k
        self.steps = 0
        self.last_lr = None
        self._bad_ids = None
        # graph mode: the whole step (forward, losses, backward, clip + Adam) of a batch SIGNATURE (shapes + length tuples: a length bucket)
        # captured once as a hipGraph and replayed, under the rules of jatts_amd/graphs.py.  See _graph_step.
        self.capture_graph = bool(capture_graph)
        self.max_graphs = max(1, int(max_graphs))     # captured graphs kept (each owns the activations of one step: GBs)
        self._policy = graphs.GraphPolicy()
        self._graphs = self._policy.states            # signature -> state dict
        self._buckets = None

    # -- gradients into the flat buffer.  With .grad pre-set to views of flat_g, autograd's AccumulateGrad runs one `view += g` kernel per
    # parameter (260 of a FastSpeech2 step's launches, 650 of a VITS step's: 1.7-4.3 ms of GPU time).  Instead .grad is cleared before
    # backward -- autograd then just keeps each produced gradient tensor -- and ONE gather (ceil(n / 64) launches) copies them into their
    # slots; .grad goes back to the flat views afterwards, so callers see what they always saw.  The overlapped all-reduce keeps the view
    # form: its bucket hooks need each gradient in place the moment it is produced.
    def _detach_grads(self):
        for p in self.params:
            p.grad = None

    def _gather_grads(self, accumulate):
        grads, offs, keep = [], [], []
        for p, o in zip(self.params, self._grad_offsets):
            g = p.grad
            if g is None:
                continue
            if g.dtype != torch.float32 or not g.is_contiguous():
                g = g.float().contiguous()
                keep.append(g)
            grads.append(g)
            offs.append(o)
        hip.gather_grads(grads, offs, self.flat_g, accumulate)
        for p, v in zip(self.params, self._grad_views):
            p.grad = v

    # -- gradient all-reduce overlapped with backward (what DistributedDataParallel's reducer does for the reference): the flat gradient
    # buffer is cut into bucket_bytes slices; a post-accumulate hook on every parameter counts its bucket down and, when the last
    # gradient of a bucket has been accumulated, issues that slice's all-reduce asynchronously (RCCL orders it after the compute
    # stream's work so far and runs it on its own stream while backward continues).  Backward produces gradients roughly in reverse
    # parameter order, so the LAST slices go first.  train_step waits for the handles, launches whatever never fired, averages.
    def _setup_overlap(self):
        per = max(1, self.bucket_bytes // 4)
        n = self.flat_g.numel()
        edges = list(range(0, n, per)) + [n]
        self._buckets = [dict(lo=edges[i], hi=edges[i + 1], total=0, left=0, work=None) for i in range(len(edges) - 1)]
        o = 0
        for p in self.params:
            touched = range(o // per, (o + p.numel() - 1) // per + 1)     # a parameter may straddle bucket edges
            for b in touched:
                self._buckets[b]["total"] += 1

            def hook(_p, touched=touched):
                for b in touched:
                    bk = self._buckets[b]
                    bk["left"] -= 1
                    if bk["left"] == 0:
                        bk["work"] = dist.all_reduce(self.flat_g[bk["lo"]:bk["hi"]], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            p.register_post_accumulate_grad_hook(hook)
            o += p.numel()

    def _arm_overlap(self, live=True):
        for bk in self._buckets:
            bk["left"], bk["work"] = (bk["total"] if live else 1 << 60), None

    def _finish_overlap(self):
        world = dist.get_world_size(self.group)
        n = 0
        for bk in self._buckets:
            if bk["work"] is None:      # a parameter of this slice got no gradient this step: reduce the slice now
                bk["work"] = dist.all_reduce(self.flat_g[bk["lo"]:bk["hi"]], op=dist.ReduceOp.SUM, group=self.group, async_op=True)
            n += 1
        for bk in self._buckets:
            bk["work"].wait()
        self.flat_g /= world
        return n

    # -- checkpoints in the reference's format (jatts/trainers/base.py:85-124): {"model", "optimizer", "scheduler", "steps", "epochs"};
    # "optimizer" is a torch.optim.Adam state_dict (state indexed by the position in model.parameters()), so a checkpoint written here
    # resumes under the reference trainer and vice versa.
    def _views(self, flat):
        out, o = [], 0
        for p in self.params:
            out.append(flat[o:o + p.numel()].view(p.shape))
            o += p.numel()
        return out

    def _sched_params(self):
        sp = dict(self.scheduler_params)
        if (self.scheduler or "").lower() == "warmuplr":
            sp.setdefault("warmup_steps", self.warmup_steps)
        return sp

    def _seed(self):
        """Dropout stream of the micro-batch about to run: a function of (optimiser step, micro-batch index) -- `_Ctx` mixes the rank
        in -- so a resumed run continues the stream instead of replaying steps 1..N, and eval_step does not consume from it."""
        return self.steps * self.accumulate + self._micro + 1

    def state_dict(self, epochs=0):
        m, v = self._views(self.flat_m), self._views(self.flat_v)
        # torch steps the scheduler AFTER the optimiser: a checkpoint holds the lr of the NEXT step (StepLR is chainable and reads
        # group["lr"] back, so storing the lr just used would lose a decay at steps % step_size == 0)
        next_lr = scheduled_lr(self.scheduler, self.base_lr, self.steps + 1, **self._sched_params())
        opt = {"state": {}, "param_groups": [dict(lr=next_lr, betas=tuple(self.betas),
                                                  eps=self.eps, weight_decay=self.wd, amsgrad=False, maximize=False, foreach=None,
                                                  capturable=False, differentiable=False, fused=None, decoupled_weight_decay=False,
                                                  initial_lr=self.base_lr, params=list(range(len(self.params))))]}
        if self.steps > 0:
            for i in range(len(self.params)):
                opt["state"][i] = {"step": torch.tensor(float(self.steps)), "exp_avg": m[i].detach().cpu().clone(),
                                   "exp_avg_sq": v[i].detach().cpu().clone()}
        sch = {"base_lrs": [self.base_lr], "last_epoch": self.steps, "_step_count": self.steps + 1, "_get_lr_called_within_step": False,
               "_last_lr": [next_lr], **self.scheduler_params}
        if (self.scheduler or "").lower() == "warmuplr":
            sch["warmup_steps"] = self.warmup_steps
        return {"model": {k: t.detach().cpu().clone() for k, t in self.model.state_dict().items()}, "optimizer": opt, "scheduler": sch,
                "steps": self.steps, "epochs": epochs}

    def save_checkpoint(self, checkpoint_path, epochs=0):
        import os
        d = os.path.dirname(checkpoint_path)
        if d and not os.path.exists(d):
            os.makedirs(d)
        torch.save(self.state_dict(epochs), checkpoint_path)

    def load_checkpoint(self, checkpoint_path, load_only_params=False):
        sd = torch.load(checkpoint_path, map_location="cpu") if isinstance(checkpoint_path, str) else checkpoint_path
        with torch.no_grad():      # copy INTO the flat views (load_state_dict copies in place: the views stay attached)
            self.model.load_state_dict(sd["model"])
        self.model._prep = None
        if load_only_params:
            return
        self.steps = int(sd["steps"])
        st = sd["optimizer"]["state"]
        if len(st) not in (0, len(self.params)):
            raise ValueError("optimizer state does not match the model's parameter list")
        with torch.no_grad():
            for i, (mv, vv) in enumerate(zip(self._views(self.flat_m), self._views(self.flat_v))):
                if i in st:
                    mv.copy_(st[i]["exp_avg"])
                    vv.copy_(st[i]["exp_avg_sq"])
        g = sd["optimizer"]["param_groups"][0]
        self.betas, self.eps, self.wd = tuple(g["betas"]), g["eps"], g["weight_decay"]
        self.base_lr = g.get("initial_lr", self.base_lr)
        if "scheduler" in sd and sd["scheduler"]:
            sch = sd["scheduler"]
            self.warmup_steps = sch.get("warmup_steps", self.warmup_steps)
            for k in ("step_size", "gamma"):           # a reference StepLR checkpoint carries its own schedule
                if k in sch:
                    self.scheduler_params[k] = sch[k]
            if "base_lrs" in sch and sch["base_lrs"]:
                self.base_lr = sch["base_lrs"][0]
        self._micro = 0
        self.last_lr = scheduled_lr(self.scheduler, self.base_lr, self.steps, **self._sched_params()) if self.steps > 0 else None

    def compute_losses(self, batch):
        """forward + criterion of trainers/fastspeech2.py:44-84 -> dict of differentiable scalars incl. "loss"."""
        from .models.fastspeech2_train import criterion, train_forward
        m = self.model
        ret = train_forward(m, batch["xs"], batch["ilens"], batch["ys"], batch["olens"], batch["durations"], batch["duration_lens"],
                            batch["pitch"], batch["pitch_lens"], batch["energys"], batch["energy_lens"], spembs=batch.get("spkembs"),
                            sids=batch.get("sids"), seed=self._seed())
        return criterion(ret, batch["durations"], batch["pitch"], batch["energys"], batch["ilens"])

    def _loss_phase(self):      # read ONCE per train_step / eval_step, before `steps` moves: what keys the graph is what compute_losses builds
        return None             # (no schedule here: _ScheduledTrainer)

    @torch.no_grad()
    def eval_step(self, batch):
        """`_eval_step` of the reference trainers (e.g. trainers/fastspeech2.py:150-215): the same forward + criterion in eval() mode
        (running-statistics BatchNorm, no dropout), no gradients, no update.  -> dict of loss tensors."""
        self._phase = self._loss_phase()
        was = self.model.training
        self.model.eval()
        try:
            with autograd.arithmetic(self.arith):
                return {k: v.detach() for k, v in self.compute_losses(batch).items()}
        finally:
            self.model.train(was)

    _phase = None              # _loss_phase() of the running call
    SCALAR_RING = 8            # pinned staging slots for the per-step scalars of a replayed graph
    GRAD_NORM_SANITY = 1e12    # a replayed step whose (pre-clip) gradient norm is not finite or beyond this is treated as a broken capture

    def _signature(self, batch):
        sig = []
        for k in sorted(batch):
            v = batch[k]
            if v is None:
                continue
            if torch.is_tensor(v) and not v.is_cuda and v.dim() == 1 and v.dtype in (torch.int64, torch.int32):
                sig.append((k, tuple(int(x) for x in v.tolist())))          # length vectors: part of the bucket
            elif torch.is_tensor(v):
                sig.append((k, tuple(v.shape), str(v.dtype)))
            else:
                sig.append((k, repr(v)))
        return tuple(sig)

    def _optimiser_tail(self, lr, step, hyper_dev=None):
        """clip_grad_norm_ + Adam on the flat buffers, on the host's (lr, step) or, inside a capture, on `hyper_dev` (hip.adam_hyper, rewritten
        before every replay).  -> the float64 sum of squares of the gradient, or None without clipping."""
        ss = None
        if self.grad_norm and self.grad_norm > 0:
            ss = torch.zeros((), dtype=torch.float64, device=self.flat_g.device)
            hip.sumsq(self.flat_g, ss)
        hip.adam_step(self.flat_p, self.flat_g, self.flat_m, self.flat_v, lr, self.betas[0], self.betas[1], self.eps, self.wd, step,
                      grad_sumsq=ss, max_norm=self.grad_norm or 0.0, hyper_dev=hyper_dev)
        return ss

    def _capture_step(self, batch, sig, st):
        """The whole step on static inputs, recorded into st["graph"] (graphs.capture): seed and Adam scalars read from device tensors."""
        dev, m = self.flat_p.device, self.model
        st["in"] = {k: (v.to(dev).clone() if torch.is_tensor(v) and (v.is_cuda or v.dim() != 1 or v.dtype not in (torch.int64, torch.int32)) else v)
                    for k, v in batch.items()}
        st["seed"], st["hyper"] = torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(7, dtype=torch.float32, device=dev)
        st["ring"] = _ScalarRing(self.SCALAR_RING)
        m._seed_dev, m._static_olens = st["seed"], [int(v) for v in batch["olens"].tolist()]
        try:
            with graphs.capture(self._policy, sig, st):
                hip.zero_pool_begin(dev)
                self.flat_g.zero_()
                self._detach_grads()
                losses = self.compute_losses(st["in"])
                losses["loss"].backward()
                self._gather_grads(False)
                ss = self._optimiser_tail(0.0, 1, st["hyper"])
                st["out"] = {k: v.detach() for k, v in losses.items()}
                if ss is not None:
                    st["out"]["grad_norm"] = ss.sqrt()
        finally:
            hip.zero_pool_end()
            m._seed_dev, m._static_olens = None, None
            for p_, v_ in zip(self.params, self._grad_views):      # (a failed capture must not leave the parameters without their .grad views)
                p_.grad = v_

    def _graph_step(self, batch, sig, st):
        """One optimiser step by replay of st["graph"] on refreshed static inputs and per-step scalars (all stream-ordered copies; no host wait).  Preconditions
        (checked where they can be): world size 1, no gradient accumulation, the length vectors (ilens / olens / *_lens) are CPU tensors, sum(durations) == olens."""
        if self._bad_ids is not None and self._bad_ids():       # out-of-range token ids of an EARLIER replay (zero rows, counted on the
            self._bad_ids = None                                # device by the embedding kernel inside the graph): IndexError, one step late
        # guard: a replay that produced garbage or a genuinely diverged run; either way the signature is marked eager-only and the
        # call raises, a few steps late, no host sync per step, BEFORE it has advanced the step counter / lr schedule or touched the static inputs
        try:
            st["ring"].check(self.GRAD_NORM_SANITY)
        except FloatingPointError:
            self._policy.fail(sig)
            raise
        for k, v in batch.items():
            if torch.is_tensor(v) and torch.is_tensor(st["in"].get(k)) and st["in"][k].is_cuda:
                st["in"][k].copy_(v, non_blocking=True)
        seed = self._seed()                  # (the step's dropout stream: the one an eager step would draw from)
        self.steps += 1
        lr = self.last_lr = scheduled_lr(self.scheduler, self.base_lr, self.steps, **self._sched_params())
        rank = dist.get_rank(self.group) if dist.is_available() and dist.is_initialized() else 0
        slot = st["ring"].take()
        slot["seed"][0] = hip.dropout_base_seed(seed, rank)
        slot["hyper"].copy_(torch.tensor(hip.adam_hyper(lr, self.betas[0], self.betas[1], self.eps, self.wd, self.steps), dtype=torch.float32))
        st["seed"].copy_(slot["seed"], non_blocking=True)
        st["hyper"].copy_(slot["hyper"], non_blocking=True)
        st["graph"].replay()
        if "grad_norm" in st["out"]:
            slot["gn"].copy_(st["out"]["grad_norm"].reshape(1), non_blocking=True)
            slot["step"], slot["at"] = 1, self.steps
        slot["ev"] = torch.cuda.Event()
        slot["ev"].record()
        self.model._prep = None
        if self._bad_ids is None:
            self._bad_ids = hip.bad_ids_async(self.flat_p.device)
        # the graph's outputs are STATIC tensors that the next replay overwrites: hand out stream-ordered copies (one concatenation per dtype),
        # so that a caller who collects loss tensors and reads them later sees each step's own values
        out, by_dtype = {}, {}
        for k, v in st["out"].items():
            by_dtype.setdefault(v.dtype, []).append(k)
        for ks in by_dtype.values():
            out.update(zip(ks, torch.stack([st["out"][k].reshape(()) for k in ks]).unbind(0)))
        return out

    def train_step(self, batch):
        """batch: dict with the collater's keys (xs, ilens, ys, olens, durations, duration_lens, pitch, pitch_lens, energys,
        energy_lens).  -> dict of the loss tensors (on the GPU; .item() them only when logging)."""
        self.model.train()
        self._phase = self._loss_phase()
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        with autograd.arithmetic(self.arith):      # around the eager, capturing and replaying forms
            if self.capture_graph and not multi and self.accumulate == 1:
                sig = self._signature(batch)
                if sig not in self._graphs and batch.get("durations") is not None:      # first sight of this bucket: verify the frame counts
                    if [int(v) for v in batch["durations"].sum(1).tolist()] != [int(v) for v in batch["olens"].tolist()]:
                        raise ValueError("graph mode needs sum(durations) == olens for every utterance")
                act, st = self._policy.decide(sig, self.max_graphs, 16 * max(1, self.max_graphs))      # (once-seen signatures: unbucketed data)
                if act == "capture":
                    self._capture_step(batch, sig, st)
                if act != "eager":                          # (no zero pool around it: the graph opens its own)
                    return self._graph_step(batch, sig, st)
            hip.zero_pool_begin(self.flat_p.device)     # the step's small zero-initialised accumulators: one fill instead of ~550
            try:
                return self._train_step(batch)
            finally:
                hip.zero_pool_end()

    def _train_step(self, batch):
        if self._bad_ids is not None and self._bad_ids():       # out-of-range token ids of an EARLIER step (zero rows, counted on the
            self._bad_ids = None                                # device): raised here, one step late, instead of a host sync per step
        if self._micro == 0:
            self.flat_g.zero_()
        last = self._micro == self.accumulate - 1
        multi = dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1
        in_place = multi and self.overlap        # gradients accumulated straight into flat_g's views (the bucket hooks need them there)
        if in_place:
            for p, v in zip(self.params, self._grad_views):      # (re-attach: a caller may have set .grad to None)
                p.grad = v
            if self._buckets is None:
                self._setup_overlap()
            self._arm_overlap(last)              # the exchange belongs to the last micro-batch's backward only
        else:
            self._detach_grads()
        losses = self.compute_losses(batch)
        (losses["loss"] / self.accumulate if self.accumulate > 1 else losses["loss"]).backward()
        if not in_place:
            self._gather_grads(self._micro > 0)
        self._micro += 1
        if not last:
            return {k: v.detach() for k, v in losses.items()}
        self._micro = 0
        if multi and self.overlap:
            self._finish_overlap()
        elif multi:
            allreduce_flat(self.flat_g, self.group, self.bucket_bytes)
        self.steps += 1
        lr = self.last_lr = scheduled_lr(self.scheduler, self.base_lr, self.steps, **self._sched_params())
        ss = self._optimiser_tail(lr, self.steps)
        self.model._prep = None
        if self._bad_ids is None:
            self._bad_ids = hip.bad_ids_async(self.flat_p.device)
        losses = {k: v.detach() for k, v in losses.items()}
        if ss is not None:
            losses["grad_norm"] = ss.sqrt()
        return losses


def loss_phase(steps, dp_train_start_steps, bin_loss_start_steps):
    """The scheduled loss terms of the step that follows `steps` optimiser steps (trainers/matchatts.py:66-103, vits.py:75-110), as the
    criteria's keyword arguments: duration loss after dp_train_start_steps, forward-sum loss before it, binarisation loss after its own start."""
    return dict(duration_loss=steps > dp_train_start_steps, forward_sum=steps < dp_train_start_steps, bin_loss=steps > bin_loss_start_steps)


class _ScheduledTrainer(FastSpeech2Trainer):
    """The loss schedule of the Matcha-TTS and VITS trainers: loss_phase() of the call, part of the graph's signature."""

    def __init__(self, model, dp_train_start_steps=0, bin_loss_start_steps=0, lambda_align=2.0, **kw):
        super().__init__(model, **kw)
        self.dp_train_start_steps, self.bin_loss_start_steps, self.lambda_align = dp_train_start_steps, bin_loss_start_steps, lambda_align
        self._phase = self._loss_phase()      # (train_step / eval_step refresh it: a direct compute_losses() sees the phase of the last call)

    def _loss_phase(self):
        return loss_phase(self.steps, self.dp_train_start_steps, self.bin_loss_start_steps)

    def _signature(self, batch):
        return super()._signature(batch) + (("schedule", *self._phase.values()),)


class MatchaTTSTrainer(_ScheduledTrainer):
    """`MatchaTTSTrainer._train_step` (jatts/trainers/matchatts.py:23-120) for the tts1 recipe (ground-truth durations; criterions
    CFMLoss + EncoderPriorLoss + DurationPredictorLoss, conf/matcha_tts.v1.prior.steplr.large.yaml): same flat-buffer optimiser,
    all-reduce and checkpoint layout as FastSpeech2Trainer; the duration loss joins once `steps > dp_train_start_steps`
    (trainers/matchatts.py:66-75).  ``cfm_t`` / ``cfm_noise`` in the batch inject the two random draws of CFM.compute_loss."""

    # graph mode: the CFM draws are device draws (graph-safe through torch's generator); the MAS model's search, its durations and the
    # Gaussian upsampling they drive all stay on the device, so its step captures too.
    def compute_losses(self, batch):
        from .models.matchatts_train import criterion, train_forward
        m, ph = self.model, self._phase
        mas = m._MAS      # tts2 MatchaTTS_MAS: alignment module + MAS; + ForwardSumLoss / binarisation loss by schedule
        ret = train_forward(m, batch["xs"], batch["ilens"], batch["ys"], batch["olens"], batch.get("durations"), batch.get("duration_lens"),
                            spembs=batch.get("spkembs"), sids=batch.get("sids"), cfm_t=batch.get("cfm_t"), cfm_noise=batch.get("cfm_noise"),
                            seed=self._seed())
        return criterion(ret, batch.get("durations"), batch["ilens"], duration_loss=ph["duration_loss"], olens=batch["olens"],
                         forward_sum=mas and ph["forward_sum"], bin_loss=mas and ph["bin_loss"], lambda_align=self.lambda_align)


class VITSTrainer(_ScheduledTrainer):
    """`VITSTrainer._train_step` (jatts/trainers/vits.py:23-140) for the mel-VITS: lambda_mel x MelLoss + KLDivergenceLoss, the
    duration loss after `dp_train_start_steps`, lambda_align x ForwardSumLoss before it, lambda_align x the binarisation loss
    after `bin_loss_start_steps`; same flat-buffer optimiser / all-reduce / checkpoint layout.  ``post_noise`` in the batch
    injects the posterior encoder's random draw.  (gradient_accumulate_steps = 1.)"""

    def __init__(self, model, dp_train_start_steps=0, bin_loss_start_steps=0, lambda_align=2.0, lambda_mel=1.0, **kw):
        super().__init__(model, dp_train_start_steps, bin_loss_start_steps, lambda_align, **kw)
        self.lambda_mel = lambda_mel

    def compute_losses(self, batch):
        from .models.vits_train import criterion, train_forward
        ret = train_forward(self.model, batch["xs"], batch["ilens"], batch["ys"], batch["olens"], batch["spkembs"],
                            post_noise=batch.get("post_noise"), seed=self._seed())
        return criterion(ret, batch["ilens"], batch["olens"], **self._phase, lambda_align=self.lambda_align, lambda_mel=self.lambda_mel)


# ------------------------------------------------------------------------------------------ stage 3: config -> trainer, the loop
# What the reference's tts_train.py reads from the recipe YAML (jatts/bin/tts_train.py:327-389) mapped onto the trainers above.  Whatever the
# trainers cannot do is refused BY NAME here, at start-up; keys that nothing reads are logged by name (unread_keys).
TRAINER_CLASSES = {"FastSpeech2Trainer": FastSpeech2Trainer, "MatchaTTSTrainer": MatchaTTSTrainer, "VITSTrainer": VITSTrainer}
NO_EFFECT_KEYS = ("pin_memory", "num_workers", "allow_cache")      # DataLoader / dataset-cache knobs: the resident data path has neither
# criterion name -> the only parameter values the trainers' criteria implement (the reference classes' defaults, jatts/losses/*.py)
CRITERION_DEFAULTS = {
    "MelLoss": {"_type": "L1Loss", "params": {}},
    "DurationPredictorLoss": {"use_masking": True, "offset": 1.0, "reduction": "mean"},
    "PitchLoss": {"use_masking": True, "reduction": "mean"},
    "EnergyLoss": {"use_masking": True, "reduction": "mean"},
    "EncoderPriorLoss": {"use_masking": True, "reduction": "mean"},
    "CFMLoss": {},
    "KLDivergenceLoss": {},
    "ForwardSumLoss": {"cache_prior": True},
}
_TRAINER_CRITERIA = {
    "FastSpeech2Trainer": ("MelLoss", "DurationPredictorLoss", "PitchLoss", "EnergyLoss"),
    "MatchaTTSTrainer": ("CFMLoss", "EncoderPriorLoss", "ForwardSumLoss", "DurationPredictorLoss"),
    "VITSTrainer": ("MelLoss", "KLDivergenceLoss", "ForwardSumLoss", "DurationPredictorLoss"),
}
_TRAINER_EXTRAS = {
    "FastSpeech2Trainer": (),
    "MatchaTTSTrainer": ("dp_train_start_steps", "bin_loss_start_steps", "lambda_align"),
    "VITSTrainer": ("dp_train_start_steps", "bin_loss_start_steps", "lambda_align", "lambda_mel"),
}


_TRAINER_FEATURES = {"FastSpeech2Trainer": ("mel", "pitch", "energy"), "MatchaTTSTrainer": ("mel",), "VITSTrainer": ("mel", "spkemb")}
# top-level keys of a recipe config that stage 3 reads (here, in tts_train and in run_training) ...
READ_KEYS = ("feat_list", "out_feat_type", "model_type", "model_params", "trainer_type", "collater_type", "criterions", "vocoder", "batch_size",
             "optimizer_type", "optimizer_params", "grad_norm", "scheduler_type", "scheduler_params", "gradient_accumulate_steps",
             "dp_train_start_steps", "bin_loss_start_steps", "lambda_align", "lambda_mel", "freeze_modules", "train_max_steps", "save_interval_steps",
             "eval_interval_steps", "log_interval_steps", "num_save_intermediate_results", "temperature", "ode_steps", "prompt_feat_list",
             "prompt_strategy") + NO_EFFECT_KEYS
# ... and those that belong to stage 1 (preprocess) or stage 4 (tts_decode) and mean nothing to training
OTHER_STAGE_KEYS = ("sampling_rate", "fft_size", "hop_size", "win_length", "window", "num_mels", "fmin", "fmax", "global_gain_scale", "log_base",
                    "pitch_extract_type", "pitch_extract_f0min", "pitch_extract_f0max", "energy_extract_type", "spkemb_checkpoint", "spkemb_params",
                    "noise_scale", "griffin_lim_iters")


def unread_keys(config, cli_keys=()):
    """Top-level config keys that stage 3 does not read and that are not another stage's: tts_train logs each by name (the FastSpeech2 and VITS
    recipes' ``scheduler: warmuplr`` is one: the reference reads ``scheduler_type``, tts_train.py:349, and so does this package)."""
    known = set(READ_KEYS) | set(OTHER_STAGE_KEYS) | set(cli_keys)
    return [k for k in config if k not in known]


def check_durations(config, has_durations):
    """Ground-truth durations come from the csv's ``durations`` column: refused by name at start-up when the trainer needs them and the csv has none
    (FastSpeech2Trainer always; MatchaTTSTrainer with the tts1 model ``MatchaTTS``; the MAS models find their own)."""
    ttype, mtype = config.get("trainer_type"), config.get("model_type")
    if not has_durations and (ttype == "FastSpeech2Trainer" or (ttype == "MatchaTTSTrainer" and mtype == "MatchaTTS")):
        raise ValueError(f"durations: {ttype} with model_type {mtype} needs the csv's durations column, and the training csv has none")


def trainer_kwargs(config):
    """Recipe config (dict) -> (trainer class, keyword arguments).  Raises ValueError naming the option for: a ``trainer_type`` that is not
    here, another ``optimizer_type`` than Adam, an ``optimizer_params`` key Adam-as-a-kernel does not take, another ``scheduler_type`` than
    warmuplr / StepLR (the names tts_train.py:37-41 reads; exponentiallr is not here), a scheduler parameter the schedule does not have, a
    criterion the trainer does not compute or a criterion parameter off its default, ``freeze_modules``, a ``feat_list`` without a feature the trainer's batch needs, and ``lambda_*`` / ``*_start_steps``
    keys given to a trainer that has no such term."""
    ttype = config.get("trainer_type", "ARTTSTrainer")
    if ttype not in TRAINER_CLASSES:
        raise ValueError(f"trainer_type: {ttype!r} is not on the HIP path ({', '.join(TRAINER_CLASSES)})")
    otype = config.get("optimizer_type", "Adam")
    if otype != "Adam":
        raise ValueError(f"optimizer_type: {otype!r} is not implemented (the optimiser step is the Adam kernel jatts_adam_step)")
    kw = {}
    op = dict(config.get("optimizer_params") or {})
    for k in op:
        if k not in ("lr", "betas", "eps", "weight_decay"):
            raise ValueError(f"optimizer_params: {k!r} is not implemented (lr, betas, eps, weight_decay)")
    if "lr" in op:
        kw["lr"] = float(op["lr"])
    if "betas" in op:
        kw["betas"] = tuple(float(b) for b in op["betas"])
    if "eps" in op:
        kw["eps"] = float(op["eps"])
    if "weight_decay" in op:
        kw["weight_decay"] = float(op["weight_decay"])
    kw["grad_norm"] = float(config.get("grad_norm", 1.0))
    stype = config.get("scheduler_type", "warmuplr")
    sp = dict(config.get("scheduler_params") or {})
    if stype == "warmuplr":
        for k in sp:
            if k != "warmup_steps":
                raise ValueError(f"scheduler_params: {k!r} is not a parameter of warmuplr (warmup_steps)")
        kw["scheduler"] = "warmuplr"
        kw["warmup_steps"] = sp.get("warmup_steps", 25000)            # WarmupLR's own default (schedulers/warmup_lr.py)
    elif stype == "StepLR":
        for k in sp:
            if k not in ("step_size", "gamma"):
                raise ValueError(f"scheduler_params: {k!r} is not implemented for StepLR (step_size, gamma)")
        if "step_size" not in sp:
            raise ValueError("scheduler_params: StepLR needs step_size")
        kw["scheduler"], kw["scheduler_params"] = "steplr", sp
    else:
        raise ValueError(f"scheduler_type: {stype!r} is not implemented (warmuplr, StepLR)")
    kw["gradient_accumulate_steps"] = int(config.get("gradient_accumulate_steps", 1))
    if config.get("freeze_modules"):
        raise ValueError("freeze_modules: freezing modules is not implemented (every parameter lives in one flat optimiser buffer)")
    for k in ("dp_train_start_steps", "bin_loss_start_steps", "lambda_align", "lambda_mel"):
        if k in config:
            if k not in _TRAINER_EXTRAS[ttype]:
                raise ValueError(f"{k}: {ttype} has no such term")
            kw[k] = config[k]
    if "feat_list" in config:
        for name in _TRAINER_FEATURES[ttype]:
            if name not in config["feat_list"]:
                raise ValueError(f"feat_list: {ttype} needs {name!r} (feat_list = {list(config['feat_list'])})")
    for name, params in (config.get("criterions") or {}).items():
        if name not in CRITERION_DEFAULTS or name not in _TRAINER_CRITERIA[ttype]:
            raise ValueError(f"criterions: {name!r} is not computed by {ttype} ({', '.join(_TRAINER_CRITERIA[ttype])})")
        for k, v in (params or {}).items():
            if k not in CRITERION_DEFAULTS[name]:
                raise ValueError(f"criterions: {name}.{k} is not a parameter of the criterion")
            if v != CRITERION_DEFAULTS[name][k]:
                raise ValueError(f"criterions: {name}.{k} = {v!r} is not implemented (only {CRITERION_DEFAULTS[name][k]!r})")
    return TRAINER_CLASSES[ttype], kw


# torch.nn.Embedding tables of the four model classes, by their full names (a suffix rule would also catch the pitch_embed / energy_embed convs)
_EMBEDDING_TABLES = ("encoder.embed.0.weight", "text_encoder.emb.weight", "sid_emb.weight", "lid_emb.weight")


@torch.no_grad()
def initialize_parameters(model, init_type="xavier_uniform"):
    """A model class of this package is built with every parameter zero (it is made to be loaded into).  Training from scratch needs what the
    reference's constructors plus ``initialize(self, init_type)`` leave behind (jatts/modules/initialize.py:70-95, called from every model's
    ``_reset_parameters``), restated on parameter names and shapes because the module tree here carries no layer types:
      * parameters of two or more dimensions: ``init_type`` (xavier_uniform / xavier_normal / kaiming_uniform / kaiming_normal), pos_bias_u / v too;
      * embedding tables (``Embedding.reset_parameters``): N(0, 1); the text embedding's padding row 0 (padding_idx = 0, fastspeech2.py:238,271) zero;
      * ``*.bias``: zero;  one-dimensional ``*.weight`` (LayerNorm / GroupNorm / BatchNorm scales): one;
      * other one-dimensional parameters (SnakeBeta's log-scale alpha / beta, matchatts/transformer.py:72-74): zero;
      * BatchNorm ``running_var``: one, ``running_mean`` and ``num_batches_tracked``: zero.
    The distributions are the reference's; the draws are not (its constructors consume torch's generator in another order)."""
    fns = {"xavier_uniform": torch.nn.init.xavier_uniform_, "xavier_normal": torch.nn.init.xavier_normal_,
           "kaiming_uniform": lambda t: torch.nn.init.kaiming_uniform_(t, nonlinearity="relu"),
           "kaiming_normal": lambda t: torch.nn.init.kaiming_normal_(t, nonlinearity="relu")}
    if init_type not in fns:
        raise ValueError(f"init_type: {init_type!r} is not implemented ({', '.join(fns)})")
    for name, p in model.named_parameters():
        if p.dim() > 1:
            if name in _EMBEDDING_TABLES and p.dim() == 2:
                p.data.normal_(0.0, 1.0)
                if name == "encoder.embed.0.weight":
                    p.data[0].zero_()
            else:
                fns[init_type](p.data)
        elif name.endswith(".weight"):
            p.data.fill_(1.0)
        else:
            p.data.zero_()
    for name, b in model.named_buffers():
        if name.endswith("running_var"):
            b.fill_(1.0)
        elif name.endswith(("running_mean", "num_batches_tracked")):
            b.zero_()
    if hasattr(model, "_prep"):
        model._prep = None
    return model


def broadcast_model(model, src=0, group=None):
    """Every parameter and buffer of ``model`` as rank ``src`` holds it, in place on all ranks: what DistributedDataParallel does at construction for
    the reference (tts_train.py:355-363).  The trainers all-reduce gradients only, so replicas that start apart stay apart: a from-scratch run draws
    its initial parameters per rank (``initialize_parameters`` on each rank's own generator), and this call is what makes them one model.  No-op
    without an initialised process group or at world size 1.  In place, so a trainer's flat views stay attached."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
        return model
    with torch.no_grad():
        for t in model.state_dict().values():
            dist.broadcast(t, src, group=group)
    if hasattr(model, "_prep"):
        model._prep = None
    return model


def replica_spread(trainer, group=None):
    """max - min over the ranks of the sum of all parameters (float64, fixed order): 0.0 while the replicas of a data-parallel job are one model
    (same start, same averaged gradients, same clip + Adam).  A collective: every rank calls it.  0.0 without a process group."""
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size(group) < 2:
        return 0.0
    s = trainer.flat_p.detach().double().sum().reshape(1)
    lo, hi = s.clone(), s.clone()
    dist.all_reduce(lo, op=dist.ReduceOp.MIN, group=group)
    dist.all_reduce(hi, op=dist.ReduceOp.MAX, group=group)
    return float(hi - lo)


def _inference_kwargs(config):
    if config.get("model_type") in ("MatchaTTS", "MatchaTTS_MAS"):          # trainers/matchatts.py: temperature / ode_steps of the config
        return {"temperature": config.get("temperature", 0.667), "n_timesteps": config.get("ode_steps", 10)}
    return {}


def griffin_lim_fallback(config, stats, device):
    """The vocoder of the intermediate waveforms for a config WITHOUT a ``vocoder:`` entry (the reference's tts_train.py:316-325): Griffin-Lim
    (``vocoder.Spectrogram2Waveform``) where the config carries every analysis key it needs, as the recipe configs do; otherwise None and the
    waveforms are skipped.  ``stats``: a {"mean", "scale"} dict or a callable that returns one (read only when it is needed)."""
    import logging
    from .vocoder.griffin_lim import CONFIG_KEYS
    missing = [k for k in CONFIG_KEYS if k not in config]
    if missing:
        logging.info("No vocoder in the config: intermediate waveforms are skipped (no Griffin-Lim fallback).")
        return None
    from .vocoder import Spectrogram2Waveform
    voc = Spectrogram2Waveform.from_config(config, stats() if callable(stats) else stats, device)
    logging.info(f"No vocoder in the config: intermediate waveforms come from Griffin-Lim, {voc.gl.n_iter} iterations.")
    return voc


@torch.no_grad()
def save_intermediate_results(trainer, batch, config, outdir, vocoder=None):
    """`_genearete_and_save_intermediate_result` (trainers/fastspeech2.py:102-223): up to ``num_save_intermediate_results`` utterances of a dev
    batch through ``model.inference`` -> predictions/<steps>steps/{durations/<idx>.txt, wav/<idx>_gen.wav (with a vocoder), outs/<idx>_out.png
    (where matplotlib imports)}."""
    import logging
    import os
    dirname = os.path.join(outdir, "predictions", f"{trainer.steps}steps")
    os.makedirs(os.path.join(dirname, "durations"), exist_ok=True)
    try:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        plt = None
        logging.info("matplotlib is not importable: figures are skipped.")
    if vocoder is None:
        logging.info("No vocoder: wav/<idx>_gen.wav is skipped (the Griffin-Lim fallback needs the config's analysis keys: griffin_lim_fallback).")
    model, kw = trainer.model, _inference_kwargs(config)
    was = model.training
    model.eval()
    try:
        ilens, olens = batch["ilens"].tolist(), batch["olens"].tolist()
        gt = batch["durations"].cpu() if batch.get("durations") is not None else None
        for idx in range(min(len(ilens), int(config.get("num_save_intermediate_results", 4)))):
            spk = None if batch.get("spkembs") is None else batch["spkembs"][idx]
            ret = model.inference(batch["xs"][idx, :ilens[idx]], spembs=spk, **kw)
            outs, d_outs = ret["feat_gen"], ret["duration"]
            if plt is not None:
                os.makedirs(os.path.join(dirname, "outs"), exist_ok=True)
                plt.figure(figsize=(12, 4), dpi=150)
                for i, a in enumerate((outs.float().cpu().numpy(), batch["ys"][idx, :olens[idx]].cpu().numpy()), 1):
                    plt.subplot(1, 2, i)
                    plt.imshow(a.T, aspect="auto", origin="lower")
                plt.tight_layout()
                plt.savefig(os.path.join(dirname, "outs", f"{idx}_out.png"))
                plt.close()
            if vocoder is not None:
                from .bin.tts_decode import write_wav_pcm16
                os.makedirs(os.path.join(dirname, "wav"), exist_ok=True)
                y, sr = vocoder.decode(outs)
                write_wav_pcm16(os.path.join(dirname, "wav", f"{idx}_gen.wav"), hip.pcm16(y.float().contiguous()).cpu().numpy(), sr)
            d_out = [str(d) for d in d_outs.reshape(-1).cpu().numpy().tolist()]
            with open(os.path.join(dirname, "durations", f"{idx}.txt"), "w") as f:
                if gt is not None:
                    for d_gt, d in zip(gt[idx, :ilens[idx]].numpy().tolist(), d_out):
                        f.write(f"{d_gt} {d}\n")
                else:
                    f.write("".join(f"{d}\n" for d in d_out))
    finally:
        model.train(was)


def run_training(trainer, train_loader, dev_loader, config, outdir, rank=0, vocoder=None, epochs=0):
    """The reference's training loop (jatts/trainers/base.py:66-224) around ``trainer.train_step`` / ``eval_step``: epochs over
    ``train_loader`` until ``trainer.steps`` reaches ``train_max_steps``; on rank 0, every ``log_interval_steps`` the mean of each loss since
    the last log line as ``(Steps: N) train/<name> = x.xxxx.``, every ``eval_interval_steps`` the mean of ``eval_step`` over ``dev_loader`` as
    ``eval/<name>`` plus the intermediate results of its first batch, every ``save_interval_steps`` ``checkpoint-<steps>steps.pkl``; and the
    same checkpoint in a ``finally`` at exit (tts_train.py:402-408).  Losses are summed as device scalars and read back only when a line is
    written: no host synchronisation in the steps between.  Every scalar also goes to ``<outdir>/scalars.jsonl`` and, where tensorboardX
    imports, to a SummaryWriter.  -> {"steps", "epochs"}."""
    import json
    import logging
    import os
    os.makedirs(outdir, exist_ok=True)
    max_steps = int(config["train_max_steps"])
    every = {k: max(1, int(config[k + "_interval_steps"])) for k in ("log", "eval", "save")}
    writer = None
    if rank == 0:
        try:
            from tensorboardX import SummaryWriter
            writer = SummaryWriter(outdir)
        except ImportError:
            logging.info("tensorboardX is not importable: scalars go to scalars.jsonl only.")

    def write_scalars(prefix, sums, n):
        vals = {f"{prefix}/{k}": v / n for k, v in sums.items()}
        host = torch.stack([v.double().reshape(()) for v in vals.values()]).cpu().tolist() if vals else []      # ONE read-back per line block
        with open(os.path.join(outdir, "scalars.jsonl"), "a") as f:
            for k, v in zip(vals, host):
                logging.info(f"(Steps: {trainer.steps}) {k} = {v:.4f}.")
                f.write(json.dumps({"steps": trainer.steps, "tag": k, "value": v}) + "\n")
                if writer is not None:
                    writer.add_scalar(k, v, trainer.steps)

    def add(sums, losses):
        for k, v in losses.items():
            v = v.detach().double()
            sums[k] = v if k not in sums else sums[k] + v

    def evaluate():
        logging.info(f"(Steps: {trainer.steps}) Start evaluation.")
        sums, n = {}, 0
        for n, batch in enumerate(dev_loader, 1):
            add(sums, trainer.eval_step(batch))
            if n == 1:
                save_intermediate_results(trainer, batch, config, outdir, vocoder)
        logging.info(f"(Steps: {trainer.steps}) Finished evaluation ({n} steps per epoch).")
        if n:
            write_scalars("eval", sums, n)

    def save():
        trainer.save_checkpoint(os.path.join(outdir, f"checkpoint-{trainer.steps}steps.pkl"), epochs=epochs)
        logging.info(f"Successfully saved checkpoint @ {trainer.steps} steps.")

    sums, n_sum = {}, 0
    finished = trainer.steps >= max_steps
    train_loader.set_epoch(epochs)
    try:
        while not finished:
            per_epoch = 0
            for per_epoch, batch in enumerate(train_loader, 1):
                add(sums, trainer.train_step(batch))
                n_sum += 1
                if trainer._micro != 0:              # gradient accumulation: the optimiser has not stepped yet (base.py:135-136)
                    continue
                finished = trainer.steps >= max_steps
                if rank == 0:
                    if trainer.steps % every["log"] == 0:
                        write_scalars("train", sums, n_sum)
                        sums, n_sum = {}, 0
                    if trainer.steps % every["eval"] == 0:
                        evaluate()
                    if trainer.steps % every["save"] == 0:
                        save()
                if finished:
                    break
            else:
                epochs += 1
                logging.info(f"(Steps: {trainer.steps}) Finished {epochs} epoch training ({per_epoch} steps per epoch).")
                train_loader.set_epoch(epochs)       # needed for the shuffle in distributed training (base.py:156-158)
                if per_epoch == 0:
                    raise ValueError("the training loader yields no batch")
        logging.info("Finished training.")
    finally:
        if rank == 0:
            save()
            if writer is not None:
                writer.close()
    return {"steps": trainer.steps, "epochs": epochs}
