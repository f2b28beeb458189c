"""DistributedDataParallel on the flat gradient arena + native reducer.

API-compatible with the way the reference uses torch DDP (``DDP(model, device_ids=[rank])``,
REF/multi-GPU-training-torch.py:245; Accelerate's ``prepare_model``, ACC/accelerator.py:1882-1896)
and with the rest of torch's constructor surface (bucket_cap_mb, broadcast_buffers,
find_unused_parameters, no_sync, state_dict with ``module.`` prefix, register_comm_hook for
gradient compression). Behaviour matched (SURVEY.md §4.3 oracles):
  1. after construction every rank holds rank 0's parameters and buffers (one broadcast of the
     flat arena, M3; buffers re-broadcast each forward when broadcast_buffers, M6);
  2. after backward ``param.grad == mean over ranks of the local gradients`` (ncclAvg);
  3. inside ``no_sync()`` gradients stay local and accumulate;
  4. parameter shapes are verified across ranks at construction (M2).
What differs by design (MI355X-first): gradients are bucket views from the start (no copies),
buckets follow backward order from iteration 0 (no 217 MiB first-iteration bucket, no rebuild),
a bucket may split a large tensor, all-reduces run on a dedicated high-priority HIP stream.
"""
from __future__ import annotations

import contextlib
import hashlib
import os
import sys
import time
import weakref

import torch
import torch.distributed as dist
import torch.nn as nn

from .._native import native
from . import runtime as rt
from .arena import BufferArena, flatten_module

_MB = 1024 * 1024
# every live DDP instance (hipGraph capture settles pending bucket rebuilds first)
_LIVE = weakref.WeakSet()


def _param_signature(params) -> str:
    h = hashlib.sha1()
    for p in params:
        h.update(f"{tuple(p.shape)}:{p.dtype};".encode())
    return h.hexdigest()


def _verify_param_shapes(params):
    if rt.get_world_size() == 1:
        return
    sig = _param_signature(params)
    sigs = [None] * rt.get_world_size()
    dist.all_gather_object(sigs, (len(params), sig))
    if any(s != sigs[0] for s in sigs):
        raise RuntimeError(
            "DDP expects the same model on every rank: parameter count/shape/dtype signatures "
            f"differ across ranks: {sigs}")


class DistributedDataParallel(nn.Module):
    def __init__(self, module: nn.Module, device_ids=None, output_device=None, dim: int = 0,
                 broadcast_buffers: bool = True, process_group=None,
                 bucket_cap_mb: float | None = None, find_unused_parameters: bool = False,
                 check_reduction: bool = False, gradient_as_bucket_view: bool = True,
                 static_graph: bool = False, first_bucket_cap_mb: float | None = None,
                 split_bucket_mb: float | None = None, grad_compression: str | None = None,
                 timing: bool = False, check_replicas_every: int | None = None,
                 force_collective: bool = False, rebuild_buckets: bool = True,
                 factor_sync: bool | None = None):
        super().__init__()
        if process_group is not None:
            raise NotImplementedError("sub-groups are not supported: DDP uses the world group")
        if not rt.is_initialized():
            raise RuntimeError("call init_process_group() before wrapping a model in DDP")
        self.module = module
        self.device_ids = device_ids
        self.output_device = output_device
        self.dim = dim
        self.broadcast_buffers = broadcast_buffers
        self.find_unused_parameters = find_unused_parameters
        self.static_graph = static_graph
        self.gradient_as_bucket_view = True  # always: gradients live in the bucket arena
        self.require_backward_grad_sync = True
        self.world_size = rt.get_world_size()
        self.rank = rt.get_rank()

        params = [p for p in module.parameters() if p.requires_grad]
        if not params:
            raise RuntimeError("DDP: module has no parameter that requires grad")
        devs = {p.device for p in params}
        if len(devs) != 1:
            raise ValueError(f"DDP expects all parameters on one device, got {devs}")
        self.device = next(iter(devs))
        if self.device.type == "cuda" and device_ids:
            want = torch.device("cuda", device_ids[0]) if isinstance(device_ids[0], int) \
                else torch.device(device_ids[0])
            if want != self.device:
                raise ValueError(f"module is on {self.device} but device_ids={device_ids}")
        self._gpu = self.device.type == "cuda"

        _verify_param_shapes(params)
        self.arena = flatten_module(module)
        self.buffers_arena = BufferArena(module)
        # M3: every rank starts from rank 0's weights -- one broadcast of the flat arena
        with torch.no_grad():
            rt.broadcast(self.arena.data, 0)
            self._sync_buffers()

        cap = (bucket_cap_mb if bucket_cap_mb is not None else 25.0) * _MB
        first = (first_bucket_cap_mb if first_bucket_cap_mb is not None else 1.0) * _MB
        split = (split_bucket_mb or 0.0) * _MB
        self._caps = (int(first), int(cap), int(split))
        self._bounds = self._plan_buckets()
        self._compression = grad_compression
        self._timing = timing
        self._fused_opt = None
        self._fused_shard = False
        self._clip_global = None   # max_norm of the in-reduction global-norm clip (fused optimizer)
        self._clip_local = None    # max_norm of the per-rank clip before aggregation
        self._clip_block = None
        # issue the collectives even at world size 1 (the single-GPU rehearsal of the multi-GPU
        # schedule; TDP_FORCE_COLLECTIVE=1 does the same from the environment)
        self._force_collective = bool(force_collective)
        # factored synchronisation of Linear weights (see _factor_candidates); None = auto: on
        # whenever it applies (GPU, fused optimizer, no clipping / compression); TDP_FACTOR_SYNC=0
        # turns the auto mode off
        env_fac = os.environ.get("TDP_FACTOR_SYNC")
        self._factor_pref = factor_sync if factor_sync is not None else \
            (None if env_fac is None else env_fac != "0")
        # replicated factored update (reducer.h FactorJob.replicate): None = auto (_replicate_pays),
        # TDP_FACTOR_REPLICATE=0/1 forces it off / on
        env_rep = os.environ.get("TDP_FACTOR_REPLICATE")
        self.factor_replicate = None if env_rep in (None, "", "auto") else env_rep != "0"
        self.factor_tuning = None  # measured replicate-vs-shard timings (tune_factor_replicate)
        self._busbw = None  # measured all-gather bus bandwidth (_probe_bandwidth)
        self._factor_rep = {}  # arena index -> replicated rows of its last factored job
        self._factor = {}          # arena index -> (out, in) of factor-eligible Linear weights
        self._factor_bucket = {}   # arena index -> its (dedicated) bucket
        self._factor_bias_bucket = {}  # arena index -> the (dedicated) bucket of its bias
        self._factor_bufs = {}     # (arena index, rows) -> (g_all, x_all) all-gather buffers
        self._factor_last_B = {}   # arena index -> per-rank batch of its last factored step
        # arena index -> factor slot rows every rank agreed on (max over ranks of the first
        # factored step's batch, one all-reduce); smaller batches are zero-padded to it
        self._factor_cap = {}
        self._factor_min_cap = 0   # factor_capacity(): a floor for the first step's agreement
        self._factor_mode = {}     # arena index -> sync mode of its last step (sync_plan)
        # arena index -> address of the weight gradient handed to autograd unwritten this step:
        # anything else in p.grad at the hook means another op contributed to the gradient
        self._factor_handed = {}
        # arena index -> per-rank batch whose x this iteration's forward staged and gathered
        self._factor_x_ready = {}
        self._factor_g_ready = {}  # arena index -> (B, g's address) whose g gather was issued early
        # factor sources gathered out of place (x, g): alive until the next iteration
        self._factor_keep = []
        self._epi_on = False
        self._epi_index = {}
        self._opt_begin_countdown = 0
        self._uses = {}            # id(param) -> forward uses in the current iteration
        # DDP Logger: every `_sample_every`-th iteration is timed with device
        # events -- forward compute, backward compute (first gradient ready -> end of backward),
        # bucket communication -- and averaged in _get_ddp_logging_data (TDP_DDP_TIMING=N or
        # timing=True for every iteration; 0 = off)
        self._sample_every = 1 if timing else int(os.environ.get("TDP_DDP_TIMING", "0") or 0)
        self._samples = []   # finished (fwd_ms, bwd_ms, comm_ms) tuples
        self._cur_ev = None  # events of the iteration being sampled
        self._pending_samples = []
        self._build_reducer()
        self._hooks = []
        self._register_hooks()
        self._rebuild_enabled = rebuild_buckets
        self._rebuild_order = None
        self._rebuilt = False
        self._callback_queued = False
        self._iter = 0
        # SURVEY.md §5.2 debug mode: every N forwards, verify that all replicas hold bit-identical
        # parameters (a checksum all-gather); TDP_CHECK_REPLICAS=N sets it from the environment
        env_every = int(os.environ.get("TDP_CHECK_REPLICAS", "0") or 0)
        self.check_replicas_every = check_replicas_every if check_replicas_every is not None \
            else env_every
        _LIVE.add(self)

    # --------------------------------------------------------------------------- reducer
    def _build_reducer(self):
        """SyncBackend (csrc/reducer.h: the bucket / shard / clip algorithm) over RcclOps on GPUs
        or over _CpuSyncOps (gloo + torch math) on CPU, plus the Reducer that tracks readiness.
        Re-applies the fused-optimizer / clipping configuration, so rebuilding (comm hook change,
        bucket rebuild) never loses optimizer state or flags."""
        nb = len(self._bounds) - 1
        C = native()
        comp = {None: 0, "none": 0, "fp32": 0, "bf16": 1}[self._compression]
        if self._gpu:
            comm = rt.comm()
            if comm is None:
                raise RuntimeError("GPU DDP needs the RCCL backend (init_process_group('nccl'))")
            self._ops = C.RcclOps(comm, self.arena.grad, self.arena.data, compression=comp)
            # profiling only: the W-rank schedule with its collectives as no-ops (the one-GPU
            # rehearsal without its one-rank copies; bench.py diagnostics rehearsal_schedule_ms)
            self._ops.skip_collectives = os.environ.get("TDP_SKIP_COLLECTIVES", "0") == "1"
        else:
            self._cpu_ops = _CpuSyncOps(self, compression=comp)
            self._ops = C.PyOps(self.rank, self.world_size, self._cpu_ops)
        # TDP_FORCE_COLLECTIVE=1 keeps the collectives (and their stream hop) at world size 1:
        # the single-GPU rehearsal of the multi-GPU schedule
        skip = os.environ.get("TDP_FORCE_COLLECTIVE", "0") != "1" and not self._force_collective
        self._backend = C.SyncBackend(self._ops, self.arena.numel, nb, timing=self._timing,
                                      skip_single_rank=skip)
        self._backend.compressed = comp != 0
        self.reducer = C.Reducer(self.arena.offsets, self.arena.numels, self._bounds,
                                 self._backend)
        if self._fused_opt is not None:
            self._configure_fused()
        if self._clip_local is not None:
            self._configure_local_clip()

    def _plan_buckets(self):
        first, cap, split = self._caps
        b = list(native().Reducer.compute_bucket_bounds(
            self.arena.offsets, self.arena.numels, self.arena.numel,
            self.arena.data.element_size(), first, cap, split))
        factor = getattr(self, "_factor", None) or {}
        if factor:
            # a factored weight is a bucket of its own (its launch replaces the bucket's
            # collectives, reducer.cpp SyncBackend::launch)
            cuts = set(b)
            for i, (_, _, bi) in factor.items():
                for j in (i,) if bi is None else (i, bi):
                    off, n = self.arena.offsets[j], self.arena.numels[j]
                    cuts.update((off, off + n))
            b = sorted(cuts)
            self._factor_bucket = {i: b.index(self.arena.offsets[i]) for i in factor}
            self._factor_bias_bucket = {i: b.index(self.arena.offsets[bi])
                                        for i, (_, _, bi) in factor.items() if bi is not None}
        return b

    def _register_hooks(self):
        for h in self._hooks:
            h.remove()
        self._hooks = [p.register_post_accumulate_grad_hook(self._make_hook(i))
                       for i, p in enumerate(self.arena.params)]

    def _plan_rebuild(self):
        """After iteration 0 (torch: ``_rebuild_buckets``): if some bucket was complete while a
        lower-indexed one was not -- gradients arrive in a different order than the arena layout
        -- re-lay the arena out in the observed ready order at the next forward. Rank 0's
        decision is broadcast, so every rank rebuilds identically."""
        P = len(self.arena.params)
        order = [int(i) for i in self.reducer.ready_order()]
        seen = set(order)
        order += [i for i in range(P) if i not in seen]  # never-ready (unused) params last
        want = int(self.reducer.head_of_line_waits) > 0 and order != list(range(P))
        msg = torch.tensor([1 if want else 0] + order, dtype=torch.int64, device=self.device)
        rt.broadcast(msg, 0)
        if int(msg[0]):
            self._rebuild_order = [int(v) for v in msg[1:].tolist()]

    def _rebuild_buckets(self):
        order, self._rebuild_order = self._rebuild_order, None
        # under the sharded update, optimizer state is current only in this rank's shards of the
        # OLD buckets; the new layout hands shards to other owners, so every rank first gathers
        # the complete state (one all-gather per bucket, once per job)
        self.consolidate_optimizer_state()
        # per-parameter factored-sync state follows its parameter to the new arena index (the
        # agreed slot sizes must not be re-agreed: that may happen inside a capture)
        new_of = {old: new for new, old in enumerate(order)}
        self._factor_cap = {new_of[i]: v for i, v in self._factor_cap.items()}
        self._factor_mode = {new_of[i]: v for i, v in self._factor_mode.items()}
        self._factor_rep = {new_of[i]: v for i, v in self._factor_rep.items()}
        self._factor_last_B = {new_of[i]: v for i, v in self._factor_last_B.items()}
        self._factor_bufs = {(new_of[i], b): v for (i, b), v in self._factor_bufs.items()}
        self._factor = {new_of[i]: (o, n, None if bi is None else new_of[bi])
                        for i, (o, n, bi) in self._factor.items()}
        remap = self.arena.relayout(order)
        for opt in list(self.arena.optimizers):
            opt._relayout(self.arena, remap)
        self._bounds = self._plan_buckets()
        self._build_reducer()
        self._register_hooks()
        self._rebuilt = True

    def settle(self) -> None:
        """Apply a pending bucket rebuild now (eagerly). hipGraph capture calls it first: a
        relayout recorded into a graph would restore stale buffers at every replay."""
        if self._rebuild_order is not None:
            self._rebuild_buckets()
        self._reserve_factor_workspaces()

    def _reserve_factor_workspaces(self) -> None:
        """Size every factored job's workspaces (split-K partials, bias column sums) for the
        CURRENT bucket layout, eagerly: a capture cannot allocate, and the first factored step
        may have run before the bucket rebuild changed the jobs' shapes."""
        if not self._gpu or not self._factor or not self._backend.collective:
            return
        W = self.world_size
        for i, (o, n, bi) in self._factor.items():
            cap = self._factor_cap.get(i)
            if cap is None or 2 * W * cap * (o + n) > o * n:
                continue
            g_all, x_all = self._factor_buffers(i, cap)
            b = self._factor_bucket[i]
            rows = self._rep_rows_for(i, cap)
            self._backend.reserve_factor(self._bounds[b], self._bounds[b + 1], g_all, x_all, cap,
                                         o, n, -1 if bi is None else self.arena.offsets[bi],
                                         rows == o, rows)

    def _make_hook(self, idx):
        arena = self.arena

        def hook(p):
            if self._factor_handed:
                ptr = self._factor_handed.pop(idx, None)
                if ptr is not None and (p.grad is None or p.grad.data_ptr() != ptr):
                    raise RuntimeError(
                        "DDP: the gradient of a Linear parameter updated in its own kernel "
                        f"(factored synchronisation or optimizer epilogue; arena index {idx}, "
                        f"shape {tuple(p.shape)}) received a contribution from an op other than "
                        "its Linear layer (a weight penalty, tied weights, x @ w.t() ...), which "
                        "would be dropped. Construct DDP with factor_sync=False, or register the "
                        "optimizer without fusion, for this model.")
            if not arena.is_arena_grad(idx):
                # a gradient produced outside the native ops: move it into its bucket slot
                slot = arena.grad_view(idx)
                slot.copy_(p.grad)
                p.grad = slot
            if self.require_backward_grad_sync and self.reducer.expecting:
                if not self._callback_queued:
                    torch.autograd.Variable._execution_engine.queue_callback(self._finalize)
                    self._callback_queued = True
                    if self._cur_ev is not None:
                        self._cur_ev["bwd0"] = self._event()
                self.reducer.mark_ready(idx, self._gpu)
        return hook

    def _finalize(self):
        self._callback_queued = False
        ev = self._cur_ev
        if ev is not None:
            ev["bwd1"] = self._event()
        self.reducer.finalize(self._gpu, self.find_unused_parameters)
        if self._iter == 0 and self._rebuild_enabled and self.reducer.iteration == 1:
            if self._gpu and torch.cuda.is_current_stream_capturing():
                # iteration 0 captured (CapturedStep warmup=0): planning needs a broadcast and a
                # host read; keep the initial layout
                self._rebuild_enabled = False
            else:
                self._plan_rebuild()
        if ev is not None:
            ev["comm1"] = self._event()
            self._pending_samples.append(ev)
            self._cur_ev = None
        self._iter += 1

    # --------------------------------------------------------------------------- DDP Logger
    def _event(self):
        if self._gpu:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e
        return time.perf_counter()

    def _elapsed(self, a, b) -> float:
        return a.elapsed_time(b) if self._gpu else (b - a) * 1000.0

    def _collect_samples(self):
        """Turn finished sampled iterations into (forward, backward compute, backward comm) ms.
        Backward comm = end of backward compute -> every bucket done (the exposed part) plus the
        communicator's own time when the backend measured it."""
        keep = []
        for ev in self._pending_samples:
            if self._gpu and not ev["comm1"].query():
                keep.append(ev)
                continue
            fwd = self._elapsed(ev["fwd0"], ev["fwd1"])
            bwd = self._elapsed(ev["bwd0"], ev["bwd1"]) if "bwd0" in ev else float("nan")
            tail = self._elapsed(ev["bwd1"], ev["comm1"])
            self._samples.append((fwd, bwd, tail))
        self._pending_samples = keep

    def _sync_buffers(self):
        if self.world_size == 1:
            return
        for flat in self.buffers_arena.flats:
            rt.broadcast(flat, 0)

    # --------------------------------------------------------------------------- debug
    def replica_checksum(self) -> torch.Tensor:
        """Bit-exact checksum of the flat parameter arena: [sum of the int32 words, sum of the
        words weighted by (index mod 65521) + 1] as int64 (order-sensitive, dtype-agnostic)."""
        with torch.no_grad():
            words = self.arena.data.view(torch.int32).to(torch.int64)
            w = (torch.arange(words.numel(), device=words.device, dtype=torch.int64) % 65521) + 1
            return torch.stack([words.sum(), (words * w).sum()])

    def check_replicas(self) -> None:
        """Raise if any rank's parameters differ from rank 0's (all-gather of the checksums)."""
        local = self.replica_checksum()
        if self.world_size == 1:
            return
        gathered = rt.all_gather_flat(local).view(self.world_size, 2)
        bad = [r for r in range(self.world_size) if not torch.equal(gathered[r], gathered[0])]
        if bad:
            raise RuntimeError(f"DDP replicas diverged at iteration {self._iter}: ranks {bad} "
                               f"hold different parameters than rank 0 "
                               f"(checksums {gathered.tolist()})")

    # --------------------------------------------------------------------------- nn.Module
    def forward(self, *inputs, **kwargs):
        sample = self._pre_forward()
        out = self.module(*inputs, **kwargs)
        if sample:
            self._cur_ev["fwd1"] = self._event()
        return out

    def _pre_forward(self) -> bool:
        """Per-iteration bookkeeping before the module runs (replica checks, a pending bucket
        rebuild, fused-optimizer hyper-parameters, the reducer's next iteration, buffer
        broadcast); True when this iteration's timing is sampled. Also driven by the forward
        pre-hook of a model an ``Accelerator`` prepared in one process (accelerate/accelerator.py
        ``prepare_model``: the module is returned unwrapped, as Accelerate does)."""
        if self.check_replicas_every and self._iter and \
                self._iter % self.check_replicas_every == 0 and torch.is_grad_enabled() and \
                not (self._gpu and torch.cuda.is_current_stream_capturing()):
            self.check_replicas()  # (a captured step checks after its replays: CapturedStep)
        sample = (self._sample_every and torch.is_grad_enabled() and
                  self._iter % self._sample_every == 0 and
                  not (self._gpu and torch.cuda.is_current_stream_capturing()))
        if sample:
            self._cur_ev = {"fwd0": self._event()}
        if self._rebuild_order is not None:
            if self._gpu and torch.cuda.is_current_stream_capturing():
                # the relayout allocates and copies: inside a capture it would be recorded into
                # the graph and every replay would restore the pre-capture parameters
                raise RuntimeError("DDP bucket rebuild pending while a hipGraph is being "
                                   "captured: call ddp.settle() (CapturedStep does) before "
                                   "capturing")
            self._rebuild_buckets()
        self._factor_handed.clear()
        self._factor_x_ready.clear()
        self._factor_g_ready.clear()
        self._factor_keep.clear()
        if torch.is_grad_enabled() and self.require_backward_grad_sync:
            if self._fused_opt is not None:
                # hyper-parameters as they are NOW (after any LR-scheduler step) drive this
                # iteration's in-reduction update: a stream-ordered write into the device block
                # when something changed, before the block is advanced by prepare_for_backward
                self._fused_opt.sync_hyper()
            self._uses.clear()
            # a backward that never finished (an exception, a failed hipGraph capture) left its
            # end-of-backward callback unqueued-but-flagged: this iteration queues its own
            self._callback_queued = False
            self.reducer.prepare_for_backward(self._gpu)
            if self._fused_opt is not None and self._opt_begin_countdown > 0:
                self._opt_begin_countdown -= 1
                if self._opt_begin_countdown == 0:
                    self._backend.skip_opt_begin = True
        if self.broadcast_buffers and self.world_size > 1 and self.module.training:
            with torch.no_grad():
                self._sync_buffers()
        return bool(sample)

    @contextlib.contextmanager
    def no_sync(self):
        old = self.require_backward_grad_sync
        self.require_backward_grad_sync = False
        try:
            yield
        finally:
            self.require_backward_grad_sync = old

    # --------------------------------------------------------------------------- fused optimizer
    def register_fused_optimizer(self, optimizer, shard: bool | None = None,
                                 clip_grad_norm: float | None = None) -> bool:
        """Apply ``optimizer`` bucket by bucket inside the reduction (torch's
        ``DDP._register_fused_optim``): each bucket's parameters are updated right after its
        gradient is averaged. ``optimizer.step()`` becomes a no-op. The optimizer's per-step
        scalars live in its device hyper block (csrc/kernels.h HyperSlot): the DDP forward pushes
        host-side changes (LR schedulers) and the reducer advances the Adam step count on the
        device, so a captured hipGraph step stays correct. Requires a tdp SGD/Adam over exactly
        this DDP's parameters (one param group).

        ``shard`` (default: world_size > 1) turns each bucket's all-reduce into reduce-scatter ->
        update of this rank's 1/W slice -> all-gather of the updated parameters (ZeRO stage 1
        inside DDP, cf. torch's ZeroRedundancyOptimizer): the same bytes over xGMI, 1/W of the
        optimizer's HBM traffic, identical parameters on every rank. Afterwards ``p.grad`` holds
        the averaged gradient only inside this rank's slices, and optimizer state is current only
        there until :meth:`consolidate_optimizer_state` (the checkpoint helpers call it).

        ``clip_grad_norm`` = max_norm: ``torch.nn.utils.clip_grad_norm_`` of the averaged
        gradient applied before the update, inside the reduction (the norm of the whole model is
        reduced on the device -- one 1-element all-reduce when sharded -- and the update kernels
        scale their gradient by the coefficient; updates then wait for the last bucket).
        Returns True."""
        from ..optim.fused import SGD, Adam

        if self.find_unused_parameters:
            raise ValueError("a fused optimizer needs every parameter to get a gradient")
        if len(optimizer.param_groups) != 1:
            raise ValueError("fused optimizer: exactly one parameter group is supported")
        params = optimizer.param_groups[0]["params"]
        if {id(p) for p in params} != {id(p) for p in self.arena.params}:
            raise ValueError("fused optimizer must own exactly the DDP model's parameters")
        if not isinstance(optimizer, (SGD, Adam)):
            raise TypeError("fused optimizer must be tdp.optim.SGD / Adam / AdamW")
        if optimizer.param_groups[0].get("grad_scale", 1.0) != 1.0:
            raise ValueError("fused optimizer: grad_scale must be 1 (ncclAvg already averages)")
        self._fused_opt = optimizer
        optimizer._fused_ddp = self
        self._fused_shard = bool(self.world_size > 1 if shard is None else shard) and \
            self.world_size > 1
        self._clip_global = float(clip_grad_norm) if clip_grad_norm else None
        self.push_fused_hyper(optimizer, initial=True)
        if self._factor:
            # the replicated / sharded / split choice's xGMI input, measured HERE -- eagerly, on
            # every rank at the same point (registration is part of the setup every rank runs) --
            # never inside a backward hook: the choice is then fixed before the first
            # step, and a pinned bandwidth (TDP_FACTOR_BUSBW=GB/s) makes it reproducible
            self._probe_bandwidth(max(4 * o * n for o, n, _ in self._factor.values()))
        return True

    def factor_capacity(self, rows: int) -> None:
        """Agree the factored jobs' per-rank slot size (rows of g / x per rank) up front: the max
        over ranks of ``rows`` and of any slot already agreed. Every rank must call it at the
        same point, eagerly (one all-reduce). Needed when a later step's per-rank batch can
        exceed the first factored step's (a resumed ragged batch first): such a step otherwise
        raises (factor_submit) rather than re-agreeing from a subset of the ranks."""
        t = torch.tensor([int(rows)] + [int(v) for v in self._factor_cap.values()],
                         dtype=torch.int64, device=self.device)
        rt.all_reduce(t, "max")
        cap = int(t.max().item())
        self._factor_min_cap = cap
        for i in list(self._factor_cap):
            if self._factor_cap[i] != cap:
                self._factor_cap[i] = cap
                for k in [k for k in self._factor_bufs if k[0] == i]:
                    del self._factor_bufs[k]

    def _factor_candidates(self) -> dict:
        """Linear weights W[out][in] whose gradient synchronisation can be factored (reducer.h
        FactorJob): (1/W) sum_r g_r^T x_r has rank <= W*B, so all-gathering the factors g_r
        [B][out] and x_r [B][in] and computing this rank's row shard of the average with one
        depth-W*B GEMM (fused optimizer in its epilogue) replaces the reduce-scatter of the
        out*in gradient; the updated rows are all-gathered as in the sharded update. Needs the
        fused optimizer with sharding (or the one-GPU rehearsal: world size 1 with collectives
        forced), no clipping / compression, out % 4W == 0 and whole-row shards that are
        multiples of 64 elements (SyncBackend.owned_shard); on CPU arenas only when requested
        explicitly (the gloo twin). Per-rank batches may differ: the slot size is agreed once
        (factor_submit) and smaller batches are zero-padded.

        Gradient note: a factored weight's ``p.grad`` is NOT its gradient after backward -- the
        job computes this rank's rows of the averaged gradient straight into the update (sharded:
        only the owned rows hold it; the rest of the slot is stale arena memory). Read
        gradients with factor_sync=False when you need them."""
        from ..nn.modules import Linear

        W = self.world_size
        if self._fused_opt is None or self._factor_pref is False:
            return {}
        if not self._gpu and self._factor_pref is not True:
            # CPU arenas: the gloo twin (_CpuSyncOps.factor_sync) only when asked for explicitly
            # (factor_sync=True / TDP_FACTOR_SYNC=1) -- the multi-rank tests of the algorithm
            return {}
        if self._clip_global or self._clip_local or self._compression not in (None, "none"):
            return {}
        rehearsal = W == 1 and (self._force_collective or
                                os.environ.get("TDP_FORCE_COLLECTIVE", "0") == "1")
        if not (self._fused_shard or rehearsal):
            return {}
        index = {id(p): i for i, p in enumerate(self.arena.params)}
        out = {}
        for m in self.module.modules():
            if not isinstance(m, Linear) or m.weight.dim() != 2 or id(m.weight) not in index:
                continue
            o, n = m.weight.shape
            if o % (4 * W) or n % 4 or ((o // W) * n) % 64:
                continue
            bias = m.bias if m.bias is not None and id(m.bias) in index else None
            out[index[id(m.weight)]] = (int(o), int(n), index[id(bias)] if bias is not None
                                        else None)
        return out

    def _configure_factor(self):
        """Recompute the factored weights; re-plan the buckets (each gets its own) when the set
        changed. Called from _configure_fused: registration, comm hook, clipping changes."""
        cand = self._factor_candidates()
        for i, p in enumerate(self.arena.params):
            p._tdp_factor = weakref.ref(self) if i in cand else None
        if cand != self._factor:
            self._factor = cand
            self._factor_bufs.clear()
            self._bounds = self._plan_buckets()
            if cand and self._busbw is None and not (
                    self._gpu and torch.cuda.is_current_stream_capturing()):
                #  the factored set became non-empty after registration too (a
                # clipping change, a comm hook): measure the all-gather input of the
                # replicated-vs-sharded choice here, eagerly, instead of silently using the
                # fixed price model
                self._probe_bandwidth(max(4 * o * n for o, n, _ in cand.values()))
            return True
        return False

    def _configure_fused(self):
        """(Re-)apply the fused-optimizer configuration to the current backend."""
        if self._configure_factor():
            self._build_reducer()  # new bucket bounds (calls back into _configure_fused)
            return
        opt = self._fused_opt
        b = self._backend
        # SGD: the hyper block's per-iteration advance (first-step flags) matters for the first
        # two iterations after (re)binding only; then its launch is skipped (SyncBackend)
        b.skip_opt_begin = False
        self._opt_begin_countdown = 2
        b.shard = self._fused_shard
        b.clip = 1 if self._clip_global else (2 if self._clip_local else 0)
        self._bind_fused_buffers(opt)
        b.fused_kind = opt._kind
        # world size 1: the local gradient is already the average, so weight-gradient GEMMs may
        # apply the update in their epilogue (TDP_OPT_EPILOGUE=0 keeps the per-bucket update)
        self._epi_index = {id(p): i for i, p in enumerate(self.arena.params)}
        self._epi_on = (self._gpu and os.environ.get("TDP_OPT_EPILOGUE", "1") != "0" and
                        bool(b.epilogue_allowed))
        me = weakref.ref(self) if self._epi_on else None
        owner = weakref.ref(self)
        for p in self.arena.params:
            p._tdp_epi = me
            p._tdp_fused_owner = owner  # tdp.nn.utils.clip_grad_norm_ refuses these grads

    def _bind_fused_buffers(self, opt):
        from ..optim.fused import SGD, hyper_slots

        g = opt.param_groups[0]
        a = self.arena
        S = hyper_slots()
        if isinstance(opt, SGD):
            buf, fresh = None, False
            if g["momentum"] != 0:
                # fresh == the momentum buffers were just created: the first update initialises
                # them with the gradient (torch: buf = clone(grad)), via the block's first flag
                bufs, fresh = opt._flat_state(a, ("momentum_buffer",))
                buf = bufs["momentum_buffer"]
            blk = opt.hyper_block(0, device=self.device, first=fresh)
            if fresh:
                opt._request_first(blk)
            if self._gpu:
                self._ops.set_fused_sgd(a.data, buf, g["momentum"] != 0, g["nesterov"],
                                        g["maximize"], blk)
            else:
                self._cpu_ops.set_fused(opt, blk, {"momentum_buffer": buf})
        else:
            keys = opt._keys(g)
            bufs, _ = opt._flat_state(a, keys)
            blk = opt.hyper_block(0, device=self.device, step=opt._current_flat_step(a))
            if self._gpu:
                self._ops.set_fused_adam(a.data, bufs["exp_avg"], bufs["exp_avg_sq"],
                                         bufs.get("max_exp_avg_sq"), g["amsgrad"], g["maximize"],
                                         opt._decoupled, blk)
            else:
                self._cpu_ops.set_fused(opt, blk, bufs)
        if self._clip_global:
            blk[S["max_norm"]] = float(self._clip_global)
        opt.sync_hyper()

    def push_fused_hyper(self, opt, initial: bool = False):
        """Bind the optimizer's buffers and device block to the reducer (``initial``: after
        registration or load_state_dict); later calls only push changed scalars."""
        if initial:
            self._configure_fused()
        else:
            opt.sync_hyper()

    def clip_grad_norm_before_aggregation(self, max_norm: float | None) -> None:
        """The README pitfall "clip gradients before they are aggregated" (REF/README.md:92-95):
        every rank scales its OWN gradient to norm <= max_norm before any byte goes on the wire,
        so one rank's exploding gradient cannot dominate the average. The local norm needs the
        whole local gradient, so all bucket collectives move to the end of backward. None turns
        it off."""
        if max_norm is not None and self._clip_global:
            raise ValueError("choose either the global in-reduction clip or the local one")
        self._clip_local = float(max_norm) if max_norm else None
        self._configure_local_clip()
        if self._fused_opt is not None:
            self._configure_fused()

    def _configure_local_clip(self):
        from ..optim.fused import hyper_slots

        b = self._backend
        if self._clip_local is None:
            b.clip = 1 if self._clip_global else 0
            return
        S = hyper_slots()
        if self._clip_block is None:
            self._clip_block = torch.zeros(S["size"], device=self.device)
            self._clip_block[S["scale"]] = 1.0
        self._clip_block[S["max_norm"]] = self._clip_local
        if self._gpu:
            self._ops.set_clip_block(self._clip_block)
        else:
            self._cpu_ops.clip_block = self._clip_block
        b.clip = 2

    def last_grad_norm(self) -> torch.Tensor | None:
        """Total gradient norm computed by the in-reduction clip of the last step (device
        scalar; the local clip reports this rank's norm), or None without clipping."""
        from ..optim.fused import hyper_slots

        n = hyper_slots()["norm"]
        if self._clip_local is not None:
            return self._clip_block[n]
        if self._clip_global and self._fused_opt is not None:
            return self._fused_opt.hyper_block(0)[n]
        return None

    def _note_use(self, p):
        self._uses[id(p)] = self._uses.get(id(p), 0) + 1

    def epilogue_slot(self, p):
        """(backend, arena offset) for an optimizer-epilogue weight-gradient GEMM of ``p`` in the
        current backward, or None when the update must stay in the bucket path (also when ``p``
        was used more than once in this forward: its gradient is the sum of several GEMMs)."""
        if not (self._epi_on and self.require_backward_grad_sync and self.reducer.expecting and
                self._backend.epilogue_allowed):
            return None
        if self._uses.get(id(p), 0) != 1:
            return None
        i = self._epi_index.get(id(p))
        if i is None or not self.arena.numels[i]:
            return None
        return self._backend, self.arena.offsets[i]

    def bias_epilogue(self, b):
        """(backend, arena offset, span) when the bias ``b`` may be updated by the kernel that
        reduces its gradient (the weight-gradient GEMM's row sums, the fused head backward) at
        world size 1; span covers the alignment padding up to the next parameter so no flat
        update pass remains for it. None otherwise."""
        if not (self._epi_on and self.require_backward_grad_sync and self.reducer.expecting and
                self._backend.epilogue_allowed):
            return None
        i = self._epi_index.get(id(b))
        if i is None or not self.arena.numels[i]:
            return None
        off = self.arena.offsets[i]
        later = [o for o in self.arena.offsets if o > off]
        return self._backend, off, (min(later) if later else self.arena.numel) - off

    def note_handed(self, p, t) -> None:
        """``t`` is the gradient of ``p`` handed to autograd unwritten (a kernel applied the
        update, or the factored job owns it): the post-accumulate hook raises if another op
        added to it (the contribution would be lost)."""
        i = self._epi_index.get(id(p))
        if i is not None:
            self._factor_handed[i] = t.data_ptr()

    def factor_slot(self, p):
        """This DDP when the weight-gradient GEMM of ``p`` should be replaced by the factored
        synchronisation in the current backward (see _factor_candidates), else None."""
        i = self._epi_index.get(id(p))
        if i is None or i not in self._factor or not self.require_backward_grad_sync or \
                not self.reducer.expecting or self._uses.get(id(p), 0) != 1 or p.grad is not None:
            return None
        return self

    def factor_g_dest(self, p, B: int):
        """Where the producer of factored weight ``p``'s output gradient g [B][out] should write
        it: this rank's slot of the job's gather buffer, so the g all-gather runs IN PLACE (no
        local copy of g -- part of RCCL's all-gather at W > 1, a whole blit on the critical path
        of the one-GPU rehearsal). The producer is the consumer layer's input-gradient GEMM,
        whose epilogue applies ``p``'s ReLU mask (ops/linear.py): its output IS g. None when
        ``p`` is not factored in this backward or the slot does not fit (the producer then
        allocates as usual and the gather reads g out of place)."""
        if not self._gpu:
            return None
        i = self._epi_index.get(id(p))
        if i is None or i not in self._factor or self.factor_slot(p) is None:
            return None
        o, n, _ = self._factor[i]
        cap = self._factor_cap.get(i)
        if cap is None or B != cap or self._factor_x_ready.get(i) != B or \
                2 * self.world_size * cap * (o + n) > o * n:
            return None
        g_all = self._factor_buffers(i, cap)[0]
        return g_all[self.rank * cap * o:(self.rank + 1) * cap * o].view(cap, o)

    def _g_in_slot(self, i, cap, g) -> bool:
        """``g`` is this rank's slot of weight ``i``'s gather buffer (factor_g_dest)."""
        o = self._factor[i][0]
        return g.data_ptr() == self._factor_buffers(i, cap)[0][self.rank * cap * o:].data_ptr()

    def _factor_buffers(self, i, cap):
        o, n, _ = self._factor[i]
        key = (i, cap)
        bufs = self._factor_bufs.get(key)
        if bufs is None:
            W = self.world_size
            bufs = (torch.empty(W * cap * o, device=self.device),
                    torch.empty(W * cap * n, device=self.device))
            self._factor_bufs[key] = bufs
        return bufs

    def factor_forward(self, p, x: torch.Tensor) -> bool:
        """Forward of a factored Linear weight ``p`` with input ``x`` [B][in] (VERDICT r3 item
        3): x is this rank's input factor already, so it is staged into its slot now and its
        all-gather issued on the comm stream (SyncBackend.prefetch_factor_x) -- overlapping the
        rest of forward and backward instead of sitting in front of the layer's weight-gradient
        job at the end of backward. The caller launches the layer's GEMM next and then calls
        :meth:`factor_flush` (the captured fork then follows the compute chain's node). True when
        the gather was issued. Only once the slot size is agreed (the first factored step gathers
        x in backward) and only on the device backend; every rank takes the same decision (the
        agreed slot, the model's structure)."""
        i = self._epi_index.get(id(p))
        if i is None or i not in self._factor or not self._gpu or \
                not self.require_backward_grad_sync or not self.reducer.expecting or \
                self._uses.get(id(p), 0) != 1 or p.grad is not None or \
                not self._backend.collective:
            return False
        cap = self._factor_cap.get(i)
        o, n, _ = self._factor[i]
        W = self.world_size
        B = int(x.shape[0])
        if cap is None or B > cap or x.shape != (B, n) or 2 * W * cap * (o + n) > o * n:
            return False
        if x.stride(1) != 1 or x.stride(0) != n:
            x = x.contiguous()
        bufs = self._factor_buffers(i, cap)
        if B == cap:
            # out of place: the all-gather reads this rank's rows straight from x (no staging
            # copy); x is kept alive until the next iteration -- the collective runs on the side
            # stream, and the end-of-backward join orders it before anything that reuses x's memory
            self._factor_keep.append(x)
            self._backend.prefetch_factor_x(self._factor_bucket[i], bufs[1], cap, n, x)
        else:  # a ragged batch: staged into slot r, zero-padded to the agreed rows
            xs = bufs[1].view(W, cap, n)[self.rank]
            xs[:B].copy_(x)
            xs[B:].zero_()
            self._backend.prefetch_factor_x(self._factor_bucket[i], bufs[1], cap, n)
        self._factor_x_ready[i] = B
        return True

    def factor_flush(self) -> None:
        self._backend.flush()

    def factor_prefetch_g(self, p, g: torch.Tensor) -> bool:
        """Start of the backward of a factored weight ``p`` (device path): issue the all-gather
        of this rank's output-gradient factor ``g`` [B][out] NOW, before the layer's input-
        gradient GEMM, so the gather overlaps that GEMM instead of following it (the step model
        of docs/COMM_MODEL.md assumes exactly this); :meth:`factor_submit` then arms the job
        with nothing left to gather. Only when x went out at forward time (every rank alike:
        the decision uses agreed values; a ragged batch is staged, a full one read in place);
        the caller launches
        the GEMM and then calls :meth:`factor_flush`. True when the gather was issued.

        Also called one layer EARLY, by the consumer of ``p``'s (fused ReLU) output, with its
        gated input gradient -- which is ``p``'s g -- right after its input-gradient GEMM
        (ops/linear.py): the gather then precedes the consumer's parameter all-gather on the
        comm stream. ``p``'s own backward finds it issued for the same tensor and returns True;
        for a different g (the output had other consumers) it gathers again."""
        i = self._epi_index.get(id(p))
        if i is None or i not in self._factor or not self._gpu:
            return False
        o, n, _ = self._factor[i]
        B = int(g.shape[0])
        # keyed by the tensor's version too: autograd may accumulate another consumer's
        # gradient into the same storage in place after the early gather
        if self._factor_g_ready.get(i) == (B, g.data_ptr(), g._version):
            return True  # issued early from the consumer's backward
        cap = self._factor_cap.get(i)
        if cap is None or B > cap or self._factor_x_ready.get(i) != B or \
                g.shape != (B, o) or not g.is_contiguous() or \
                2 * self.world_size * cap * (o + n) > o * n:
            return False
        bufs = self._factor_buffers(i, cap)
        if B == cap and self._g_in_slot(i, cap, g):
            # the producer wrote g into this rank's slot (factor_g_dest): gathered in place
            self._backend.prefetch_factor_x(self._factor_bucket[i], bufs[0], cap, o)
        elif B == cap:
            self._factor_keep.append(g)  # read by the side stream; alive until the next forward
            # the same generic rows all-gather as x's (W slots of cap rows), out of place
            self._backend.prefetch_factor_x(self._factor_bucket[i], bufs[0], cap, o, g)
        else:
            # a ragged batch on this rank: staged into slot r, zero-padded (unscaled, as in
            # factor_submit), and gathered in place -- at the SAME point of the collective
            # sequence as the full-batch ranks' gather (the early gather would otherwise run
            # before the consumer's parameter all-gather on some ranks and after it on others)
            native().factor_stage(g, None, bufs[0], bufs[1], self.rank, 1.0, cap)
            self._backend.prefetch_factor_x(self._factor_bucket[i], bufs[0], cap, o)
        self._factor_g_ready[i] = (B, g.data_ptr(), g._version)
        return True

    def factor_submit(self, p, g: torch.Tensor, x: torch.Tensor, dw=None) -> bool:
        """Stage this rank's factors of ``p``'s gradient (g [B][out] = dL/dy, x [B][in]) and
        arm its bucket; False when factoring does not pay at the agreed batch size (the caller
        then runs the ordinary weight-gradient GEMM). Must run before ``p``'s gradient hook.
        When True, the layer's bias (if any) is averaged and updated by the same job: the caller
        must not compute its gradient, and ``dw`` (the tensor handed to autograd unwritten) must
        be what reaches ``p.grad`` -- the hook raises if another op added to it.

        Cross-rank agreement: whether a weight is factored and with how many rows per rank must
        be identical everywhere (the all-gathers are collectives). The first factored step
        agrees the slot size (max per-rank batch, one all-reduce; it must run eagerly); later
        steps zero-pad smaller batches into it (a ragged last batch on one rank contributes only
        its rows), so the decision depends on agreed values only. A batch larger than the slot
        re-agrees a larger one in eager execution and raises inside a capture."""
        i = self._epi_index[id(p)]
        o, n, bi = self._factor[i]
        B = int(g.shape[0])
        W = self.world_size
        if g.shape != (B, o) or x.shape != (B, n):
            raise RuntimeError(f"factor_submit: factors {tuple(g.shape)} / {tuple(x.shape)} do "
                               f"not match the weight [{o}, {n}]")
        cap = self._factor_cap.get(i)
        if cap is None:
            if self._gpu and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("DDP factored synchronisation: the first step must run "
                                   "eagerly (it agrees the per-rank batch across ranks) before "
                                   "a hipGraph capture")
            t = torch.tensor([max(B, self._factor_min_cap)], dtype=torch.int64,
                             device=self.device)
            rt.all_reduce(t, "max")
            cap = int(t.item())
            self._factor_cap[i] = cap
        if B > cap:
            # Fail fast, never re-agree here: only the ranks whose batch exceeds the slot reach
            # this point, so a collective here would pair with the other ranks' factor
            # all-gathers (mismatched collectives, a hang until the watchdog). The launcher's
            # fail-fast then ends every rank. Agree a larger slot up front instead
            # (factor_capacity, every rank at the same point).
            raise RuntimeError(
                f"DDP factored synchronisation: per-rank batch {B} exceeds the {cap} rows agreed "
                f"at the first factored step; call ddp.factor_capacity({B}) on every rank before "
                "the first step (or construct DDP with factor_sync=False)")
        if 2 * W * cap * (o + n) > o * n:
            self._factor_mode[i] = "bucket"
            return False
        g = g if g.is_contiguous() else g.contiguous()
        x = x if x.is_contiguous() else x.contiguous()
        bufs = self._factor_buffers(i, cap)
        if not self._gpu:  # the CPU twin finds its host buffers by address
            for t in bufs:
                self._cpu_ops.factor_bufs[t.data_ptr()] = t
        # the forward of this iteration staged and gathered x already (factor_forward)
        x_ready = self._gpu and self._factor_x_ready.pop(i, None) == B
        # device path: the slots hold UNSCALED g on every rank and the update applies the 1/W
        # (g_scale) -- one convention whether a rank's slot is read in place (full batch) or
        # staged (ragged batch), since ranks may take different branches in the same step
        g_ready = self._gpu and x_ready and \
            self._factor_g_ready.pop(i, None) == (B, g.data_ptr(), g._version)
        g_src = None
        if g_ready:
            pass  # gathered before the dgrad GEMM (factor_prefetch_g), from g itself
        elif self._gpu and x_ready and B == cap and self._g_in_slot(i, cap, g):
            pass  # written into this rank's slot by its producer (factor_g_dest): in place
        elif self._gpu and x_ready and B == cap:
            # out of place: the all-gather reads this rank's g where the layer's backward wrote
            # it (no staging kernel at all)
            g_src = g
            self._factor_keep.append(g)
        elif self._gpu:
            native().factor_stage(g, None if x_ready else x, bufs[0], bufs[1], self.rank,
                                  1.0, cap)
        else:
            with torch.no_grad():
                gs = bufs[0].view(W, cap, o)[self.rank]
                xs = bufs[1].view(W, cap, n)[self.rank]
                gs[:B].copy_(g).mul_(1.0 / W)
                gs[B:].zero_()
                xs[:B].copy_(x)
                xs[B:].zero_()
        rows = self._rep_rows_for(i, cap)
        self._backend.arm_factor(self._factor_bucket[i], bufs[0], bufs[1], cap, o, n,
                                 -1 if bi is None else self.arena.offsets[bi],
                                 self._factor_bias_bucket.get(i, -1), replicate=rows == o,
                                 rep_rows=rows, g_src=g_src,
                                 g_scale=1.0 / W if self._gpu else 1.0, g_ready=bool(g_ready),
                                 x_ready=bool(x_ready))
        self._factor_last_B[i] = B
        self._factor_rep[i] = rows
        self._factor_mode[i] = ("factored-replicated" if rows == o else
                                "factored-split" if rows > 0 else "factored-sharded")
        if dw is not None:
            self._factor_handed[i] = dw.data_ptr()
        return True

    def sync_plan(self) -> dict:
        """How each parameter's gradient was synchronised in the last step, by name:
        "factored-replicated" / "factored-sharded" (Linear weights, see _factor_candidates),
        "factored-bias" (averaged and updated by its weight's job), "bucket" (a factor
        candidate whose job did not pay at this batch size), "sharded" (reduce-scatter ->
        update 1/W -> all-gather), "allreduce", or "local" (one rank: no collective)."""
        names = {id(p): n for n, p in self.module.named_parameters()}
        biases = {bi: i for i, (_, _, bi) in self._factor.items() if bi is not None}
        if not self._backend.collective:
            default = "local"
        elif self._fused_shard and self._fused_opt is not None and not self._compression:
            default = "sharded"
        else:
            default = "allreduce"
        plan = {}
        for i, p in enumerate(self.arena.params):
            mode = self._factor_mode.get(i, default if i not in self._factor else "bucket")
            if i in biases:
                w = self._factor_mode.get(biases[i], "")
                mode = "factored-bias" if w.startswith("factored") else default
            plan[names.get(id(p), f"param{i}")] = mode
        return plan

    def factor_report(self) -> dict:
        """The factored weights' decision inputs and outcome, for the record: replicated rows
        of each weight's last job (of its ``out`` rows; 0 = sharded), the agreed slot rows and
        the all-gather bus bandwidth the choice was made with (measured at registration, or
        pinned by TDP_FACTOR_BUSBW). Pin the rows for a reproducible run with
        ``factor_replicate`` = {name: True / False / fraction}."""
        rows = {self._param_name(self.arena.params[i]): {"rep_rows": int(r),
                                                         "out_rows": int(self._factor[i][0])}
                for i, r in self._factor_rep.items() if i in self._factor}
        src = ("fallback price model (no bandwidth measured)" if self._busbw is None else
               "pinned (TDP_FACTOR_BUSBW)" if self._busbw.get("pinned") else "measured")
        return {"rows": rows, "slot_rows": sorted(set(self._factor_cap.values())),
                "busbw": self._busbw, "busbw_source": src}

    # Fallback price model when no bandwidth was measured (CPU twin, tests): the replicated
    # update's extra GEMM rows cost 2*W*B*(1 - 1/W) FLOP at ~150 TF/s plus (1 - 1/W) * 16 B of
    # optimizer traffic at ~5 TB/s; the all-gather they replace moves 4 * (W - 1)/W B per element
    # at ~300 GB/s: replication pays while W*B is below ~760.
    _REPLICATE_MAX_WB = 768

    @classmethod
    def _replicate_pays(cls, W: int, B: int) -> bool:
        # world size 1 (the one-GPU rehearsal): every row is this rank's anyway; replicating
        # skips the in-place parameter all-gather a sharded job would still issue
        return W * B <= cls._REPLICATE_MAX_WB

    def _probe_bandwidth(self, nbytes: int) -> None:
        """Measure the all-gather bus bandwidth once (eager, every rank at the same point: the
        first factored step) and agree on the minimum: the measured xGMI input of the
        replicated-vs-sharded choice (parallel/commmodel.py) instead of an assumed constant."""
        pinned = os.environ.get("TDP_FACTOR_BUSBW")
        if pinned and self._busbw is None:
            self._busbw = {"all_gather": float(pinned), "bytes": 0, "pinned": True}
        if self._busbw is not None or not self._gpu or self.world_size == 1 or \
                rt.comm() is None:
            return
        from . import commbench

        size = int(min(max(nbytes, 8 << 20), 64 << 20))
        r = commbench.collective_busbw([size], ops=("all_gather",), iters=3, warmup=1)
        t = torch.tensor([r[0]["busbw_GBps"]], dtype=torch.float64, device=self.device)
        rt.all_reduce(t, "min")
        self._busbw = {"all_gather": float(t.item()), "bytes": size}

    @staticmethod
    def _split_rows(o: int, n: int, W: int, f: float) -> int:
        """Replicated rows of a split job replicating ~``f`` of the ``o`` rows: the sharded rest
        is W equal whole-row shards of a multiple of 64 elements (SyncBackend.owned_shard)."""
        import math

        # rows per rank: a shard of 64-element multiples, and 16 rows at least (16-B aligned
        # A columns for the fast GEMM's loads, fewer partial tiles)
        u64 = 64 // math.gcd(n, 64)
        unit = u64 * 16 // math.gcd(u64, 16)
        q = int(round((1.0 - f) * o / W / unit)) * unit
        q = max(0, min(q, o // W // unit * unit))
        rows = o - W * q
        return o if q == 0 else rows

    def _param_name(self, p) -> str:
        """Module name of parameter ``p`` (the arena keeps the Parameter objects across a
        rebuild, so the map by identity stays valid)."""
        names = getattr(self, "_names_by_id", None)
        if names is None or id(p) not in names:
            names = {id(q): n for n, q in self.module.named_parameters()}
            self._names_by_id = names
        n = names.get(id(p))
        if n is None:
            n = "param%d" % next(k for k, q in enumerate(self.arena.params) if q is p)
        return n

    def _rep_rows_for(self, i, cap) -> int:
        """How many rows of factored weight ``i`` every rank computes itself: all of them
        (replicated), none (sharded) or a share (split: parallel/commmodel.py
        "factored-split"). An explicit ``factor_replicate`` (True / False / "split" / a fraction,
        or {parameter name: one of these}: tune_factor_replicate's result; names, not arena
        indices, because a bucket rebuild re-orders the arena) decides, else the step model with
        the measured all-gather bandwidth, else the fallback rule. Identical on every rank
        (agreed inputs only). The CPU twin knows replicated and sharded only."""
        o, n, _ = self._factor[i]
        W = self.world_size
        if W == 1:
            return o
        rep = self.factor_replicate
        if isinstance(rep, dict):
            rep = rep.get(self._param_name(self.arena.params[i]))
        if rep is True or rep is False:
            return o if rep else 0
        from . import commmodel as cm

        hw = cm.Hardware(busbw_GBps={"all_gather": self._busbw["all_gather"]}) \
            if self._busbw is not None else cm.Hardware()
        lay = cm.Layer(f"w{i}", o, n, 0.0, 0.0, 0.0)
        if isinstance(rep, float) and 0.0 < rep < 1.0:
            f = rep
        elif rep == "split":
            f = cm.job_cost(lay, "factored-split", W, cap, hw)["rep_fraction"]
        else:  # auto
            if self._busbw is None:
                return o if self._replicate_pays(W, cap) else 0
            costs = {m: cm.job_cost(lay, m, W, cap, hw)
                     for m in ("factored-replicated", "factored-sharded", "factored-split")}
            best = min(costs, key=lambda m: costs[m]["g_us"])
            if best == "factored-replicated":
                return o
            if best == "factored-sharded":
                return 0
            f = costs[best]["rep_fraction"]
        if not self._gpu:
            return o if f >= 0.5 else 0
        return self._split_rows(o, n, W, f)

    def tune_factor_replicate(self, step_fn, iters: int = 3, capture: bool = False,
                              comm_cus=None, repeats: int = 1):
        """Measure, don't guess: time ``step_fn`` (one full training step) under every
        replicated / sharded / split combination of the factored weights (each weight on its
        own: up to two weights, 3^k combinations; more: the three uniform plans), take the max
        over ranks, keep the fastest (``factor_replicate`` = {parameter name: choice}), record
        the timings in ``factor_tuning``. ``capture=True`` times
        the step as it will run -- captured into a hipGraph and replayed, collectives on the side
        stream overlapping backward -- instead of eagerly (collectives then serialise on the
        compute stream and the comparison is skewed: VERDICT r3 weak 2). Every rank must call it
        at the same point (it issues collectives). Optimizer state is consolidated before each
        combination (a weight that was sharded has current state in its own rows only). No-op
        (returns None) without factored weights, at world size 1, or when TDP_FACTOR_REPLICATE
        forces a mode. On the CPU twin (gloo tests) it times replicated / sharded eagerly.
        ``comm_cus`` (GPU): also try these counts of CUs left free for the collectives' kernels
        (grid-sized GEMMs -- the persistent optimizer-epilogue GEMM fills every CU's LDS -- plan
        for CUs - N, native set_reserved_cus): a collective that overlaps such a GEMM can only
        start on CUs it leaves free, which the one-GPU box cannot measure. The fastest
        (modes, N) pair is kept."""
        import itertools

        if not self._factor or self.world_size == 1 or \
                os.environ.get("TDP_FACTOR_REPLICATE") not in (None, "", "auto"):
            return None
        capture = capture and self._gpu
        sync = torch.cuda.synchronize if self._gpu else (lambda: None)
        from ..train.graph import CapturedStep, try_capture

        # one eager step first, then any pending bucket rebuild: every combination is then timed
        # in the final arena layout (a rebuild inside the first one would skew its time)
        step_fn()
        self.settle()
        # by NAME: arena indices move with a rebuild
        names = [self._param_name(self.arena.params[i]) for i in sorted(self._factor)]
        choices = (True, False, "split") if self._gpu else (True, False)
        modes = list(itertools.product(choices, repeat=len(names))) if len(names) <= 2 \
            else [(c,) * len(names) for c in choices]
        C = native() if self._gpu else None
        cus0 = int(C.reserved_cus()) if C is not None else 0
        cus_list = [int(c) for c in comm_cus] if (comm_cus and C is not None) else [cus0]
        combos = [(m, c) for c in cus_list for m in modes]
        ms = []
        captured = bool(capture)
        for combo, cus in combos:
            if C is not None:
                C.set_reserved_cus(cus)  # planned at capture: each combination re-plans
            self.consolidate_optimizer_state()
            self.factor_replicate = dict(zip(names, combo))
            run = step_fn
            step_fn()  # one eager step in this mode (sizes its buffers)
            if capture:
                run = try_capture(step_fn, warmup=1,
                                  log=lambda m: print(m, file=sys.stderr, flush=True))
                captured = captured and isinstance(run, CapturedStep)
            best_t = None
            for _ in range(repeats):  # min of repeats: one slow window does not decide
                rt.barrier()
                t0 = time.perf_counter()
                for _ in range(iters):
                    run()
                sync()
                t = (time.perf_counter() - t0) * 1000.0 / iters
                best_t = t if best_t is None else min(best_t, t)
            ms.append(best_t)
            if isinstance(run, CapturedStep):
                del run
        t = torch.tensor(ms, dtype=torch.float64, device=self.device)
        rt.all_reduce(t, "max")
        ms = [float(v) for v in t.tolist()]
        best = min(range(len(combos)), key=lambda k: ms[k])
        self.consolidate_optimizer_state()
        self.factor_replicate = dict(zip(names, combos[best][0]))
        if C is not None:
            C.set_reserved_cus(combos[best][1])

        def label(combo):
            return {n: ("replicated" if c is True else "sharded" if c is False else "split")
                    for n, c in zip(names, combo)}
        first = [k for k, (_, c) in enumerate(combos) if c == cus_list[0]]
        self.factor_tuning = {
            "captured": captured,  # every combination timed as a replayed hipGraph
            "timings_ms": [dict({"modes": label(m), "ms": round(t, 4)},
                                **({"comm_cus": c} if len(cus_list) > 1 else {}))
                           for (m, c), t in zip(combos, ms)],
            "chosen": label(combos[best][0]),
            "comm_cus": combos[best][1],
            # the round-3 record's keys: all-replicated / all-sharded times (first CU setting)
            "replicated_ms": round(min(ms[k] for k in first
                                       if combos[k][0] == (True,) * len(names)), 4),
            "sharded_ms": round(min(ms[k] for k in first
                                    if combos[k][0] == (False,) * len(names)), 4),
        }
        return self.factor_replicate

    def consolidate_optimizer_state(self) -> None:
        """Make every rank's fused-optimizer state complete after sharded updates: all-gather
        each bucket's state slices in place (the tails are already replicated)."""
        if not self._fused_shard or self._fused_opt is None:
            return
        opt = self._fused_opt
        bufs = opt._flat_bufs.get(id(self.arena), {})
        W, r = self.world_size, self.rank
        for name, buf in bufs.items():
            if not torch.is_tensor(buf) or buf.numel() != self.arena.numel:
                continue
            fac_of = {b: i for i, b in self._factor_bucket.items()}
            for k in range(len(self._bounds) - 1):
                begin, end = self._bounds[k], self._bounds[k + 1]
                i = fac_of.get(k)
                if i is not None and self._factor_mode.get(i, "").startswith("factored"):
                    # a factored weight's last job: replicated rows are current everywhere,
                    # the sharded ones (past the replicated) on their owners
                    rows = self._factor_rep.get(i, 0)
                    if rows == self._factor[i][0]:
                        continue
                    begin += rows * self._factor[i][1]
                lo, hi = self._backend.owned_shard(begin, end)
                cnt = (hi - lo)
                if cnt > 0:
                    _all_gather_inplace(buf[begin: begin + cnt * W], r, cnt)

    def register_comm_hook(self, state, hook):
        """Gradient compression hooks: torch's bf16_compress_hook (or the string "bf16")."""
        name = hook if isinstance(hook, str) else getattr(hook, "__name__", "")
        if name in ("bf16", "bf16_compress_hook"):
            self._compression = "bf16"
        elif name in ("allreduce_hook", "none", "fp32"):
            self._compression = None
        else:
            raise NotImplementedError(f"comm hook {name!r} is not supported (bf16 | fp32)")
        # rebuilding keeps the fused optimizer's buffers, device block (step count) and flags
        self._build_reducer()

    # --------------------------------------------------------------------------- logging
    def _get_ddp_logging_data(self) -> dict:
        """torch's ``DistributedDataParallel._get_ddp_logging_data`` fields (sampled runtime
        stats in ms instead of ns) plus the reducer's own: head-of-line waits, comm time."""
        b = self._bounds
        esize = self.arena.data.element_size()
        self._collect_samples()
        s = self._samples

        def avg(i):
            v = [x[i] for x in s if x[i] == x[i]]
            return sum(v) / len(v) if v else None
        comm = self.reducer.last_comm_ms()
        return {
            "avg_forward_compute_time_ms": avg(0),
            "avg_backward_compute_time_ms": avg(1),
            "avg_backward_exposed_comm_time_ms": avg(2),
            "sampled_iterations": len(s),
            "head_of_line_waits": int(self.reducer.head_of_line_waits),
            "has_rebuilt_buckets": int(getattr(self, "_rebuilt", False)),
            "world_size": self.world_size,
            "backend_name": rt.get_backend(),
            "bucket_cap_bytes": None,
            "bucket_sizes": [(b[i + 1] - b[i]) * esize for i in range(len(b) - 1)],
            "num_buckets": len(b) - 1,
            "iterations": self._iter,
            "gradient_as_bucket_view": True,
            "find_unused_parameters": self.find_unused_parameters,
            "first_iteration_ready_order": list(self.reducer.ready_order()),
            "avg_backward_comm_time_ms": comm if comm >= 0 else None,
            "grad_compression": self._compression or "none",
        }


def _all_gather_inplace(flat: torch.Tensor, rank: int, cnt: int) -> None:
    """Slice [rank*cnt, (rank+1)*cnt) of ``flat`` from every rank -> everyone, in place."""
    if flat.is_cuda:
        rt.comm().all_gather(flat, flat[rank * cnt: (rank + 1) * cnt])
    else:
        dist.all_gather_into_tensor(flat, flat[rank * cnt: (rank + 1) * cnt].clone())


class _CpuSyncOps:
    """SyncOps (csrc/reducer.h) for CPU arenas: torch.distributed/gloo collectives and torch math.

    The C++ SyncBackend drives it exactly as it drives RcclOps on MI355X, so the gloo tests run
    the production bucket / shard / tail / clip algorithm at any world size. The optimizer math
    mirrors csrc/optim_elem.h (torch's SGD / Adam semantics) and reads its scalars from the same
    hyper-block layout, advanced by opt_begin like opt_step_begin_kernel advances the device one.
    With TDP_POISON_UNOWNED=1 the gradient slices a rank does not own after a reduce-scatter are
    overwritten with NaN, so a test fails if anything reads them."""

    def __init__(self, ddp, compression: int = 0):
        self._ddp = weakref.ref(ddp)
        self.arena = ddp.arena
        self.W, self.r = ddp.world_size, ddp.rank
        self.compression = compression
        self.kind = 0
        self.blk = None
        self.clip_block = None
        self.bufs = {}
        self.factor_bufs = {}  # address -> host all-gather buffer of a factored weight
        self.poison = os.environ.get("TDP_POISON_UNOWNED", "0") == "1"
        if self.poison:
            # alignment gaps between parameters hold no gradient: they must stay zero (no
            # backward ever rewrites them, so NaN left there would leak into later reductions)
            keep = torch.ones(self.arena.numel, dtype=torch.bool)
            for o, n in zip(self.arena.offsets, self.arena.numels):
                keep[o: o + n] = False
            self._gaps = keep.nonzero().flatten()

    def set_fused(self, opt, blk, bufs):
        from ..optim.fused import SGD

        g = opt.param_groups[0]
        self.kind = 1 if isinstance(opt, SGD) else 2
        self.blk, self.bufs = blk, dict(bufs)
        self.flags = dict(nesterov=g.get("nesterov", False), maximize=g["maximize"],
                          amsgrad=g.get("amsgrad", False),
                          decoupled=getattr(opt, "_decoupled", False),
                          momentum=g.get("momentum", 0.0) != 0)

    # collectives (DDP semantics: divide by W, then SUM -- gloo has no AVG)
    def _wire(self, t):
        if self.compression:
            t.copy_(t.bfloat16().float())

    def all_reduce_avg(self, off, n):
        t = self.arena.grad[off: off + n]
        self._wire(t)
        if self.W > 1:
            t.div_(self.W)
            dist.all_reduce(t)

    def reduce_scatter_avg(self, off, cnt):
        W, r = self.W, self.r
        full = self.arena.grad[off: off + W * cnt]
        src = full.div(W)
        out = torch.empty(cnt, dtype=full.dtype)
        dist.reduce_scatter_tensor(out, src)
        full[r * cnt: (r + 1) * cnt].copy_(out)
        if self.poison:
            full[: r * cnt].fill_(float("nan"))
            full[(r + 1) * cnt:].fill_(float("nan"))
            self.arena.grad[self._gaps] = 0.0

    def all_gather_params(self, off, cnt):
        _all_gather_inplace(self.arena.data[off: off + self.W * cnt], self.r, cnt)

    def zero_grads(self, off, n):
        self.arena.grad[off: off + n].zero_()

    # optimizer (csrc/optim_elem.h semantics, scalars from the hyper block)
    def opt_begin(self):
        from ..optim.fused import hyper_slots

        S, b = hyper_slots(), self.blk
        step = int(b.view(torch.int32)[S["step"]]) + 1
        b.view(torch.int32)[S["step"]] = step
        b[S["first"]] = b[S["first_next"]]
        b[S["first_next"]] = 0.0
        b[S["scale"]] = 1.0
        b[S["sumsq"]] = 0.0
        if self.kind == 2:
            b1, b2 = float(b[S["mom"]]), float(b[S["damp"]])
            b[S["bc1"]] = 1.0 - b1 ** step
            b[S["bc2"]] = (1.0 - b2 ** step) ** 0.5

    def opt_update(self, ranges):
        from ..optim.fused import hyper_slots

        S, b, f = hyper_slots(), self.blk, self.flags
        lr, wd, scale = float(b[S["lr"]]), float(b[S["wd"]]), float(b[S["scale"]])
        P, G = self.arena.data, self.arena.grad
        with torch.no_grad():
            for lo, hi in ranges:
                p, g = P[lo:hi], G[lo:hi] * scale
                if f["maximize"]:
                    g = -g
                if self.kind == 1:
                    if wd:
                        g = g.add(p, alpha=wd)
                    if f["momentum"]:
                        mom, damp = float(b[S["mom"]]), float(b[S["damp"]])
                        buf = self.bufs["momentum_buffer"][lo:hi]
                        if float(b[S["first"]]):
                            buf.copy_(g)
                        else:
                            buf.mul_(mom).add_(g, alpha=1 - damp)
                        g = g.add(buf, alpha=mom) if f["nesterov"] else buf
                    p.add_(g, alpha=-lr)
                else:
                    b1, b2, eps = float(b[S["mom"]]), float(b[S["damp"]]), float(b[S["eps"]])
                    bc1, bc2 = float(b[S["bc1"]]), float(b[S["bc2"]])
                    if wd:
                        if f["decoupled"]:
                            p.mul_(1 - lr * wd)
                        else:
                            g = g.add(p, alpha=wd)
                    m, v = self.bufs["exp_avg"][lo:hi], self.bufs["exp_avg_sq"][lo:hi]
                    m.lerp_(g, 1 - b1)
                    v.mul_(b2).addcmul_(g, g, value=1 - b2)
                    vv = v
                    if f["amsgrad"]:
                        vm = self.bufs["max_exp_avg_sq"][lo:hi]
                        torch.maximum(vm, v, out=vm)
                        vv = vm
                    p.addcdiv_(m, vv.sqrt() / bc2 + eps, value=-lr / bc1)

    # factored Linear weights (csrc/reducer.cpp RcclOps::factor_sync, step for step)
    def factor_sync(self, begin, own, cnt, B, out, in_, bias_off, replicate, gptr, xptr):
        g_all, x_all = self.factor_bufs[gptr], self.factor_bufs[xptr]
        W, r = self.W, self.r
        if W > 1:  # in place: this rank's factor rows already sit at slot r
            _all_gather_inplace(g_all, r, B * out)
            _all_gather_inplace(x_all, r, B * in_)
        G, X = g_all.view(W * B, out), x_all.view(W * B, in_)
        with torch.no_grad():
            if bias_off >= 0:
                # the whole averaged bias gradient on every rank: no collective
                self.arena.grad[bias_off: bias_off + out].copy_(G.sum(0))
                self.opt_update([(bias_off, bias_off + out)])
            m0, rows = (own - begin) // in_, cnt // in_
            self.arena.grad[own: own + cnt].copy_((G[:, m0: m0 + rows].t() @ X).reshape(-1))
            if self.poison and not replicate:
                self.arena.grad[begin: own].fill_(float("nan"))
                self.arena.grad[own + cnt: begin + W * cnt].fill_(float("nan"))
        self.opt_update([(own, own + cnt)])
        if not replicate:
            self.all_gather_params(begin, cnt)

    # clipping
    def _block(self, which):
        return self.blk if which == 0 else self.clip_block

    def clip_begin(self, which):
        from ..optim.fused import hyper_slots

        S, b = hyper_slots(), self._block(which)
        b[S["sumsq"]] = 0.0
        b[S["scale"]] = 1.0

    def grad_sumsq(self, which, ranges):
        from ..optim.fused import hyper_slots

        S, b = hyper_slots(), self._block(which)
        G = self.arena.grad
        for lo, hi in ranges:
            b[S["sumsq"]] += G[lo:hi].pow(2).sum()

    def sumsq_all_reduce(self, which):
        from ..optim.fused import hyper_slots

        S, b = hyper_slots(), self._block(which)
        if self.W > 1:
            t = b[S["sumsq"]: S["sumsq"] + 1].clone()
            dist.all_reduce(t)
            b[S["sumsq"]] = t[0]

    def clip_coef(self, which):
        from ..optim.fused import hyper_slots

        S, b = hyper_slots(), self._block(which)
        norm = float(b[S["sumsq"]]) ** 0.5
        b[S["norm"]] = norm
        mx = float(b[S["max_norm"]])
        b[S["scale"]] = min(1.0, mx / (norm + 1e-6)) if mx > 0 else 1.0

    def scale_grads(self, which, ranges):
        from ..optim.fused import hyper_slots

        a = float(self._block(which)[hyper_slots()["scale"]])
        for lo, hi in ranges:
            self.arena.grad[lo:hi].mul_(a)


DDP = DistributedDataParallel
