"""The gradient transport of the native graph engine: the flat gradient buffer cut into
buckets (native_plan.plan_buckets), each all-reduced -- and, with DAMD_BUCKET_OPT, updated --
on a side stream as soon as backward has written it, inside the captured step."""
from __future__ import annotations

import torch

from ..utils import env
from ..utils import logging as dlog
from .native_plan import plan_buckets


class BucketReducer:
    """Chooses and builds the all-reduce transport of ``params.G`` (RCCL, the native xGMI peer
    all-reduce, or the host collective the engine's driver runs) and issues the buckets of a
    backward pass: :meth:`begin`, then :meth:`progress` after every backward op.
    ``norm_clip``: the optimizer's norm-clipping mode, if any (no per-bucket updates then)."""

    def __init__(self, strategy, C, device, params, plan, norm_clip=None):
        self.C, self.device, self.G, self.nparam = C, device, params.G, params.n
        self.world, self.rank = strategy.num_replicas_in_sync, strategy.rank
        dev = device
        force = env.get_bool("DAMD_FORCE_ALLREDUCE", False)  # exercise the RCCL path at world 1
        self.native_comm = strategy.communicator.native if (self.world > 1 or force) else None
        self.peer, self.peers = None, []  # native xGMI peer all-reduce as the bucket transport (set below)
        # DAMD_GRAD_DTYPE=bf16: the RCCL buckets carry bf16 gradients (half the ring traffic;
        # the metric tail stays fp32, the master update fp32); default fp32 (reference parity)
        self.grad_bf16 = env.get_str("DAMD_GRAD_DTYPE", "fp32").lower() == "bf16"
        self.buckets, self._writes = plan_buckets(plan, params.vars, params.sizes, params.offsets, self.G.numel(),
                                                  env.get_float("DAMD_BUCKET_MB", 8.0),
                                                  env.get_float("DAMD_BUCKET_LAST_MB", 1.0))
        for k, b in enumerate(self.buckets):
            b["k"] = k
        # bucket transport at world > 1 (DAMD_ALLREDUCE): RCCL (auto, when the RCCL
        # communicator exists), or the native xGMI peer all-reduce over IPC-mapped staging
        # (xgmi; auto without RCCL, e.g. ranks sharing one GPU in a rehearsal) -- both on the
        # side stream, overlapped with the rest of backward, inside the captured step
        mode = env.get_str("DAMD_ALLREDUCE", "auto").lower()
        if self.world > 1 and (mode == "xgmi" or (mode == "auto" and self.native_comm is None)):
            from ..parallel.communicator import make_peer_allreduce

            from ..utils.watchdog import deadline_for

            wd = deadline_for(self.world)  # in-kernel wait deadline = the watchdog's
            # one peer all-reduce (own IPC-mapped staging, own epochs) PER BUCKET, each on its
            # own side stream: the buckets' all-reduces then need no order among themselves, so
            # in the captured graph each depends on the backward kernels that wrote its bucket
            # only.  (One staging for all = a chain of all-reduce nodes, each with two parents
            # -- the previous all-reduce and the backward -- which the HIP graph executor ran in
            # line with the backward: profiles/r04_resnet18_dp, scripts/probe_graph_branches.py)
            self.peers = []
            for b in self.buckets:
                p = make_peer_allreduce(strategy.communicator, dev.index or 0, b["hi"] - b["lo"],
                                        blocks=env.get_int("DAMD_PEER_BLOCKS", 64), timeout_s=wd if wd > 0 else 60.0)
                if p is None:
                    self.peers = []
                    break
                self.peers.append(p)
            self.peer = self.peers[0] if self.peers else None
            if self.peer is None and mode == "xgmi":
                raise RuntimeError("DAMD_ALLREDUCE=xgmi but the xGMI peer mapping is unavailable")
        if self.peer is not None and self.grad_bf16:
            dlog.warning("DAMD_GRAD_DTYPE=bf16 applies to the RCCL buckets; the peer transport reduces fp32")
            self.grad_bf16 = False
        # RCCL buckets: one communicator PER BUCKET (a unique id each, exchanged over the gloo
        # control plane), each on its own stream.  Collectives on ONE communicator must run
        # in issue order, so a shared communicator forces the captured graph into a chain --
        # each all-reduce node waiting on the previous one AND on its backward -- which the
        # graph executor serialised with the backward (profiles/r05_graph_branches: no
        # overlap for the last buckets).  With a communicator per bucket every all-reduce
        # node depends only on the backward work that wrote its bucket.  DAMD_BUCKET_COMMS=0:
        # the single shared communicator and one comm stream (the round-5 chain).
        self.bucket_comms = []
        if (self.native_comm is not None and self.peer is None and len(self.buckets) > 1
                and env.get_bool("DAMD_BUCKET_COMMS", True)):
            comm = strategy.communicator
            uids = [self.C.rccl_unique_id() for _ in self.buckets] if self.rank == 0 else None
            if self.world > 1:
                uids = comm.broadcast_object(uids, 0)
            self.bucket_comms = [self.C.RcclComm(self.world, self.rank, u, dev.index or 0) for u in uids]
        self.host_collective = self.world > 1 and self.native_comm is None and self.peer is None
        self.allreduce_kind = ("none" if self.native_comm is None and self.peer is None else
                               "xgmi-peer-bucketed" if self.peer is not None else
                               "rccl-bucketed-bf16" if self.grad_bf16 else "rccl-bucketed")
        if self.host_collective:
            self.allreduce_kind = "host-gloo"
        self.g16 = (torch.zeros(self.nparam, dtype=torch.bfloat16, device=dev)
                    if self.grad_bf16 and self.native_comm is not None else None)
        # created up front: no stream creation while a graph is being captured.  One stream
        # per bucket (peer staging or RCCL communicator per bucket); a single comm stream
        # when all buckets share one RCCL communicator (its collectives stay in order)
        per_bucket = self.peer is not None or bool(self.bucket_comms)
        self._comm_stream = (torch.cuda.Stream(dev) if (self.native_comm is not None or self.peer is not None)
                             else None)
        self._comm_streams = [torch.cuda.Stream(dev) for _ in self.buckets] if per_bucket else []
        # the SGD / Adam / RMSprop update of a bucket's variables runs right behind the
        # bucket's all-reduce on its own stream (it overlaps the rest of backward, and only
        # the update of the LAST bucket trails the step; DAMD_BUCKET_OPT=0: one optimizer
        # launch after the join).  The bucket holding the metric tail also does the step's
        # bookkeeping (metric fold, cursor, iterations).
        # (world 1, no all-reduce: off by default -- the 4096-block update launches on side
        # streams took CUs from the backward kernels, measured +170 us per ResNet-18 step;
        # the persistent direct convs need every CU)
        reduce = self.native_comm is not None or self.peer is not None
        self.bucket_opt = (env.get_bool("DAMD_BUCKET_OPT", reduce) and not self.host_collective
                           and len(self.buckets) > 1)
        if self.bucket_opt and norm_clip is not None:
            # a norm needs the whole gradient before the first update: one opt_step after the
            # join, whatever DAMD_BUCKET_OPT says (the last buckets' updates no longer overlap
            # the rest of backward)
            dlog.info("%s: the optimizer update runs once after all gradient buckets (no per-bucket updates)",
                      norm_clip)
            self.bucket_opt = False
        if self.bucket_opt and not self._comm_streams:
            self._comm_streams = [torch.cuda.Stream(dev) for _ in self.buckets]
        # convolution weight gradients on a side stream (DAMD_WGRAD_STREAM): a conv's
        # weight gradient and its backprop-input read the same dy and are independent, so
        # the weight-gradient kernel (+ its split-K reduce) runs beside the backprop-input /
        # BatchNorm-backward chain of the main stream (own workspace); joined before the
        # optimizer, and every bucket all-reduce waits for it
        self.wgrad_stream = torch.cuda.Stream(dev) if env.get_bool("DAMD_WGRAD_STREAM", False) else None

    def begin(self):
        for b in self.buckets:
            b["left"] = set(b["vars"])
            b["sent"] = False

    def _reduce_bucket(self, b, st: int):
        """SUM all-reduce of G[lo:hi] on stream ``st`` by the configured transport."""
        lo, hi = b["lo"], b["hi"]
        gp = self.G.data_ptr()
        comm = self.bucket_comms[b["k"]] if self.bucket_comms else self.native_comm
        if self.peer is not None:
            self.peers[b["k"]].allreduce(gp + 4 * lo, hi - lo, st)
        elif self.g16 is not None:
            n = min(hi, self.nparam) - lo  # the parameter part travels as bf16 ...
            g16 = self.g16.data_ptr() + 2 * lo
            self.C.cast_f32_bf16(gp + 4 * lo, g16, n, st)
            comm.allreduce(g16, g16, n, 1, 0, st)
            self.C.cast_bf16_f32(g16, gp + 4 * lo, n, st)
            if hi > self.nparam:  # ... the metric tail (counts, sums) as fp32
                comm.allreduce(gp + 4 * self.nparam, gp + 4 * self.nparam, hi - self.nparam, 0, 0, st)
        else:
            comm.allreduce(gp + 4 * lo, gp + 4 * lo, hi - lo, 0, 0, st)

    def progress(self, nd, optimizer_step, final=False):
        """Backward op ``nd`` has been enqueued: send every bucket it completed (all-reduce, then
        ``optimizer_step(bucket)`` when the update runs per bucket, on the bucket's stream);
        ``final``: send what is left and join the side streams."""
        reduce = self.native_comm is not None or self.peer is not None
        if not reduce and not self.bucket_opt:
            return
        done = set(self._writes.get(id(nd), ())) if nd is not None else set()
        main = torch.cuda.current_stream(self.device)
        for b in self.buckets:
            if b["sent"]:
                continue
            b["left"] -= done
            if b["left"] and not final:
                continue
            cs = self._comm_streams[b["k"]] if self._comm_streams else self._comm_stream
            cs.wait_stream(main)
            if self.wgrad_stream is not None:
                cs.wait_stream(self.wgrad_stream)
            if reduce:
                self._reduce_bucket(b, cs.cuda_stream)
            if self.bucket_opt:
                with torch.cuda.stream(cs):
                    optimizer_step(b)
            b["sent"] = True
        if final:
            for cs in (self._comm_streams or [self._comm_stream]):
                main.wait_stream(cs)

    def check_peer(self):
        if self.peer is not None and any(p.status() for p in self.peers):
            raise RuntimeError("xGMI peer all-reduce: a wait for a peer timed out (peer missing or wedged)")
