"""StepEngine — one training / validation step of the hot path on one GPU (rank).

Owns the per-shape device workspaces (torch tensors = plumbing for HBM allocations) and
sequences the C-ABI calls on the current HIP stream:

    train:  ultr_dnn_forward -> ultr_<loss> -> ultr_dnn_backward [-> ultr_comm_allreduce (one kernel over xGMI; or
            the process group's all-reduce + ultr_grad_sumsq)] -> ultr_apply_update
    valid:  ultr_dnn_forward -> ultr_ndcg

Nothing here synchronises with the host; the caller decides when to read `scalars`
(the reference's `loss.item()` is the only sync, base_algorithm.py / ipw_rank.py:182).
"""
import ctypes
import os
import random
import time

import numpy as np
import torch

from . import _lib, hip_ops
from .utils import metrics as metrics_mod

ALGOS = {"softmax": _lib.ALGO_SOFTMAX, "dla": _lib.ALGO_DLA, "pairdebias": _lib.ALGO_PAIRDEBIAS,
         "lambdarank": _lib.ALGO_LAMBDARANK, "regem": _lib.ALGO_REGEM, "prs": _lib.ALGO_PRS,
         "pdgd": _lib.ALGO_PDGD, "dbgd": _lib.ALGO_DBGD, "twotower": _lib.ALGO_TWOTOWER, "plrank": _lib.ALGO_PLRANK,
         "affine": _lib.ALGO_AFFINE}


def optimizer_id(name):
    """grad_strategy -> ultr_opt for the engines whose state the learning algorithm sizes with opt_state_floats: 'sgd', 'adam', and
    Adagrad for every other string (the reference's own rule, base_algorithm.py:208-226)."""
    return {"sgd": _lib.OPT_SGD, "adam": _lib.OPT_ADAM}.get(name, _lib.OPT_ADAGRAD)


def opt_state_floats(algo, optimizer, list_size, n_params):
    """Floats of optimizer state (ultr_opt_state_floats; host-only) for an engine algorithm name, a grad_strategy, the list size and
    the parameter count: SGD 0, Adagrad P, Adam 2 P (m | v) and 2 (L + 1) more for DLA's propensity parameters; TwoTower's observation
    tower adds L (Adagrad) / 2 L (Adam) behind the ranker's."""
    u = _lib.UpdateDesc()
    u.algo, u.optimizer, u.list_size, u.n_params = ALGOS[algo], optimizer_id(optimizer), int(list_size), int(n_params)
    n = int(_lib.load().ultr_opt_state_floats(ctypes.byref(u)))
    if n < 0:
        raise ValueError("ultr_opt_state_floats refused algo=%r optimizer=%r list_size=%r n_params=%r" % (algo, optimizer, list_size, n_params))
    return n


def _f32(n, device, zero=False):
    n = max(int(n), 1)
    return (torch.zeros if zero else torch.empty)(n, dtype=torch.float32, device=device)


class StepEngine:
    def __init__(self, shape, batch, list_size, device, algo="softmax", optimizer="ada", learning_rate=0.05,
                 max_gradient_norm=5.0, ranker_loss_weight=1.0, propensity_learning_rate=None, em_step_size=0.05,
                 regulation_p=1.0, sigma=1.0, logits_to_prob="softmax", process_group=None, rng_seed=0, l2_loss=0.0,
                 batch_total=None, comm=None, no_peer_comm=False, cutoff=None, tower_combination="product", mask_padding=True,
                 num_samples=64, gain="linear"):
        if not torch.cuda.is_available():
            raise RuntimeError("ultra_pytorch_amd needs an MI355X/ROCm GPU: there is no CPU fallback")
        self.shape, self.B, self.L, self.device = shape, int(batch), int(list_size), device
        # PDGD: the pairs stop at the cutoff (selection_bias_cutoff); tau rides in sigma (include/ultr_hip.h: ultr_step_args)
        self.cutoff = self.L if cutoff is None else int(cutoff)
        shape.lib.ultr_config_reload()  # the ULTR_* knobs are read when an engine is built, never per step
        self.N = self.B * self.L
        self.algo = algo
        self.sigma = float(sigma)
        self.l2p = 1 if logits_to_prob == "sigmoid" else 0
        if algo == "twotower":
            # the same descriptor field carries TwoTower's combination (bit 0: sum) and mask flag (bit 1): include/ultr_hip.h
            if tower_combination not in ("product", "sum"):
                raise ValueError("tower_combination must be 'product' or 'sum', got %r" % (tower_combination,))
            self.tower_combination, self.mask_padding = tower_combination, bool(mask_padding)
            self.l2p = (_lib.TWOTOWER_SUM if tower_combination == "sum" else 0) | (_lib.TWOTOWER_MASK if mask_padding else 0)
        if algo == "plrank":
            # the sampled Plackett-Luce policy gradient: cutoff (None / 0: the whole list), samples per list and gain ride in the same
            # descriptor field (ULTR_PLRANK_PACK, include/ultr_hip.h); the draw's key is (rng_seed, the step set_draw_step hands in)
            if process_group is not None:
                raise NotImplementedError("PLRank does not train data parallel")
            if gain not in _lib.PLRANK_GAIN:
                raise ValueError("gain must be one of %s, got %r" % (sorted(_lib.PLRANK_GAIN), gain))
            if not 1 <= int(num_samples) <= _lib.PLRANK_MAX_SAMPLES:
                raise ValueError("num_samples must be in 1 .. %d, got %r" % (_lib.PLRANK_MAX_SAMPLES, num_samples))
            self.cutoff = 0 if cutoff is None else max(int(cutoff), 0)
            self.num_samples, self.gain = int(num_samples), gain
            self.l2p = _lib.plrank_pack(self.cutoff, self.num_samples, gain)
        if algo == "affine":
            # the affine-corrected softmax loss: ipw_table carries [alpha(n) | beta(n)]; the PAD-mask flag rides in the descriptor's
            # logits_to_prob (ULTR_AFFINE_MASK, include/ultr_hip.h)
            if process_group is not None:
                raise NotImplementedError("AffineRank does not train data parallel")
            self.mask_padding = bool(mask_padding)
            self.l2p = _lib.AFFINE_MASK if mask_padding else 0
        self.pg = process_group
        self.world = 1 if process_group is None else torch.distributed.get_world_size(process_group)
        self.rank = 0 if process_group is None else torch.distributed.get_rank(process_group)
        # RegressionEM's Bernoulli draw when no uniforms are injected: Philox keyed by (seed, step); every shard gets its own
        # key, otherwise list i of every rank would draw the same uniforms
        self.rng_seed, self.rng_step = (int(rng_seed) + 0x9E3779B1 * self.rank) & 0xFFFFFFFFFFFFFFFF, 0
        # PairDebias' xB factor (base_algorithm.py:242-248) is the GLOBAL batch: shards may be uneven (parallel.shard_bounds),
        # so it is the sum of the local batches, not B * world
        # (`batch_total` given: the caller already agreed on it - learning_algorithm.BaseAlgorithm does, per step, so that a
        # cached engine can never sit on a stale value or enter a collective its peers do not)
        self.batch_total = self.B if batch_total is None else int(batch_total)
        if process_group is not None and batch_total is None:
            cpu_pg = torch.distributed.get_backend(process_group) == "gloo"
            t = torch.tensor([self.B], dtype=torch.int64, device="cpu" if cpu_pg else device)
            torch.distributed.all_reduce(t, group=process_group)
            self.batch_total = int(t.item())
        P, tail = shape.n_params, hip_ops.tail_floats(self.L)
        self.P, self.tail = P, tail
        # the gradient exchange: a communicator handed in by the caller (one per process group, shared by every engine of an
        # algorithm object), or this engine's own
        self.comm, self._own_comm = comm, False
        if process_group is not None and comm is None and not no_peer_comm:
            from . import parallel
            self.comm = parallel.PeerComm.create(process_group, P + tail, device)
            self._own_comm = self.comm is not None
        if self.comm is not None and self.comm.n < P + tail:
            raise ValueError("the shared communicator is too small for this model")
        self._alloc(shape, device)
        self.loss_ws = _f32(hip_ops.loss_workspace_bytes(self.B, self.L) // 4, device, zero=True)
        self.scores = _f32(self.N, device).view(self.B, self.L)
        self.dscores = _f32(self.N, device).view(self.B, self.L)
        self.grads = _f32(P + tail, device, zero=True)
        self.scalars = _f32(16, device, zero=True)
        # step report in HOST-mapped pinned memory (ultr_update_desc::host_scalars): the update kernel's block 0 writes the step
        # scalars, the exchange's status word and - last - the step's sequence number there; read_loss() spins on the sequence
        # number instead of a stream synchronisation + device-to-host copy (the reference's loss.item(): 16-18 us -> one PCIe write)
        self._hs = torch.zeros(16, dtype=torch.float32).pin_memory()
        self._hs_f = self._hs.numpy()
        self._hs_u = self._hs_f.view(np.uint32)
        self._seq = 0
        self._host_report = os.environ.get("ULTR_HOST_REPORT", "1") != "0"
        u = _lib.UpdateDesc()
        u.algo = ALGOS[algo]
        u.optimizer = optimizer_id(optimizer)
        u.list_size = self.L
        u.logits_to_prob = self.l2p
        u.n_params = P
        u.learning_rate = float(learning_rate)
        u.max_gradient_norm = float(max_gradient_norm)
        u.adagrad_eps = _lib.ADAM_EPS if u.optimizer == _lib.OPT_ADAM else 1e-10
        # Adam's step count t is NOT this engine's: engines are cached per (batch, list size) and evicted, the count belongs beside the
        # state tensor.  The owner of the state hands it in before every step (set_opt_step); 0 makes the update launch refuse.
        u.adam_t = 0
        u.ranker_loss_weight = float(ranker_loss_weight)
        plr = propensity_learning_rate
        u.propensity_learning_rate = float(learning_rate if plr is None or plr < 0 else plr)
        u.em_step_size = float(em_step_size)
        u.regulation_p = float(regulation_p)
        u.l2_loss = float(l2_loss)
        u.guard = None
        u.range_flag = None
        u.host_scalars = self._hs.data_ptr() if self._host_report else None
        u.seq = 0
        self.udesc = u
        self._args = None
        self._loss_route = None  # "short" | "long": which loss kernel the pair-walk algorithms run at this list size (_loss_is_long)
        self._cached = (None,) * 8  # the tensor objects behind the pointer fields of self._args (train_step)
        self.next_click_source = None  # a DeviceClickFeed (set per step by the plugin algorithm): its next batch is drawn behind the step

    def _alloc(self, shape, device):
        self.saved = _f32(shape.saved_bytes(self.N) // 4, device)
        self.bwd_ws = _f32(shape.bwd_workspace_bytes(self.N) // 4, device)

    # ---- forward only (validation / DNN.build) -------------------------------------------------
    def forward(self, params, features, n_docs, docids, scores=None, train=False):
        scores = self.scores if scores is None else scores
        hip_ops.dnn_forward(self.shape, params, features, n_docs, docids, self.B, self.L, scores,
                            self.saved if train else None)
        return scores

    # ---- loss stage ------------------------------------------------------------------------------
    def loss(self, labels, aux=None, ipw_table=None, pw=None, uniforms=None, docids=None, n_docs=None):
        B, L = self.B, self.L
        if self.algo == "softmax":
            hip_ops.softmax_ce(self.scores, labels, B, L, self.dscores, self.loss_ws, pw=pw, ipw_table=ipw_table)
        elif self.algo == "dla":
            hip_ops.dla_loss(self.scores, labels, aux, self.l2p, B, L, self.dscores, self.loss_ws)
        elif self.algo in ("pairdebias", "lambdarank", "prs"):
            # the short kernel for every list it takes, the long one only for a list it refuses (the rule of ultr_train_step)
            long_list = self._loss_is_long()
            if self.algo == "pairdebias":
                fn = hip_ops.pairdebias_loss_long if long_list else hip_ops.pairdebias_loss
                fn(self.scores, labels, aux[:L], aux[L:], B, L, self.batch_total, self.dscores, self.loss_ws)
            elif self.algo == "lambdarank":
                fn = hip_ops.lambdarank_loss_long if long_list else hip_ops.lambdarank_loss
                fn(self.scores, labels, aux[:L], aux[L:], self.sigma, B, L, self.dscores, self.loss_ws)
            elif pw is not None:  # a weight per list entry [B, L] (hip_ops.history_pw) instead of the position table
                fn = hip_ops.prs_loss_pw_long if long_list else hip_ops.prs_loss_pw
                fn(self.scores, labels, pw, self.sigma, B, L, self.dscores, self.loss_ws)
            elif ipw_table is None:
                raise ValueError("PRSrank's loss needs the IPW table (ipw_table=) or per-entry weights (pw=)")
            else:
                fn = hip_ops.prs_loss_long if long_list else hip_ops.prs_loss
                fn(self.scores, labels, ipw_table, self.sigma, B, L, self.dscores, self.loss_ws)
        elif self.algo == "pdgd":
            if docids is None or n_docs is None:
                raise ValueError("PDGD's loss needs the docids and n_docs (its PADs)")
            hip_ops.pdgd_loss(self.scores, labels, docids, n_docs, self.sigma, self.cutoff, B, L, self.dscores, self.loss_ws)
        elif self.algo == "regem":
            hip_ops.regem_loss(self.scores, labels, aux, B, L, self.dscores, self.loss_ws, uniforms=uniforms,
                               seed=self.rng_seed, step=self.rng_step)
            self.rng_step += 1
        elif self.algo == "twotower":
            if self.mask_padding and (docids is None or n_docs is None):
                raise ValueError("TwoTower's loss with mask_padding needs the docids and n_docs (its PADs)")
            hip_ops.twotower_loss(self.scores, labels, aux, B, L, self.dscores, self.loss_ws, combination=self.tower_combination,
                                  docids=docids if self.mask_padding else None, n_docs=n_docs if self.mask_padding else 0)
        elif self.algo == "plrank":
            if docids is None or n_docs is None:
                raise ValueError("PLRank's loss needs the docids and n_docs (its PADs)")
            self._loss_is_long()  # (raises for a list beyond the kernel's layout, before anything is launched)
            hip_ops.plrank_loss(self.scores, labels, docids, n_docs, B, L, self.dscores, self.loss_ws, n_samples=self.num_samples,
                                cutoff=self.cutoff, gain=self.gain, seed=self.rng_seed, step=self.rng_step, pw=pw, ipw_table=ipw_table)
        elif self.algo == "affine":
            if ipw_table is None or ipw_table.numel() < 2 or ipw_table.numel() % 2:
                raise ValueError("AffineRank's loss needs its table [alpha(n) | beta(n)] (ipw_table=)")
            if self.mask_padding and (docids is None or n_docs is None):
                raise ValueError("AffineRank's loss with mask_padding needs the docids and n_docs (its PADs)")
            self._loss_is_long()  # (raises for a list beyond the kernel's layout, before anything is launched)
            n = ipw_table.numel() // 2
            hip_ops.affine_loss(self.scores, labels, ipw_table[:n], ipw_table[n:], B, L, self.dscores, self.loss_ws,
                                docids=docids if self.mask_padding else None, n_docs=n_docs if self.mask_padding else 0)
        else:
            raise ValueError(self.algo)

    def set_draw_step(self, step):
        """PLRank: the step of the key (rng_seed, step) the NEXT train_step / loss draws its rankings under.  As Adam's t it is counted
        by the owner of the model, not here: engines are cached per (batch, list size) and evicted, a count of theirs would replay
        samples."""
        self.rng_step = int(step)

    def _loss_is_long(self):
        """hip_ops.loss_route of this engine's algorithm and list size, asked once (raises for a list neither kernel takes)."""
        if self._loss_route is None:
            self._loss_route = hip_ops.loss_route(ALGOS[self.algo], self.L)
        return self._loss_route == "long"

    def backward(self, params, features, n_docs, docids):
        hip_ops.dnn_backward(self.shape, params, features, n_docs, docids, self.B, self.L, self.saved, self.dscores,
                             self.loss_ws, self.bwd_ws, self.grads)
        self.dp_reduce()

    def dp_reduce(self):
        """Queries shard across ranks: ONE sum of [grads | step tail] per step, then the sum-of-squares partials of the
        reduced gradient for the clip."""
        if self.pg is None:
            return
        if self.comm is not None:  # one kernel: publish, xGMI reads of every peer, fixed-order sum, partials
            self.comm.allreduce(self.grads, self.P + self.tail, self.P, self.grads, self.bwd_ws)
        else:  # the process group's collective (RCCL over xGMI; gloo in tests)
            torch.distributed.all_reduce(self.grads, group=self.pg)
            hip_ops.grad_sumsq(self.grads, self.P, self.L, self.bwd_ws)

    def update(self, params, state, aux=None):
        hip_ops.apply_update(self.shape, self.udesc, params, state, self.grads, aux, self.bwd_ws, self.scalars)

    def _next_seq(self):
        self._seq = (self._seq % 0xFFFFFFFF) + 1  # 1 .. 2^32-1: never 0, the buffer's initial content
        self.udesc.seq = self._seq

    def set_opt_step(self, t):
        """The step count t >= 1 the NEXT train_step / update applies to `state` (ultr_update_desc::adam_t; read by Adam only).  The
        caller counts it beside the state tensor, one count per state, whichever engine a step runs in."""
        self.udesc.adam_t = min(int(t), 0xFFFFFFFF)  # (beyond 2^32 - 1 steps both bias corrections are 1 anyway)

    def read_scalars(self, timeout_s=60.0, scheduled=False):
        """The step scalars of the LAST queued step as a numpy array ([0] loss, [1] gradient norm, [2] clip coefficient, [3] D,
        [4] rank_loss, [5] exam_loss, [6] propensity gradient norm, [7] sum g^2) - the reference's `loss.item()`.  Waits for the
        update kernel's report in host-mapped memory (no stream synchronisation); raises if the gradient exchange of a
        data-parallel step timed out on any rank (the update was then NOT applied, ultr_update_desc::guard)."""
        if not self._host_report:
            torch.cuda.current_stream().synchronize()
            if self.comm is not None and self.comm.status() != 0:
                raise _lib.UltrHipError("data-parallel gradient exchange timed out (ULTR_E_COMM_TIMEOUT): the update was not applied")
            return self.scalars[:8].cpu().numpy()
        seq, u, spins, t0 = self._seq, self._hs_u, 0, None
        if seq == 0:
            raise RuntimeError("read_scalars() before the first train_step()")
        while int(u[9]) != seq:
            spins += 1
            if spins & 0x3FF == 0:  # look at the clock every 1024 polls only
                now = time.perf_counter()
                t0 = now if t0 is None else t0
                if now - t0 > timeout_s:
                    raise _lib.UltrHipError("no step report from the GPU within %.0f s (step %d)" % (timeout_s, seq))
        self._raise_on_status(int(u[8]), scheduled)
        return self._hs_f[:8].copy()

    H3_RANGE, H3_NEAR = 0x100, 0x200  # include/ultr_hip.h: ULTR_STATUS_H3_RANGE / ULTR_STATUS_H3_NEAR

    DP_STATUS_CADENCE = 64  # data parallel: every rank examines the step report of the same steps (train_step)

    def _raise_on_status(self, st, scheduled=False):
        """Act on the status word of the latest full step report (host_scalars[8]).
        Data parallel: the switch to the fp32 products changes the bits of the following steps, so every rank must make it at the
        SAME step.  The replicas are bit-identical, hence every rank's update kernel raises the NEAR bit in the report of the same
        step - but ranks read reports when their callers ask for a loss (rank 0 may log every step, the others never).  There the
        switch is only made from train_step's own scheduled look at the report (every DP_STATUS_CADENCE-th step, on every rank
        alike: ADVICE r05); a read in between leaves the NEAR bit alone (the copies are still exact: one step moves a weight by at
        most lr x the clip norm, 64 steps by far less than the 64 .. 128 margin)."""
        if st == 0:
            return
        if self.pg is not None and not scheduled:
            st &= ~self.H3_NEAR
            if st == 0:
                return
        if st & (self.H3_RANGE | self.H3_NEAR):
            # a hidden weight is near (>= 64) or beyond (>= 128) the range of the split-half weight copies.  Near: every copy is
            # still exact and one optimizer step moves a weight by at most lr x the clip norm - switch to the fp32 products now
            # and go on, as the reference would (base_algorithm.py:208-226 trains any weight magnitude).  Beyond, with the
            # split-half products still on: some step already read an overflowed copy.
            switched = hip_ops.fall_back_to_fp32_products(self.shape, "a hidden weight reached |w| >= 64 during training (the "
                                                          "split-half weight copies cover |w| < 128)")
            if (st & self.H3_RANGE) and switched:
                raise _lib.UltrHipError("a hidden weight jumped to |w| >= 128 within the steps between two reads of the step report, "
                                        "outside the range of the split-half (fp16 hi / lo) weight copies (ULTR_STATUS_H3_RANGE): the "
                                        "last steps are not to be trusted - restart from the last checkpoint (this model is on the fp32 "
                                        "matrix-core products now: ULTR_MODEL_FP32_PRODUCTS)")
            st &= ~(self.H3_RANGE | self.H3_NEAR)
            if st == 0:
                return
        raise _lib.UltrHipError("data-parallel gradient exchange timed out on some rank (ULTR_E_COMM_TIMEOUT): this and all "
                                "later updates were NOT applied - restart from the last checkpoint")

    def read_loss(self, timeout_s=60.0):
        """The loss of the last queued step (the reference's `loss.item()`).  Returns as soon as the loss is FINAL: on one GPU
        that is behind forward + loss (the weight-gradient launch reports it, include/ultr_hip.h: host_scalars[10]), while the
        step's reduction and update are still running - later work simply queues behind them on the stream.  The status word
        of the LATEST full report is examined on every call (it is one or two launches older than the loss: a failure -
        exchange timeout, split-half range - surfaces one step late at most; both conditions are sticky on the device)."""
        if not self._host_report:
            return float(self.read_scalars()[0])
        seq, u, spins, t0 = self._seq, self._hs_u, 0, None
        if seq == 0:
            raise RuntimeError("read_loss() before the first train_step()")
        while int(u[10]) != seq:
            spins += 1
            if spins & 0x3FF == 0:
                now = time.perf_counter()
                t0 = now if t0 is None else t0
                if now - t0 > timeout_s:
                    raise _lib.UltrHipError("no loss report from the GPU within %.0f s (step %d)" % (timeout_s, seq))
        self._raise_on_status(int(u[8]))
        return float(self._hs_f[0])

    def close(self):
        if self._own_comm and self.comm is not None:
            self.comm.close()
        self.comm = None

    def train_step(self, params, state, features, n_docs, docids, labels, aux=None, ipw_table=None, pw=None,
                   uniforms=None):
        """One full step through ONE C call (ultr_train_step); returns the device tensor of step scalars ([0] = loss)."""
        a = self._args
        if a is None:
            a = self._args = _lib.StepArgs()
            a.desc = ctypes.pointer(self.shape.desc)
            a.upd = ctypes.pointer(self.udesc)
            a.scores, a.dscores = self.scores.data_ptr(), self.dscores.data_ptr()
            a.saved, a.loss_ws, a.bwd_ws = self.saved.data_ptr(), self.loss_ws.data_ptr(), self.bwd_ws.data_ptr()
            a.grads, a.scalars = self.grads.data_ptr(), self.scalars.data_ptr()
            a.batch, a.list_size = self.B, self.L
            a.sigma = self.sigma
            # data parallel: with the peer exchange the whole sharded step is still ONE C call (backward -> exchange kernel ->
            # update); with the process group's all-reduce the call stops behind the backward and the host issues the rest
            a.skip_update = 1 if (self.pg is not None and self.comm is None) else 0
            a.comm = self.comm.h if self.comm is not None else None
            self._fn = self.shape.lib.ultr_train_step
            self._fn_feed = self.shape.lib.ultr_feed_train_step
            self._aref = ctypes.byref(a)
        a.batch_total = self.batch_total  # per step: uneven data-parallel shards may change it (PairDebias' xB factor)
        # pointer fields are rewritten only when the tensor OBJECT behind them changed (a ctypes field store + data_ptr() is ~0.3 us;
        # the same parameters / state / feature matrix / table come back every step, only the batch tensors alternate)
        c = self._cached
        a.params = params.data_ptr()  # (always: `.data = ...` re-seats a tensor object's storage)
        a.wt = hip_ops.weight_copy(self.shape).get(params).data_ptr()
        a.state = state.data_ptr() if state is not None else None
        if aux is not c[2]:
            a.aux = aux.data_ptr() if aux is not None else None
        if features is not c[3] or n_docs != a.n_docs:
            a.features = features.data_ptr() if n_docs > 0 else None
            a.n_docs = n_docs
        if docids is not c[4]:
            a.docids = docids.data_ptr()
        if labels is not c[5]:
            a.labels = labels.data_ptr()
        if pw is not c[6]:
            a.pw = pw.data_ptr() if pw is not None else None
        if ipw_table is not c[7]:
            a.ipw_table = ipw_table.data_ptr() if ipw_table is not None else None
            a.n_ipw = int(ipw_table.numel()) if ipw_table is not None else 0
            if self.algo == "affine":  # [alpha(n) | beta(n)]: the entry's n
                a.n_ipw //= 2
        if self.algo == "pdgd":
            a.n_ipw = self.cutoff
        self._cached = (params, state, aux, features, docids, labels, pw, ipw_table)
        if self.algo == "regem":
            a.uniforms = uniforms.data_ptr() if uniforms is not None else None
            a.rng_seed, a.rng_step = self.rng_seed, self.rng_step
            self.rng_step += 1
        elif self.algo == "plrank":
            a.rng_seed, a.rng_step = self.rng_seed, self.rng_step  # (set_draw_step: the owner counts)
        if self.comm is not None:
            a.comm_step = self.comm.step
            self.comm.step += 1
        if self.pg is not None and self._host_report and self._seq > 0 and self._seq % self.DP_STATUS_CADENCE == 0:
            self.read_scalars(scheduled=True)  # the same step on every rank: a switch to the fp32 products happens everywhere at once
        self._next_seq()
        src = self.next_click_source
        nxt = src.next_click_args() if src is not None else None
        if nxt is not None and a.skip_update == 0:
            rc = self._fn_feed(self._aref, nxt, hip_ops.raw_stream())
        else:
            rc = self._fn(self._aref, hip_ops.raw_stream())
            if nxt is not None and rc == 0:  # (process-group path: the draw follows the step's first half)
                rc = self.shape.lib.ultr_click_batch_args(nxt, hip_ops.raw_stream())
        if rc != 0:
            _lib.check(rc, "ultr_train_step")
        if self.pg is not None and self.comm is None:
            self.dp_reduce()
            self.update(params, state, aux)
        return self.scalars


# ULTR_METRIC_* (include/ultr_hip.h) by RankingMetricKey
METRIC_IDS = {"ndcg": 0, "dcg": 1, "mrr": 2, "err": 3, "map": 4, "arp": 5, "precision": 6, "ordered_pair_accuracy": 7}
_METRICS_SEQ_WORD = 8 * 16  # ultr_metrics_report's sequence word in the host report (ultr_ndcg_report's is 16)


def _metric_ids(metrics):
    """The ULTR_METRIC_* ids of a tuple of distinct RankingMetricKey names, as the metric launch takes them."""
    unknown = [m for m in metrics if m not in METRIC_IDS]
    if unknown or len(set(metrics)) != len(metrics) or not metrics:
        raise ValueError("metrics must be distinct keys of %s, got %r" % (sorted(METRIC_IDS), metrics))
    return (ctypes.c_int32 * len(metrics))(*[METRIC_IDS[m] for m in metrics])


def _wait_report(u, word, seq, timeout_s, noun):
    """Spin until word `word` of a report in host-mapped memory (u: its uint32 view) carries the launch's sequence number."""
    spins, t0 = 0, None
    while int(u[word]) != seq:
        spins += 1
        if spins & 0x3FF == 0:
            now = time.perf_counter()
            t0 = now if t0 is None else t0
            if now - t0 > timeout_s:
                raise _lib.UltrHipError("no %s report from the GPU within %.0f s" % (noun, timeout_s))


def metrics_fit_short(list_size):
    """Whether the metric launch's kernel of one wave per list takes this list size (csrc/ultr_metrics.hip ndcg_lds_bytes: 64 KiB of LDS
    for four lists) - the routing threshold of ultr_metrics_report, 813 documents."""
    L = int(list_size)
    return (4 * 5 * L + 4 * 2 * ((L + 63) // 64) + 4) * 4 <= 64 * 1024


def ndcg_fit(list_size):
    """Whether ultr_ndcg_report / ultr_dnn_forward_ndcg take this list size (four arrays per list: 1023 documents)."""
    return (4 * 4 * int(list_size) + 4) * 4 <= 64 * 1024


def metrics_fit(list_size):
    """Whether the metric launch (ultr_metrics_report) takes this list size, with either of its kernels: up to ultr_metrics_max_list()."""
    return 1 <= int(list_size) <= int(_lib.load().ultr_metrics_max_list())


class EvalEngine:
    """validation(): forward at max_candidate_num + padding mask + NDCG@topn; with metrics other than ("ndcg",) every requested metric
    of utils.metrics in the same launch (ultr_metrics_report), read with read_metrics()."""

    def __init__(self, shape, batch, list_size, device, topn=(1, 3, 5, 10), metrics=("ndcg",)):
        if not torch.cuda.is_available():
            raise RuntimeError("ultra_pytorch_amd needs an MI355X/ROCm GPU: there is no CPU fallback")
        self.shape, self.B, self.L, self.device = shape, int(batch), int(list_size), device
        self.topn = [int(t) for t in topn]
        self.scores = _f32(self.B * self.L, device).view(self.B, self.L)
        self.masked = _f32(self.B * self.L, device).view(self.B, self.L)
        self.order = torch.empty(self.B, self.L, dtype=torch.int32, device=device)
        self.ndcg = _f32(len(self.topn), device)
        self.ndcg_ws = _f32(self.B * len(self.topn), device)
        # the metric vector in HOST-mapped pinned memory + a sequence word (ultr_ndcg_report): read_ndcg() spins on the word instead
        # of a stream synchronisation + device-to-host copy per validation batch
        self._counter = torch.zeros(1, dtype=torch.int32, device=device)
        self._hs = torch.zeros(32, dtype=torch.float32).pin_memory()
        self._hs_f = self._hs.numpy()
        self._hs_u = self._hs_f.view(np.uint32)
        self._seq = 0
        self._topn_arr = (ctypes.c_int32 * len(self.topn))(*self.topn)
        self._lib = shape.lib
        self.metrics = tuple(metrics)
        # ("ndcg",) beyond the NDCG launch's 1023 documents: the metric launch with the one id (the same arithmetic in the same order)
        self._all = self.metrics != ("ndcg",) or not ndcg_fit(self.L)
        if self._all:
            self._ids_arr = _metric_ids(self.metrics)
            nm, nt = len(self.metrics), len(self.topn)
            self.metric_out = _f32(nm * nt, device).view(nm, nt)  # batch means, a row per metric in the order asked
            self.metric_ws = _f32(self.B * nm * nt, device).view(self.B, nm, nt)  # per-list values
            # (self.ndcg / self.ndcg_ws stay allocated; the NDCG row of this path is metric_out's)
            self.ndcg = self.metric_out[self.metrics.index("ndcg")] if "ndcg" in self.metrics else None
            self._hs = torch.zeros(_METRICS_SEQ_WORD + 32, dtype=torch.float32).pin_memory()
            self._hs_f = self._hs.numpy()
            self._hs_u = self._hs_f.view(np.uint32)

    @staticmethod
    def _max_label():
        """RankingMetricKey.MAX_LABEL is set by the data loader, possibly after this engine was built: read at every run()."""
        ml = metrics_mod.RankingMetricKey.MAX_LABEL
        return 4.0 if ml is None else float(ml)

    def _launch_tail(self):
        """The next launch's sequence number taken, the arguments every entry of this engine's path ends with - from the cutoffs to the
        stream: the metric launch's (ultr_metrics_report, ultr_dnn_forward_metrics) or the NDCG launch's (ultr_ndcg_report,
        ultr_dnn_forward_ndcg)."""
        self._seq = (self._seq % 0xFFFFFFFF) + 1
        if self._all:
            outs = (self._ids_arr, len(self.metrics), self._max_label(), self.metric_out.data_ptr(), self.order.data_ptr(),
                    self.masked.data_ptr(), self.metric_ws.data_ptr())
        else:
            outs = (self.ndcg.data_ptr(), self.order.data_ptr(), self.masked.data_ptr(), self.ndcg_ws.data_ptr())
        return (self._topn_arr, len(self.topn)) + outs + (self._counter.data_ptr(), self._hs.data_ptr(), self._seq, hip_ops.raw_stream())

    def _ndcg(self, labels, docids, n_docs):
        """The metric launch alone, on self.scores."""
        name = "ultr_metrics_report" if self._all else "ultr_ndcg_report"
        _lib.check(getattr(self._lib, name)(self.scores.data_ptr(), labels.data_ptr(), docids.data_ptr(), int(n_docs), self.B, self.L,
                                            *self._launch_tail()), name)

    def run(self, params, features, n_docs, docids, labels):
        """ONE host call (ultr_dnn_forward_ndcg): the forward, then the metric launch with its report in host-mapped memory."""
        name = "ultr_dnn_forward_metrics" if self._all else "ultr_dnn_forward_ndcg"
        wt = hip_ops.weight_copy(self.shape).get(params)
        _lib.check(getattr(self._lib, name)(ctypes.byref(self.shape.desc), params.data_ptr(), wt.data_ptr() if wt is not None else None,
                                            features.data_ptr() if n_docs > 0 else None, int(n_docs), docids.data_ptr(), labels.data_ptr(),
                                            self.B, self.L, self.scores.data_ptr(), *self._launch_tail()), name)
        return self.scores, self.ndcg

    def forward(self, params, features, n_docs, docids):
        """The forward alone into self.scores - for a list no metric launch takes (validation() then computes on the host)."""
        hip_ops.dnn_forward(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores)
        return self.scores

    def read_ndcg(self, timeout_s=60.0):
        """NDCG@topn of the LAST run() as a numpy array - the reference's `.item()` per metric (ipw_rank.py:204-210) without a stream
        synchronisation: waits for the launch's report in host-mapped memory."""
        if self._all:
            if "ndcg" not in self.metrics:
                raise RuntimeError("read_ndcg() of an engine built without the ndcg metric")
            return self.read_metrics(timeout_s)["ndcg"]
        self._wait_report(16, timeout_s)
        return self._hs_f[:len(self.topn)].copy()

    def _wait_report(self, word, timeout_s):
        if self._seq == 0:
            raise RuntimeError("read_ndcg() before the first run()")
        _wait_report(self._hs_u, word, self._seq, timeout_s, "NDCG")

    def read_metrics(self, timeout_s=60.0):
        """{metric: values per cutoff} of the LAST run(), from the launch's report in host-mapped memory (no stream synchronisation)."""
        if not self._all:
            return {"ndcg": self.read_ndcg(timeout_s)}
        self._wait_report(_METRICS_SEQ_WORD, timeout_s)
        nt = len(self.topn)
        vals = self._hs_f[:len(self.metrics) * nt].copy()
        return {m: vals[k * nt:(k + 1) * nt] for k, m in enumerate(self.metrics)}


class EvalSetEngine:
    """A whole validation / test set from a ResidentDataset without returning to the host between batches (csrc/ultr_eval.hip): per
    chunk of `batch` queries (the last one short) the sequential pick, the launches validation() issues for that batch and the
    accumulate in double - utils.merge_Summary operation for operation - then ONE host read of the merged report.

    A DNN / Linear model runs the chunks from one C call (ultr_dnn_eval_set).  A model with another eval engine (SetRank) runs the same
    three stages per chunk from Python: ultr_eval_pick, that engine's run() without reading its report, ultr_eval_accumulate."""

    def __init__(self, shape, batch, list_size, device, topn=(1, 3, 5, 10), metrics=("ndcg",), eval_engine_cls=None):
        if not torch.cuda.is_available():
            raise RuntimeError("ultra_pytorch_amd needs an MI355X/ROCm GPU: there is no CPU fallback")
        self.shape, self.B, self.L, self.device = shape, int(batch), int(list_size), device
        self.topn, self.metrics = [int(t) for t in topn], tuple(metrics)
        self._ids_arr = _metric_ids(self.metrics)
        if not metrics_fit(self.L):
            raise ValueError("list size %d is beyond the metric launch's bound (engine.metrics_fit)" % self.L)
        self._lib = shape.lib
        B, L, nm, nt = self.B, self.L, len(self.metrics), len(self.topn)
        self.n_values = nm * nt
        self._cls = eval_engine_cls if eval_engine_cls not in (None, EvalEngine) else None
        self.acc = torch.zeros(self.n_values + 1, dtype=torch.float64, device=device)
        # the merged report in HOST-mapped pinned memory: 128 values, the summed weights, the sequence word (ULTR_EVAL_SEQ_BYTE)
        self._hs = torch.zeros(_lib.EVAL_SEQ_BYTE // 8 + 1, dtype=torch.float64).pin_memory()
        self._hs_d = self._hs.numpy()
        self._hs_u = self._hs_d.view(np.uint32)
        self._seq = 0
        self.docids = torch.empty(L, B, dtype=torch.int32, device=device)
        self.labels = torch.empty(L, B, dtype=torch.float32, device=device)
        self.scores_all = self.per_query = None
        self.n_queries = 0
        if self._cls is None:
            self._topn_arr = (ctypes.c_int32 * nt)(*self.topn)
            self.scores = _f32(B * L, device).view(B, L)
            self.masked = _f32(B * L, device).view(B, L)
            self.order = torch.empty(B, L, dtype=torch.int32, device=device)
            self.metric_out = _f32(nm * nt, device).view(nm, nt)
            self.metric_ws = _f32(B * nm * nt, device).view(B, nm, nt)
            self._counter = torch.zeros(1, dtype=torch.int32, device=device)
        else:
            self._engines = {}  # chunk size -> the model's own eval engine (the full chunk and the short last one)

    def _chunk_engine(self, b):
        ev = self._engines.get(b)
        if ev is None:
            ev = self._engines[b] = self._cls(self.shape, b, self.L, self.device, topn=self.topn, metrics=self.metrics)
        return ev

    def _outputs(self, n_queries, want_scores, per_query):
        nm, nt = len(self.metrics), len(self.topn)
        if want_scores and (self.scores_all is None or self.scores_all.shape[0] != n_queries):
            self.scores_all = _f32(n_queries * self.L, self.device).view(n_queries, self.L)
        if per_query and (self.per_query is None or self.per_query.shape[0] != n_queries):
            self.per_query = _f32(n_queries * nm * nt, self.device).view(n_queries, nm, nt)
        return (self.scores_all if want_scores else None), (self.per_query if per_query else None)

    def run(self, params, resident, want_scores=False, per_query=False):
        """Queue the whole set on the current stream; read() waits for the report.  want_scores / per_query: keep every query's scores
        [n_queries, L] / per-list metric values [n_queries, n_metrics, n_topn] on the device (self.scores_all / self.per_query)."""
        rd, st = resident, hip_ops.raw_stream()
        nq = self.n_queries = int(rd.n_queries)
        sa, pq = self._outputs(nq, want_scores, per_query)
        self._seq = (self._seq % 0xFFFFFFFF) + 1
        feats = rd.features.data_ptr() if rd.n_docs > 0 else None
        if self._cls is None:
            wt = hip_ops.weight_copy(self.shape).get(params)
            _lib.check(self._lib.ultr_dnn_eval_set(
                ctypes.byref(self.shape.desc), params.data_ptr(), wt.data_ptr() if wt is not None else None, feats, rd.n_docs,
                rd.lists.data_ptr(), rd.labels.data_ptr(), nq, rd.lmax, self.B, self.L, self._topn_arr, len(self.topn), self._ids_arr,
                len(self.metrics), EvalEngine._max_label(), self.docids.data_ptr(), self.labels.data_ptr(), self.scores.data_ptr(),
                self.metric_out.data_ptr(), self.order.data_ptr(), self.masked.data_ptr(), self.metric_ws.data_ptr(),
                self._counter.data_ptr(), sa.data_ptr() if sa is not None else None, pq.data_ptr() if pq is not None else None,
                self.acc.data_ptr(), self._hs.data_ptr(), self._seq, st), "ultr_dnn_eval_set")
            return
        nm, nt = len(self.metrics), len(self.topn)
        for start in range(0, nq, self.B):
            b = min(self.B, nq - start)
            ids, lab = self.docids.view(-1)[:self.L * b].view(self.L, b), self.labels.view(-1)[:self.L * b].view(self.L, b)
            _lib.check(self._lib.ultr_eval_pick(rd.lists.data_ptr(), rd.labels.data_ptr(), nq, rd.lmax, rd.n_docs, start, b, self.L,
                                                ids.data_ptr(), lab.data_ptr(), None, st), "ultr_eval_pick")
            ev = self._chunk_engine(b)
            scores, _ = ev.run(params, rd.features, rd.n_docs, ids, lab)
            means = ev.metric_out if ev._all else ev.ndcg
            if sa is not None:
                sa[start:start + b].copy_(scores)
            if pq is not None:
                pq[start:start + b].copy_((ev.metric_ws if ev._all else ev.ndcg_ws).view(b, nm, nt))
            flags = (_lib.EVAL_RESET if start == 0 else 0) | (_lib.EVAL_FINISH if start + b >= nq else 0)
            _lib.check(self._lib.ultr_eval_accumulate(means.data_ptr(), self.n_values, b, self.acc.data_ptr(), flags, self._hs.data_ptr(),
                                                      self._seq, st), "ultr_eval_accumulate")

    def read(self, timeout_s=60.0):
        """{metric: float64 [n_topn]} of the LAST run(), merged over the set - from the report in host-mapped memory."""
        if self._seq == 0:
            raise RuntimeError("read() before the first run()")
        _wait_report(self._hs_u, _lib.EVAL_SEQ_BYTE // 4, self._seq, timeout_s, "evaluation")
        nt = len(self.topn)
        vals = self._hs_d[:self.n_values].copy()
        return {m: vals[k * nt:(k + 1) * nt] for k, m in enumerate(self.metrics)}


def _setrank_draw(list_size):
    """The reference's SetRank.build shuffles an index list on EVERY forward and never uses it (SetRank.py:245-246), but the
    call advances Python's global `random` stream - the one ClickSimulationFeed draws queries and clicks from.  Consuming
    the same draws keeps a seeded SetRank run on the reference's batches and clicks."""
    random.shuffle(list(range(int(list_size))))


class StagedStepEngine(StepEngine):
    """A step issued as stage calls instead of ONE C call, for the ranking models whose forward and backward are entries of their own
    (SetRank, DLCM, GSF): forward(train=True) -> loss -> backward -> ultr_apply_update on the flat vector (no k-major weight copy).  At
    their size (hundreds of microseconds to milliseconds per step) the host is not on the critical path.  A subclass supplies _alloc,
    forward and backward (which leaves the sum-of-squares partials in self.bwd_ws)."""

    def _sumsq_floats(self):
        """Floats of self.bwd_ws: the sum-of-squares partials of ultr_grad_sumsq / ultr_apply_update."""
        return (self.P + self.tail + 63) // 64 + self.P // 4096 + 16

    def _range_flag(self):
        """Device address of the model's split-half range word (ultr_update_desc::range_flag), None: it builds no such planes."""
        return None

    def update(self, params, state, aux=None):
        check = _lib.check
        self.udesc.range_flag = self._range_flag()
        check(self.shape.lib.ultr_apply_update(ctypes.byref(self.udesc), None, ctypes.c_void_p(params.data_ptr()), None,
                                               ctypes.c_void_p(state.data_ptr()) if state is not None else None,
                                               ctypes.c_void_p(self.grads.data_ptr()),
                                               ctypes.c_void_p(aux.data_ptr()) if aux is not None else None,
                                               ctypes.c_void_p(self.bwd_ws.data_ptr()), ctypes.c_void_p(self.scalars.data_ptr()),
                                               hip_ops.raw_stream()), "ultr_apply_update")

    def train_step(self, params, state, features, n_docs, docids, labels, aux=None, ipw_table=None, pw=None, uniforms=None):
        self._next_seq()
        self.forward(params, features, n_docs, docids, train=True)
        if self.algo == "regem":
            self.loss(labels, aux=aux, uniforms=uniforms)
        else:
            self.loss(labels, aux=aux, ipw_table=ipw_table, pw=pw, docids=docids, n_docs=n_docs)
        self.backward(params, features, n_docs, docids)
        self.update(params, state, aux)
        src = self.next_click_source
        nxt = src.next_click_args() if src is not None else None
        if nxt is not None:
            _lib.check(self.shape.lib.ultr_click_batch_args(nxt, hip_ops.raw_stream()), "ultr_click_batch")
        return self.scalars


class SetRankStepEngine(StagedStepEngine):
    """The same step for the SetRank ranking model: ultr_setrank_forward -> ultr_<loss> ->
    ultr_setrank_backward -> [all-reduce] -> ultr_grad_sumsq -> ultr_apply_update, as stage calls (StagedStepEngine).

    Dropout (shape.rate > 0): forward(train=True) takes the model's next dropout step (shape.next_dropout_step()) and passes
    (rate, shape.dropout_seed, step, dropout_stream) to ultr_setrank_forward_dropout; backward() hands the same struct, with the
    extra scratch, to ultr_setrank_backward_dropout.  dropout_stream is the data-parallel rank: replicas drop different elements of
    their different shards.  forward(train=False) never drops."""

    def __init__(self, shape, batch, list_size, device, **kw):
        self._sr_shape = shape
        super().__init__(shape, batch, list_size, device, **kw)

    def _alloc(self, shape, device):
        self.saved = _f32(shape.saved_bytes(self.N) // 4, device)
        self.sr_ws = _f32(shape.workspace_bytes(self.N) // 4, device)
        self.bwd_ws = _f32(self._sumsq_floats(), device)
        self._flag_off = shape.range_flag_offset(self.N)
        self.saved[self._flag_off].zero_()  # (every forward zeroes it again: this is for a report before the first forward)
        self.dropout_stream = self.rank
        self.drop_ws = None  # the backward's extra buffer of a dropout step, allocated by the first one
        self._drop = None    # ultr_setrank_dropout of the forward in flight (None: a plain step)

    def forward(self, params, features, n_docs, docids, scores=None, train=False):
        scores = self.scores if scores is None else scores
        _setrank_draw(self.L)
        self._drop = None
        if train and getattr(self.shape, "rate", 0.0) > 0.0:
            if self.drop_ws is None:
                self.drop_ws = _f32(self.shape.dropout_workspace_bytes(self.N) // 4, self.device)
            self._drop = hip_ops.setrank_dropout(self.shape.rate, self.shape.dropout_seed, self.shape.next_dropout_step(),
                                                 self.dropout_stream, self.drop_ws)
        hip_ops.setrank_forward(self.shape, params, features, n_docs, docids, self.B, self.L, scores, self.saved, dropout=self._drop)
        return scores

    def backward(self, params, features, n_docs, docids):
        hip_ops.setrank_backward(self.shape, params, self.B, self.L, self.saved, self.dscores, self.loss_ws, hip_ops.loss_part_count(self.B),
                                 self.sr_ws, self.grads, dropout=self._drop)
        if self.pg is not None:
            self.dp_reduce()
        else:
            hip_ops.grad_sumsq(self.grads, self.P, self.L, self.bwd_ws)

    def _range_flag(self):
        # the range word of this step's split-half planes (raised by ultr_setrank_forward) travels in the step report
        return self.saved.data_ptr() + 4 * self._flag_off


class SetRankEvalEngine(EvalEngine):
    def __init__(self, shape, batch, list_size, device, topn=(1, 3, 5, 10), metrics=("ndcg",)):
        super().__init__(shape, batch, list_size, device, topn=topn, metrics=metrics)
        # no backward follows an evaluation forward: the scoring entry's buffer (live activations only), not `saved`
        self.work = _f32(shape.score_bytes(self.B * self.L) // 4, device)
        self._flag = self.work[shape.score_range_flag_offset(self.B * self.L):][:1].view(torch.int32)
        self._checked = None  # (data_ptr, version) of the parameters whose split-half planes were last looked at

    def run(self, params, features, n_docs, docids, labels):
        _setrank_draw(self.L)
        hip_ops.setrank_score(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores, self.work)
        # the split-half planes of a loaded checkpoint may be out of range (|w| >= 64 / 128): the forward raised the word - look
        # (validation reads its metrics on the host anyway), switch this model to the fp32 products and score again
        # ONCE per parameter version (the word is a function of the weights; a blocking .item() per validation batch put a stream
        # synchronisation between the forward and the NDCG launch - ADVICE r05)
        key = (params.data_ptr(), params._version)
        look = key != self._checked
        self._checked = key
        if look and hip_ops.split_half_enabled(self.shape) and int(self._flag.item()) != 0:
            hip_ops.fall_back_to_fp32_products(self.shape, "a SetRank weight of magnitude >= 64 was loaded (the split-half weight planes "
                                                           "cover |w| < 128)")
            hip_ops.setrank_score(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores, self.work)
        self._ndcg(labels, docids, n_docs)
        return self.scores, self.ndcg

    def forward(self, params, features, n_docs, docids):
        _setrank_draw(self.L)
        hip_ops.setrank_score(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores, self.work)
        return self.scores


class DlcmStepEngine(StagedStepEngine):
    """The step for the DLCM ranking model: ultr_dlcm_forward -> ultr_<loss> -> ultr_dlcm_backward -> ultr_grad_sumsq ->
    ultr_apply_update.  One GPU: a process_group is refused."""

    def __init__(self, shape, batch, list_size, device, **kw):
        if kw.get("process_group") is not None:
            raise NotImplementedError("DLCM has no data-parallel step: train it on one GPU (process_group=None)")
        super().__init__(shape, batch, list_size, device, **kw)

    def _alloc(self, shape, device):
        self.saved = _f32(shape.saved_bytes(self.N) // 4, device)
        self.dl_ws = _f32(shape.workspace_bytes(self.B, self.L) // 4, device)
        self.bwd_ws = _f32(self._sumsq_floats(), device)

    def forward(self, params, features, n_docs, docids, scores=None, train=False):
        scores = self.scores if scores is None else scores
        hip_ops.dlcm_forward(self.shape, params, features, n_docs, docids, self.B, self.L, scores, saved=self.saved)
        return scores

    def backward(self, params, features, n_docs, docids):
        hip_ops.dlcm_backward(self.shape, params, features, n_docs, docids, self.B, self.L, self.saved, self.dscores, self.loss_ws,
                              hip_ops.loss_part_count(self.B), self.dl_ws, self.grads)
        hip_ops.grad_sumsq(self.grads, self.P, self.L, self.bwd_ws)


class StagedEvalEngine(EvalEngine):
    """validation() for a staged model: the scoring form of its forward on `work` (no record for a backward), then the metric launch.
    A subclass supplies forward."""

    def __init__(self, shape, batch, list_size, device, topn=(1, 3, 5, 10), metrics=("ndcg",)):
        super().__init__(shape, batch, list_size, device, topn=topn, metrics=metrics)
        self.work = _f32(shape.score_bytes(self.B * self.L) // 4, device)

    def run(self, params, features, n_docs, docids, labels):
        self.forward(params, features, n_docs, docids)
        self._ndcg(labels, docids, n_docs)
        return self.scores, self.ndcg


class DlcmEvalEngine(StagedEvalEngine):
    """validation() for DLCM: ultr_dlcm_forward's scoring form."""

    def forward(self, params, features, n_docs, docids):
        hip_ops.dlcm_forward(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores, work=self.work)
        return self.scores


class GsfStepEngine(StagedStepEngine):
    """The step for the GSF ranking model: [ultr_gsf_shuffle] -> ultr_gsf_forward -> ultr_<loss> -> ultr_gsf_backward ->
    ultr_grad_sumsq -> ultr_apply_update.  forward(train=True) of a model that shuffles (shape.train_shuffle) draws the step's
    permutations from (shape.shuffle_seed, shape.next_shuffle_step()) - the key is the model's, so another batch shape continues the
    stream - and backward() reads the same draw; every other forward runs in presented order.  One GPU: a process_group is refused."""

    def __init__(self, shape, batch, list_size, device, **kw):
        if kw.get("process_group") is not None:
            raise NotImplementedError("GSF has no data-parallel step: train it on one GPU (process_group=None)")
        super().__init__(shape, batch, list_size, device, **kw)

    def _alloc(self, shape, device):
        self.saved = _f32(shape.saved_bytes(self.N) // 4, device)
        self.gsf_ws = _f32(shape.workspace_bytes(self.B, self.L) // 4, device)
        self.bwd_ws = _f32(self._sumsq_floats(), device)
        self.perm = torch.zeros(self.B, self.L, dtype=torch.int32, device=device)
        self._perm = None  # the draw of the forward in flight (None: presented order)

    def forward(self, params, features, n_docs, docids, scores=None, train=False):
        scores = self.scores if scores is None else scores
        self._perm = None
        if train and getattr(self.shape, "train_shuffle", False):
            hip_ops.gsf_shuffle(self.shape.shuffle_seed, self.shape.next_shuffle_step(), self.B, self.L, self.perm)
            self._perm = self.perm
        hip_ops.gsf_forward(self.shape, params, features, n_docs, docids, self.B, self.L, scores, perm=self._perm, saved=self.saved)
        return scores

    def backward(self, params, features, n_docs, docids):
        hip_ops.gsf_backward(self.shape, params, features, n_docs, docids, self.B, self.L, self.saved, self.dscores, self.loss_ws,
                             hip_ops.loss_part_count(self.B), self.gsf_ws, self.grads, perm=self._perm)
        hip_ops.grad_sumsq(self.grads, self.P, self.L, self.bwd_ws)


class GsfEvalEngine(StagedEvalEngine):
    """validation() for GSF: ultr_gsf_forward's scoring form, in presented order."""

    def forward(self, params, features, n_docs, docids):
        hip_ops.gsf_forward(self.shape, params, features, n_docs, docids, self.B, self.L, self.scores, work=self.work)
        return self.scores


class DbgdEngine:
    """One DBGD / MGD step (learning_algorithm.DBGD) on one GPU, every launch on the current stream (csrc/ultr_dbgd.hip):

        ultr_dbgd_noise_args -> R + 1 x ultr_dnn_forward (validation path; ultr_dnn_build_wt before each candidate's)
        -> [need_interleave: ultr_dbgd_interleave_args] -> ultr_ndcg (R + 1 of them without interleaving) -> ultr_dbgd_grad_args
        -> ultr_apply_update (ULTR_ALGO_DBGD)

    The buffers are this engine's (one per (batch, max_candidates) shape, cached by the algorithm).  The loss is read from the update's
    host-mapped step report (read_loss, as StepEngine): no other host synchronisation."""

    def __init__(self, shape, batch, max_candidates, rank_list_size, n_rankers, device, need_interleave=True, stochastic=True, tau=1.0,
                 noise_rate=0.5, learning_rate=0.5, max_gradient_norm=5.0, optimizer="sgd", click_model=0, exam=None, n_exam=0,
                 cprob=None, seed=0, max_redraws=100):
        if not torch.cuda.is_available():
            raise RuntimeError("ultra_pytorch_amd needs an MI355X/ROCm GPU: there is no CPU fallback")
        B, M, rls, R = int(batch), int(max_candidates), int(rank_list_size), int(n_rankers)
        if not 0 < M <= _lib.DBGD_MAX_M:
            raise ValueError("DBGD / MGD support max_candidate_num up to %d (got %d)" % (_lib.DBGD_MAX_M, M))
        if not 1 <= R < _lib.DBGD_MAX_RANKERS:
            raise ValueError("DBGD / MGD support 1 .. %d candidate rankers (got %d)" % (_lib.DBGD_MAX_RANKERS - 1, R))
        if not 0 < rls <= M:
            raise ValueError("rank_list_size must be in 1 .. max_candidate_num (got %d, %d)" % (rls, M))
        self.shape, self.lib, self.device = shape, shape.lib, device
        shape.lib.ultr_config_reload()
        self.B, self.M, self.rls, self.R = B, M, rls, R
        self.need_interleave = bool(need_interleave)
        self.L = M if self.need_interleave else rls  # the forwards' list length
        P, tail = shape.n_params, hip_ops.tail_floats(M)
        self.P, self.pg, self.comm = P, None, None
        self.noise = _f32(R * P, device, zero=True).view(R, P)
        # candidate vectors on a 64-float stride: each starts 16-byte aligned, as the fast forward path needs
        self.cand_stride = (P + 63) // 64 * 64
        self.cand = _f32(R * self.cand_stride, device, zero=True).view(R, self.cand_stride)[:, :P]
        nwt = int(shape.lib.ultr_dnn_wt_floats(ctypes.byref(shape.desc)))
        self.cand_wt = [_f32(nwt, device, zero=True) for _ in range(R)]  # (alignment gaps stay zero, as WeightCopy's)
        self.scores = _f32((R + 1) * B * self.L, device, zero=True).view(R + 1, B, self.L)
        self.winners = _f32(B * (R + 1), device, zero=True).view(B, R + 1)
        self.loss_scores = _f32(B * rls, device, zero=True).view(B, rls)
        self.ndcg = _f32(R + 1, device, zero=True)
        self.ndcg_ws = _f32(B, device)
        self.grads = _f32(P + tail, device, zero=True)
        self.bwd_ws = _f32((P + tail + 63) // 64 + 16, device, zero=True)
        self.scalars = _f32(16, device, zero=True)
        self._hs = torch.zeros(16, dtype=torch.float32).pin_memory()
        self._hs_f = self._hs.numpy()
        self._hs_u = self._hs_f.view(np.uint32)
        self._seq, self._host_report = 0, True
        self._topn = (ctypes.c_int32 * 1)(rls)
        u = _lib.UpdateDesc()
        u.algo = _lib.ALGO_DBGD
        u.optimizer = _lib.OPT_SGD if optimizer == "sgd" else _lib.OPT_ADAGRAD
        u.list_size = M
        u.n_params = P
        u.learning_rate = float(learning_rate)
        u.max_gradient_norm = float(max_gradient_norm)
        u.adagrad_eps = 1e-10
        u.host_scalars = self._hs.data_ptr()
        self.udesc = u
        self._exam, self._cprob = exam, cprob  # (kept alive: the argument block points at them)
        a = self.args = _lib.DbgdArgs()
        a.desc = ctypes.pointer(shape.desc)
        a.n_params, a.n_rankers, a.batch, a.max_candidates, a.rank_list_size = P, R, B, M, rls
        a.need_interleave = 1 if self.need_interleave else 0
        a.mode = _lib.ONLINE_STOCHASTIC if stochastic else _lib.ONLINE_DETERMINISTIC
        a.max_redraws, a.click_model = int(max_redraws), int(click_model)
        a.n_exam, a.n_rel = int(n_exam), int(cprob.numel()) if cprob is not None else 0
        a.exam_prob = exam.data_ptr() if exam is not None else None
        a.click_prob = cprob.data_ptr() if cprob is not None else None
        a.noise_rate, a.tau = float(noise_rate), float(tau)
        a.seed, a.step = int(seed) & 0xFFFFFFFFFFFFFFFF, 0
        a.noise, a.cand_params, a.cand_stride = self.noise.data_ptr(), self.cand.data_ptr(), self.cand_stride
        a.scores, a.winners, a.loss_scores = self.scores.data_ptr(), self.winners.data_ptr(), self.loss_scores.data_ptr()
        a.ndcg, a.grads, a.bwd_ws = self.ndcg.data_ptr(), self.grads.data_ptr(), self.bwd_ws.data_ptr()
        self._aref = ctypes.byref(a)
        self.rng_step = 0

    read_scalars = StepEngine.read_scalars
    read_loss = StepEngine.read_loss
    _raise_on_status = StepEngine._raise_on_status
    H3_RANGE, H3_NEAR = StepEngine.H3_RANGE, StepEngine.H3_NEAR

    def close(self):
        pass

    def train_step(self, params, state, features, n_docs, docids, labels, noise_in=None, shuffles_in=None, clicks_in=None,
                   interleaved=None, teams=None, clicks=None, step=None):
        """One step on the batch docids / labels [max_candidates, B] (device).  The draws are Philox(seed, step), step = this engine's
        step counter unless given; noise_in [R, P] / shuffles_in [B, M, R + 1] / clicks_in [M, B] replace them (tests).  Optional
        [M, B] outputs: interleaved, teams, clicks.  Returns the device scalars of the update ([0] loss)."""
        lib, shape, a, st = self.lib, self.shape, self.args, hip_ops.raw_stream()
        B, L, R = self.B, self.L, self.R
        a.step = self.rng_step if step is None else int(step)
        self.rng_step += 1
        a.params = params.data_ptr()
        a.noise_in = noise_in.data_ptr() if noise_in is not None else None
        a.shuffles_in = shuffles_in.data_ptr() if shuffles_in is not None else None
        a.clicks_in = clicks_in.data_ptr() if clicks_in is not None else None
        a.interleaved = interleaved.data_ptr() if interleaved is not None else None
        a.teams = teams.data_ptr() if teams is not None else None
        a.clicks = clicks.data_ptr() if clicks is not None else None
        a.docids, a.labels, a.n_docs = docids.data_ptr(), labels.data_ptr(), int(n_docs)
        self._launch_noise(st)
        fp = features.data_ptr() if n_docs > 0 else None
        ids = docids.data_ptr()
        desc = ctypes.byref(shape.desc)
        wt0 = hip_ops.weight_copy(shape).get(params)
        _lib.check(lib.ultr_dnn_forward(desc, params.data_ptr(), wt0.data_ptr(), fp, int(n_docs), ids, B, L, self.scores[0].data_ptr(),
                                        None, st), "ultr_dnn_forward")
        for r in range(R):
            cp, cw = self.cand[r].data_ptr(), self.cand_wt[r].data_ptr()
            _lib.check(lib.ultr_dnn_build_wt(desc, cp, cw, st), "ultr_dnn_build_wt")
            _lib.check(lib.ultr_dnn_forward(desc, cp, cw, fp, int(n_docs), ids, B, L, self.scores[r + 1].data_ptr(), None, st),
                       "ultr_dnn_forward")
        ndcg = lib.ultr_ndcg
        if self.need_interleave:
            _lib.check(lib.ultr_dbgd_interleave_args(self._aref, st), "ultr_dbgd_interleave_args")
            _lib.check(ndcg(self.loss_scores.data_ptr(), labels.data_ptr(), None, int(n_docs), B, self.rls, self._topn, 1,
                            self.ndcg.data_ptr(), None, None, self.ndcg_ws.data_ptr(), st), "ultr_ndcg")
        else:
            for r in range(R + 1):
                _lib.check(ndcg(self.scores[r].data_ptr(), labels.data_ptr(), None, int(n_docs), B, self.rls, self._topn, 1,
                                self.ndcg.data_ptr() + 4 * r, None, None, self.ndcg_ws.data_ptr(), st), "ultr_ndcg")
        self._after_winners(st)
        _lib.check(lib.ultr_dbgd_grad_args(self._aref, st), "ultr_dbgd_grad_args")
        self._seq = (self._seq % 0xFFFFFFFF) + 1
        self.udesc.seq = self._seq
        _lib.check(lib.ultr_apply_update(ctypes.byref(self.udesc), desc, params.data_ptr(), wt0.data_ptr(),
                                         state.data_ptr() if state is not None else None, self.grads.data_ptr(), None,
                                         self.bwd_ws.data_ptr(), self.scalars.data_ptr(), st), "ultr_apply_update")
        return self.scalars

    def _launch_noise(self, st):
        """noise [R, P] and the candidate vectors (args.noise_in: the injected normals, or NULL)."""
        _lib.check(self.lib.ultr_dbgd_noise_args(self._aref, st), "ultr_dbgd_noise_args")

    def _after_winners(self, st):
        """Runs once the winners (or the R + 1 NDCGs) are on the stream, before the gradient: nothing for DBGD / MGD."""


class NsgdEngine(DbgdEngine):
    """One NSGD step (learning_algorithm.NSGD): DbgdEngine's step with the noise drawn from the null space of `memory` and the memory
    rewritten after the winners (csrc/ultr_nsgd.hip):

        ultr_nsgd_noise_args -> R + 1 x ultr_dnn_forward -> [ultr_dbgd_interleave_args] -> ultr_ndcg -> ultr_nsgd_memory_args
        -> ultr_dbgd_grad_args -> ultr_apply_update (ULTR_ALGO_DBGD)

    memory [R, P] (device, fp32) belongs to the caller (the algorithm: it outlives this per-shape engine) and every step reads and
    rewrites it in place."""

    def __init__(self, shape, batch, max_candidates, rank_list_size, n_rankers, device, memory=None, **kw):
        super().__init__(shape, batch, max_candidates, rank_list_size, n_rankers, device, **kw)
        R, P = self.R, self.P
        if memory is None:
            memory = _f32(R * P, device, zero=True).view(R, P)
        if (tuple(memory.shape) != (R, P) or memory.dtype != torch.float32 or not memory.is_contiguous()
                or memory.device != self.noise.device):
            raise ValueError("NSGD memory must be a contiguous float32 [%d, %d] tensor on %s" % (R, P, self.noise.device))
        self.memory = memory
        nb = int(shape.lib.ultr_nsgd_workspace_bytes(ctypes.byref(shape.desc), R))
        if nb < 0:
            raise ValueError("ultr_nsgd_workspace_bytes refused the model (%d candidate rankers)" % R)
        self.nsgd_ws = torch.zeros(max((nb + 7) // 8, 1), dtype=torch.float64, device=device)
        n = self.nargs = _lib.NsgdArgs()
        n.dbgd = ctypes.pointer(self.args)
        n.memory, n.ws = memory.data_ptr(), self.nsgd_ws.data_ptr()
        self._nref = ctypes.byref(n)
        self._unit_noise_in = None

    def train_step(self, params, state, features, n_docs, docids, labels, noise_in=None, unit_noise_in=None, **kw):
        """DbgdEngine.train_step; noise_in [R, P] replaces the Philox normals, unit_noise_in [R, P] the whole noise law (tests)."""
        self._unit_noise_in = unit_noise_in
        try:
            return super().train_step(params, state, features, n_docs, docids, labels, noise_in=noise_in, **kw)
        finally:
            self._unit_noise_in = None

    def _launch_noise(self, st):
        n, a = self.nargs, self.args
        n.normals_in, a.noise_in = a.noise_in, None
        n.unit_noise_in = self._unit_noise_in.data_ptr() if self._unit_noise_in is not None else None
        _lib.check(self.lib.ultr_nsgd_noise_args(self._nref, st), "ultr_nsgd_noise_args")

    def _after_winners(self, st):
        _lib.check(self.lib.ultr_nsgd_memory_args(self._nref, st), "ultr_nsgd_memory_args")
