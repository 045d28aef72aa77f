"""Whole-step execution: forward + backward + L2 norm [+ Adamax] captured once as a hipGraph and replayed.

The eager schedule of one CIFAR-15 step is several thousand dependent launches; replaying a
captured graph removes the Python / launch overhead without a tracing compiler. RNG state lives in device memory
and is advanced by a kernel inside the graph, so every replay draws fresh noise. With world_size > 1 the gradient
all-reduce is part of the same graph: each bucket of the (completion-ordered) gradient arena is exchanged on a side stream as
soon as backward has left it (dist.GradAllReduce), and Adamax waits for the last one. LVAE_DDP_MODE=split keeps the exchange
outside the graphs instead (fwd+bwd graph | eager all-reduce | Adamax graph): collectives that are not captured.
With a `feed` (data.DeviceDataset) the step also forms its own batch: a gather from the device-resident image table is its first launch
and the advance of the feed's cursor its last, so the replayed graph takes nothing from the host but an index table once per epoch.
With a `summary` (summary.TrainSummary) the step also folds its own metrics and the norm of the final gradient into the log window's
device accumulator, immediately before Adamax: two more launches, captured with the rest.
With a spectral regulariser on the optimizer (spectral.SpectralReg) the step runs one power-iteration step over every convolution weight
immediately before the guard's check / the summary's fold (after the exchange; under accum_steps once, in the epilogue): it adds the
penalty's gradient into the arena, and the step's dict gains the device scalars `sr_sum` and `sr_max`. The printed loss stays what it is.
With a guard on the optimizer (optim.GradGuard) the step saves the BatchNorm running statistics before the forward pass, and immediately
before Adamax takes the gradient's norm, decides whether the step is clipped or skipped and, if skipped, puts the statistics back; the
summary then reads the guard's norm instead of taking it again. A skipped step still counts as a step of the run: the global step, the beta
warm-up, the data cursor, the noise stream and num_batches_tracked advance; the model and the optimizer keep their bits.
With kl_balance (balance.KlBalance) every forward pass of the step balances the per-layer KL terms of its loss while beta < 1, in the KL
bookkeeping launch it issues anyway (one launch replaced each way); under accum_steps every micro-pass on its own rows, with several ranks
every rank on its shard.
With accum_steps = M > 1 one optimizer step consumes M micro-batches: zero_grad [+ the guard's save] once | gather, forward, backward, the
fold of the pass's metrics into their means (kernels.micro_fold) and the cursor advance, M times | the exchange (split form) once | guard,
summary, optimizer and beta counter once. Captured, these are three graphs in one pool, the middle one replayed M times.
"""
import os
import sys
import time

import torch

from . import kernels as K
from . import ops


def linear_anneal(step, start, end, steps):
    """boilr.utils.linear_anneal (absent; restated): linear ramp from start to end over `steps` steps, then flat."""
    if steps <= 0:
        return end
    return start + (end - start) * min(max(step / float(steps), 0.0), 1.0)


def global_step_counter(model):
    """The device int64[1] mirror of `model.global_step` that the annealed loss reads (created on first use, then advanced on the device
    by every annealed training step, inside its graph)."""
    dev = next(model.parameters()).device
    c = getattr(model, 'global_step_dev', None)
    if c is None or c.device != dev:
        c = torch.full((1,), int(model.global_step), dtype=torch.int64, device=dev)
        model.global_step_dev = c
    return c


def check_iw_objective(model, iw_samples):
    """The K-sample importance-weighted bound needs per-row log weights ll - kl_sep with kl_sep the Monte-Carlo log q - log p; ValueError for
    a model whose configuration makes the bound meaningless."""
    iw_samples = int(iw_samples)
    if iw_samples < 1:
        raise ValueError("iw_samples must be at least 1, got %d" % iw_samples)
    if iw_samples > 1:
        if float(model.free_bits) >= 1e-6:
            raise ValueError("iw_samples=%d with free_bits=%g: the free-bits clamp has no importance-weighted form; train the bound with "
                             "free_bits=0" % (iw_samples, model.free_bits))
        if any(layer.analytical_kl for layer in model.top_down_layers):
            raise ValueError("iw_samples=%d with analytical_kl=True: the importance weights need the Monte-Carlo log q - log p of the drawn "
                             "sample, not the analytical KL" % iw_samples)
    return iw_samples


def micro_slices(rows, accum_steps):
    """The rows of one optimizer step cut into `accum_steps` equal micro-batches, in order: [(lo, hi), ...]. ValueError when accum_steps < 1
    or the rows do not divide by it (a pure function: no tensor, no device)."""
    rows, m = int(rows), int(accum_steps)
    if m < 1:
        raise ValueError("accum_steps must be at least 1, got %d" % m)
    if rows < m or rows % m:
        raise ValueError("a step of %d rows cannot be cut into %d equal micro-batches" % (rows, m))
    per = rows // m
    return [(j * per, (j + 1) * per) for j in range(m)]


def bind_kl_balance(model, kl_balance, beta=1.0, beta_anneal=0, iw_samples=1):
    """Hands a balance.KlBalance to the model, bound to the beta source the loss head uses: the device step counter under beta_anneal, else
    the constant. ValueError with iw_samples > 1: the bound is formed from kl_sep, and a balanced bound has no reported meaning."""
    if int(iw_samples) > 1:
        raise ValueError("KL balancing reweights the per-layer terms of the ELBO's kl_loss; the importance-weighted bound (iw_samples=%d) "
                         "is formed from kl_sep and has no balanced form" % int(iw_samples))
    kl_balance.attach(model)
    if beta_anneal:
        kl_balance.bind(step=global_step_counter(model), anneal_steps=int(beta_anneal))
    else:
        kl_balance.bind(beta=float(beta))
    model.kl_balance = kl_balance


def forward_pass(model, x, beta=1.0, compute_l2=True, beta_anneal=0, iw_samples=1, kl_balance=None):
    """LVAEExperiment.forward_pass (experiment/experiment_manager.py:322-367) on the HIP engine. beta_anneal != 0: the KL warm-up,
    beta = linear_anneal(global step, 0, 1, beta_anneal) read on the device from `global_step_counter(model)` (`beta` is ignored).
    iw_samples = K > 1 (engine-only): the loss is the K-sample importance-weighted bound, -mean_b logmeanexp_k(ll - beta kl_sep), over K
    samples per image that share one bottom-up pass (LadderVAE.forward(n_samples=K)); `elbo`, `recons`, `kl` are means over the K * B rows
    and `out` also carries `iw` (the bound at beta = 1), `ess` (the effective sample size of the weights) and `iw_weights`.
    kl_balance (engine-only; a balance.KlBalance): becomes the model's `kl_balance`, bound to this pass's beta source, so that a training
    pass balances the per-layer KL terms of `loss` while beta < 1; `elbo`, `kl`, `recons` and `kl_avg_layerwise` stay the plain numbers.
    None leaves the model as it is."""
    iw_samples = check_iw_objective(model, iw_samples)
    if kl_balance is not None:
        bind_kl_balance(model, kl_balance, beta, beta_anneal, iw_samples)
    mo = model(x, n_samples=iw_samples) if iw_samples > 1 else model(x)
    iw = None
    if iw_samples > 1 and beta_anneal:
        elbo_sep, loss, elbo, recons, iw, ess, w = ops.IwLossAnnealFn.apply(mo['ll'], mo['kl_sep'], global_step_counter(model), int(beta_anneal),
                                                                            iw_samples)
    elif iw_samples > 1:
        elbo_sep, loss, elbo, recons, iw, ess, w = ops.IwLossFn.apply(mo['ll'], mo['kl_sep'], float(beta), iw_samples)
    elif beta_anneal:
        elbo_sep, loss, elbo, recons = ops.ElboLossAnnealFn.apply(mo['ll'], mo['kl_sep'], mo['kl_loss'], global_step_counter(model),
                                                                  int(beta_anneal))
    else:
        elbo_sep, loss, elbo, recons = ops.ElboLossFn.apply(mo['ll'], mo['kl_sep'], mo['kl_loss'], float(beta))
    out = {'loss': loss, 'elbo': elbo, 'elbo_sep': elbo_sep, 'kl': mo['kl'], 'recons': recons,
           'out_mean': mo['out_mean'], 'out_mode': mo['out_mode'], 'out_sample': mo['out_sample'],
           'likelihood_params': mo['likelihood_params'], 'kl_avg_layerwise': mo['kl_avg_layerwise']}
    if iw is not None:
        out.update(iw=iw, ess=ess, iw_weights=w)
    if compute_l2:
        with torch.no_grad():
            out['l2'] = K.l2norm(model.arena.params).view(())
    return out


class TrainStep:
    """step(x) -> dict of scalars (device tensors, valid until the next step). With feed=DeviceDataset: step(), the batch is gathered on
    the device at the feed's cursor (eager steps and the captured step alike: gather | forward, backward, exchange, Adamax | cursor advance)."""

    def __init__(self, model, optimizer, beta=1.0, use_graph=True, allreduce=None, eager_warmup=2, async_wgrad=False,
                 wgrad_streams=1, wgrad_group_rows=16384, beta_anneal=0, feed=None, summary=None, iw_samples=1, accum_steps=1,
                 kl_balance=None):
        self.model, self.opt, self.beta = model, optimizer, beta
        self.accum = int(accum_steps)         # M > 1: one optimizer step over M micro-batches (prologue | M micro-passes | exchange | epilogue)
        if self.accum < 1:
            raise ValueError("accum_steps must be at least 1, got %d" % self.accum)
        self.iw_samples = check_iw_objective(model, iw_samples)   # K > 1: train on the K-sample importance-weighted bound
        self.kl_balance = kl_balance          # balance.KlBalance: every (micro-)pass balances its KL terms on its own rows while beta < 1
        if kl_balance is not None:
            # weights on the device, beta source bound, the model's property set: all before anything is captured
            bind_kl_balance(model, kl_balance, beta, beta_anneal, self.iw_samples)
        self.feed = feed
        self.summary = summary                # None: the step issues not one launch more
        self._grad_norm = None
        self.beta_anneal = int(beta_anneal)   # != 0: KL warm-up on the device counter (beta is then ignored)
        dev = next(model.parameters()).device
        self.side = [torch.cuda.Stream(device=dev) for _ in range(max(1, int(wgrad_streams)))] if async_wgrad else None
        self.use_graph, self.allreduce = use_graph, allreduce
        self.wgrad_group_rows = wgrad_group_rows
        self.eager_left = eager_warmup if use_graph else -1
        self.graph_a = self.graph_b = self.graph_p = None
        self.fallback_reason = None
        self.static_x = None
        self.static_out = None
        self._bns = None
        self._table_ref = None
        if allreduce is not None and allreduce.world > 1:
            optimizer._state()
            optimizer.gscale = allreduce.scale
        if (allreduce is not None and allreduce.active and allreduce.on_gpu and not allreduce.capturable
                and os.environ.get('LVAE_ALLOW_GLOO_GRAPH') != '1'):   # (the override exists for the stall diagnosis of DESIGN.md §6)
            self.use_graph, self.eager_left = False, -1   # gloo stages device buffers through the host: cannot be part of a graph
        self.trace = os.environ.get('LVAE_STEP_TRACE') == '1'   # diagnosis only: host-synchronised phase times on stderr
        self.overlap = allreduce is not None and allreduce.active and allreduce.overlap
        if self.overlap and self.accum > 1:
            raise ValueError("accum_steps=%d needs the gradient exchange in split form (one exchange after the last micro-pass); the "
                             "overlapped form (LVAE_DDP_MODE=overlap) would exchange every micro-pass: use LVAE_DDP_MODE=split" % self.accum)
        if self.accum > 1:
            # the arena holds the SUM over the M micro-passes (and, after the exchange, over the ranks): the guard's norm, the summary's
            # grad and the update all scale it by this one device float, so they see the mean over the M * batch-size images
            optimizer._state()
            world = allreduce.world if allreduce is not None else 1
            optimizer.gscale = torch.full((1,), 1.0 / (self.accum * world), dtype=torch.float32, device=dev)
            n = K.MICRO_FIXED + len(model.top_down_layers)
            self._macc = torch.zeros(n, dtype=torch.float64, device=dev)     # lvae_micro_fold_f64: sums of the passes so far,
            self._mcount = torch.zeros(1, dtype=torch.int64, device=dev)     # how many there were,
            self._mean = torch.zeros(n, dtype=torch.float32, device=dev)     # and the means of the last complete step
            names = ('loss', 'elbo', 'recons', 'kl', 'l2') + (('iw', 'ess') if self.iw_samples > 1 else ())
            slot = {'loss': 0, 'elbo': 1, 'recons': 2, 'kl': 3, 'l2': 4, 'iw': 5, 'ess': 6}
            self._mean_out = {k: self._mean[slot[k]] for k in names}
            self._mean_out['kl_avg_layerwise'] = self._mean[K.MICRO_FIXED:]
        if self.overlap and self.use_graph:
            # can the exchange be part of the step graph? If not, the same process continues with the exchange
            # outside the graphs: fwd+bwd graph | eager all-reduce | Adamax graph
            ok, why = allreduce.capture_probe()
            if not ok:
                print('[lvae] the gradient exchange cannot be captured into the step graph (%s); keeping it outside '
                      '(LVAE_DDP_MODE=split)' % why, file=sys.stderr, flush=True)
                self.overlap, self.fallback_reason = False, why
        if self.overlap:
            model.grad_tracker = allreduce   # the model's segment markers report to it during backward
        if getattr(optimizer, 'guard', None) is not None:
            optimizer._state()
            optimizer.guard.attach(model)    # state, shadow and copy tables exist before anything is captured
        if getattr(optimizer, 'spectral', None) is not None:
            optimizer._state()
            optimizer.spectral.prepare(model, guarded=getattr(optimizer, 'guard', None) is not None)   # table, iterate (warm start), twin
        if feed is not None:
            feed.attach(model, self.accum)   # cursor = model.global_step * M: a resumed run continues in the middle of its epoch
            self.static_x = feed.new_batch()

    def _fwd_bwd(self, x, micro=False):
        """One forward and backward pass. micro: a micro-pass of an accumulated step, which neither clears the arena nor saves the BatchNorm
        statistics (the prologue did) nor advances the beta counter (the epilogue will), and ends in micro_fold and the feed's advance."""
        done = False
        try:
            if self.feed is not None:
                x = self.feed.gather(self.static_x)   # first launch of a fed step
            if getattr(self.opt, 'guard', None) is not None and not micro:
                self.opt.guard.save_bn(self.model)    # a skipped step puts them back (_fold)
            if not micro:
                self.opt.zero_grad()
            K.prepared.prepare_all()  # one launch: transformed weights of every Winograd convolution seen so far
            # (a kl_balance was bound and handed to the model by __init__, once: the pass finds it there)
            out = forward_pass(self.model, x, self.beta, beta_anneal=self.beta_anneal, iw_samples=self.iw_samples)
            if self.allreduce is not None:
                self.allreduce.begin_step()
            ops.set_wgrad_stream(self.side)
            ops.set_wgrad_grouping(self.wgrad_group_rows)
            if self.side is not None:
                for st in self.side:
                    st.wait_stream(torch.cuda.current_stream())  # zero_grad happens-before every wgrad accumulate
            out['loss'].backward()
            ops.flush_wgrad_group()
            ops.join_wgrad_stream()
            if self.overlap:
                self.allreduce.finish()  # last bucket + join: the gradients are summed over ranks from here on
            if self.beta_anneal and not micro:
                K.counter_advance(global_step_counter(self.model), 1)   # the next step's beta; inside the graph when captured
            if micro:
                K.micro_fold(out['loss'], out['elbo'], out['recons'], out['kl'], out['l2'], out['kl_avg_layerwise'], self.accum,
                             self._macc, self._mcount, self._mean, iw=out.get('iw'), ess=out.get('ess'))
                if self.feed is not None:
                    self.feed.advance()   # the cursor counts micro-batches
            done = True
        finally:
            if not done:
                # The pass was abandoned by an exception (possibly inside a hipGraph capture that is being torn down). Nothing more may be
                # LAUNCHED on its behalf: the queued weight gradients are dropped, not flushed (their inputs belong to the abandoned pass);
                # the transformed-weight stamps are withdrawn (prepare_all marked the buffers current for a launch that may never have
                # run); the exchange's bucket cursor is rewound; side streams are joined so that no fork is left dangling. The next
                # step — eager or a fresh capture — starts from a clean state (tests/test_model_gpu.py raises inside a captured backward).
                ops.drop_wgrad_group()
                K.prepared.invalidate()
                if self.allreduce is not None:
                    self.allreduce.begin_step()
                if not torch.cuda.is_current_stream_capturing():
                    try:
                        ops.join_wgrad_stream()
                    except RuntimeError:
                        pass
            ops.set_wgrad_grouping(None)
            ops.set_wgrad_stream(None)
        keys = ('loss', 'elbo', 'recons', 'kl', 'l2', 'kl_avg_layerwise') + (('iw', 'ess') if self.iw_samples > 1 else ())
        return {k: out[k].detach() for k in keys}

    def _fold(self, out):
        """The step's metrics and the norm of the gradient Adamax is about to apply (summed over ranks by now, scaled like Adamax scales it)
        into the log window. Called immediately before every `self.opt.step()`; captured with it."""
        guard = getattr(self.opt, 'guard', None)
        sr = getattr(self.opt, 'spectral', None)
        if sr is not None:
            # the spectral penalty's gradient joins the arena first: the guard's norm, the clip factor and `grad:` see the regularised gradient
            sr.step(self.model, self.opt.gscale, guarded=guard is not None)
            out['sr_sum'], out['sr_max'] = sr.sr_sum, sr.sr_max
        if guard is not None:
            # the same place is the guard's: norm, decision, and the BatchNorm statistics of a skipped step back where they were
            guard.check(self.model.arena.grads, self.opt.gscale)
            if sr is not None:
                sr.finish(guard.skip)    # a skipped step leaves u, v and sigma where they were
            guard.restore_bn()
            if self.summary is not None:
                self.summary.fold(out, guard.norm, self.opt.gscale)
            return
        if self.summary is None:
            if sr is not None:
                sr.finish()
            return
        grads = self.model.arena.grads
        if self._grad_norm is None:
            self._grad_norm = torch.empty((1,), dtype=torch.float32, device=grads.device)
        self.summary.fold(out, K.l2norm(grads, out=self._grad_norm), self.opt.gscale)
        if sr is not None:
            sr.finish()

    def _eager(self, x):
        out = self._fwd_bwd(x)
        if self.allreduce is not None and not self.overlap:
            self.allreduce.run()
        self._fold(out)
        self.opt.step()
        if self.feed is not None:
            self.feed.advance()   # last launch: a step abandoned before this point leaves the cursor where it was
        return out

    # ---- accum_steps = M > 1 ------------------------------------------------------------------------------------------------------
    def _prologue(self):
        self.opt.zero_grad()
        if getattr(self.opt, 'guard', None) is not None:
            self.opt.guard.save_bn(self.model)    # the statistics from before the first micro-pass: a skipped step puts them back

    def _epilogue(self):
        self._fold(self._mean_out)                # guard, BatchNorm restore and log window read the means over the micro-passes
        self.opt.step()
        if self.beta_anneal:
            K.counter_advance(global_step_counter(self.model), 1)

    def _capture_accum(self, x0):
        """Three graphs in one pool: the prologue, ONE micro-pass (replayed M times) and the epilogue; the exchange runs between the last
        two, outside them."""
        if self.feed is None:
            self.static_x = torch.empty_like(x0)
        torch.cuda.synchronize()
        self.graph_p, self.graph_a, self.graph_b = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph_p, capture_error_mode='thread_local'):
            self._prologue()
        with torch.cuda.graph(self.graph_a, pool=self.graph_p.pool(), capture_error_mode='thread_local'):
            self._fwd_bwd(self.static_x, micro=True)
        with torch.cuda.graph(self.graph_b, pool=self.graph_p.pool(), capture_error_mode='thread_local'):
            self._epilogue()
        self._bns = self.model.bn_modules()
        self._table_ref = K.prepared.pin_current()

    def _abandon(self, completed, bns, pend0):
        """An accumulated step was given up (a failed capture, an exception in a micro-pass): no graph, no host counter and no device
        counter of the step's own keeps anything of it. Runs outside any capture."""
        self.graph_p = self.graph_a = self.graph_b = None
        self.static_out = None
        self._table_ref = None
        for bn, p0 in zip(bns, pend0):
            bn._pending = p0
        self.model.global_step = completed
        if not torch.cuda.is_current_stream_capturing():
            self._macc.zero_()
            self._mcount.zero_()
            if self.feed is not None and self.feed.cursor is not None:
                self.feed.cursor.fill_(completed * self.accum)

    def _accum_step(self, x):
        m, model, feed = self.accum, self.model, self.feed
        # (cut before anything is counted: rows that do not divide by M raise here)
        parts = None if feed is not None else [x[lo:hi] for lo, hi in micro_slices(x.shape[0], m)]
        if self.beta_anneal:
            global_step_counter(model)
        completed = model.global_step
        bns = model.bn_modules()
        pend0 = [bn._pending for bn in bns]
        model.global_step += 1
        try:
            if not self.use_graph or self.eager_left > 0:
                self.eager_left -= 1
                self._prologue()
                for j in range(m):
                    if feed is not None:
                        feed.before_step(completed * m + j)   # an epoch may end inside a step
                    self._fwd_bwd(None if parts is None else parts[j], micro=True)
                if self.allreduce is not None:
                    self.allreduce.run()
                self._epilogue()
                return self._mean_out
            just_captured = self.graph_a is None
            if just_captured:
                self._capture_accum(None if parts is None else parts[0])   # the Python micro-pass ran once: one BN forward is counted
            self.graph_p.replay()
            for j in range(m):
                if feed is not None:
                    feed.before_step(completed * m + j)
                else:
                    self.static_x.copy_(parts[j], non_blocking=True)
                self.graph_a.replay()
            if self.allreduce is not None:
                self.allreduce.run()
            self.graph_b.replay()
            K.prepared.weights_written()
            if model.training:
                for bn in self._bns:
                    bn._pending += m - (1 if just_captured else 0)
            return self._mean_out
        except BaseException:
            self._abandon(completed, bns, pend0)
            raise

    def _capture(self, x):
        if self.feed is None:
            self.static_x = torch.empty_like(x)
            self.static_x.copy_(x)
        fused = self.allreduce is None or not self.allreduce.active or self.overlap
        torch.cuda.synchronize()
        self.graph_a = torch.cuda.CUDAGraph()
        # thread_local: the RCCL watchdog thread of an initialised process group may query events while this thread captures.
        # (Whether the exchange CAN be captured was settled by GradAllReduce.capture_probe() in __init__: a refusal inside this capture
        # would leave a half-captured training step behind, and unwinding that is not safe.)
        # Host-side counters the Python pass advances while it is captured: if EITHER capture fails they go back, so that a caller who catches
        # the error and steps again neither replays half a step (graph A without the exchange and the optimizer) nor counts a BatchNorm
        # forward / a global step that never ran
        bns = self.model.bn_modules()
        pend0 = [bn._pending for bn in bns]
        try:
            with torch.cuda.graph(self.graph_a, capture_error_mode='thread_local'):
                self.static_out = self._fwd_bwd(self.static_x)
                if fused:
                    self._fold(self.static_out)
                    self.opt.step()
                    if self.feed is not None:
                        self.feed.advance()
            if not fused:
                self.graph_b = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.graph_b, pool=self.graph_a.pool(), capture_error_mode='thread_local'):
                    self._fold(self.static_out)
                    self.opt.step()
                    if self.feed is not None:
                        self.feed.advance()
        except BaseException:
            # a failed capture leaves no usable graph: drop both so that the next call captures again (or runs eagerly) from clean state
            self.graph_a = self.graph_b = None
            self.static_out = None
            self._table_ref = None
            for bn, p0 in zip(bns, pend0):
                bn._pending = p0
            self.model.global_step -= 1   # __call__ counted this step before capturing it
            raise
        self._bns = bns
        # the captured prepare_all launch baked in the device address (and entry count) of the transformed-weight table: keep exactly
        # that table, and the scratch buffers its entries point to, alive and unmodified for as long as this graph can be replayed
        self._table_ref = K.prepared.pin_current()

    def exchange_description(self):
        """How the gradients are exchanged in this process (bench.py's config.grad_exchange)."""
        ar = self.allreduce
        if ar is None or not ar.active:
            return 'none (single rank)'
        if self.overlap:
            where = 'inside the step graph' if self.use_graph else 'eager launches'
            return '%d completion-ordered buckets on a side stream during backward, %s' % (len(ar.buckets), where)
        why = ' (fallback: %s)' % self.fallback_reason if getattr(self, 'fallback_reason', None) else ''
        return ('%d bucket(s) after backward on the side stream, between the fwd+bwd graph and the Adamax graph (split: side branches of a '
                'captured graph do not overlap on this platform, DESIGN.md §6)%s' % (len(ar.buckets), why))

    def _traced_split_step(self):
        ts = [time.perf_counter()]
        for phase in (self.graph_a.replay, self.allreduce.run, self.graph_b.replay):
            phase()
            torch.cuda.synchronize()
            ts.append(time.perf_counter())
        print('[step-trace] graph A %.1f ms | all-reduce %.1f ms | graph B %.1f ms' %
              tuple((b - a) * 1e3 for a, b in zip(ts, ts[1:])), file=sys.stderr, flush=True)
        K.prepared.weights_written()
        return self.static_out

    def __call__(self, x=None):
        if (x is None) == (self.feed is None):
            raise ValueError("a step takes its batch either as x or from feed=, not both and not neither")
        if self.accum > 1:
            return self._accum_step(x)
        if self.beta_anneal:
            global_step_counter(self.model)   # (created before this step is counted: it holds the number of COMPLETED steps)
        if self.feed is not None:
            self.feed.before_step(self.model.global_step)   # outside the graph: a new epoch's index table, ordered before the step
        self.model.global_step += 1
        if not self.use_graph or self.eager_left > 0:
            self.eager_left -= 1
            return self._eager(x)
        just_captured = self.graph_a is None
        if just_captured:
            self._capture(x)  # the Python forward ran once while capturing: it already counted this step's BN forwards
        elif self.feed is None:
            self.static_x.copy_(x, non_blocking=True)
        if self.trace and self.graph_b is not None:
            return self._traced_split_step()
        self.graph_a.replay()
        if self.graph_b is not None:
            self.allreduce.run()
            self.graph_b.replay()
        K.prepared.weights_written()  # the replayed optimizer kernel changed the weights behind Python's back
        if self.model.training and not just_captured:
            for bn in self._bns:
                bn._pending += 1
        return self.static_out


class AutoExchangeStep:
    """step(x) for a multi-rank run that does not take the form of its gradient exchange on faith.

    north_star asks for the all-reduce "overlapped with backward on a side HIP stream"; on a one-rank rehearsal that form measured SLOWER
    inside a captured step than one exposed message between two graphs. Which one wins on N real ranks over xGMI is a
    measurement this process can make itself: it builds BOTH forms — 'split' (fwd+bwd graph | whole-arena all-reduce | Adamax graph) and
    'overlap' (completion-ordered 8 MB buckets on the side stream during backward, one graph) — on one shared communicator, runs
    `trial_steps` timed steps of each after its warm-up / capture steps (all of them REAL training steps: both forms compute the same
    update), reduces the times with MAX over ranks (dist.FormSelector) and continues with the faster form; the other form's graph is dropped.
    LVAE_DDP_MODE=split|overlap skips the trial. `timings_ms` / `chosen` go into bench.py's line (config.grad_exchange_ab).
    A gradient guard is the optimizer's (`optimizer.guard`), so both forms run under the same one: one shadow, one pair of counters."""

    def __init__(self, model, optimizer, flat_grads, segments, group=None, trial_steps=3, forms=None, feed=None, summary=None,
                 **step_kwargs):
        from . import dist as ldist
        self.model = model
        env = os.environ.get('LVAE_DDP_MODE')
        if forms is None and env != 'overlap' and int(step_kwargs.get('accum_steps', 1)) > 1:
            forms = ['split']   # accumulated steps exchange once, after the last micro-pass: there is no second form to try
        forms = list(forms) if forms is not None else ([env] if env in ('split', 'overlap') else ['split', 'overlap'])
        self.ars, self.steps = {}, {}
        comm = None
        for f in forms:
            ar = ldist.GradAllReduce(flat_grads, group=group, segments=segments, mode=f, comm=comm)
            if comm is None:
                comm = ar.comm
            # one feed, one cursor, one summary: every trial step is a real step
            st = TrainStep(model, optimizer, allreduce=ar, feed=feed, summary=summary, **step_kwargs)
            if f == 'overlap' and not st.overlap and 'split' in forms:
                continue   # the overlapped form is not available here (capture probe refused): it would just be a second 'split'
            self.ars[f], self.steps[f] = ar, st
        dev = flat_grads.device
        self.selector = ldist.FormSelector(list(self.steps), trial_steps, group=group, device=dev if flat_grads.is_cuda else 'cpu')
        self.group = group
        self.chosen = self.selector.chosen
        self.timings_ms = None
        self._untimed = {}
        self._arm(self.chosen or self.selector.current())

    def _arm(self, form):
        st = self.steps[form]
        self.model.grad_tracker = self.ars[form] if st.overlap else None
        return st

    @property
    def ready(self):
        return self.chosen is not None

    @property
    def use_graph(self):
        return self.steps[self.chosen or next(iter(self.steps))].use_graph

    @property
    def allreduce(self):
        return self.ars[self.chosen or next(iter(self.ars))]

    def __call__(self, x=None):
        if self.chosen is not None:
            return self.steps[self.chosen](x)
        import torch.distributed as tdist
        form = self.selector.current()
        st = self._arm(form)
        # eager warm-up steps and the capturing step are not timed; without a graph, the first step of a form (lazy initialisations) is not
        warming = (st.use_graph and (st.eager_left > 0 or st.graph_a is None)) or self._untimed.get(form, 0) < 1
        if warming:
            self._untimed[form] = self._untimed.get(form, 0) + 1
            return st(x)
        on_gpu = x is None or x.is_cuda
        if tdist.is_initialized() and tdist.get_world_size(self.group) > 1:
            tdist.barrier(group=self.group)
        if on_gpu:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = st(x)
        if on_gpu:
            torch.cuda.synchronize()
        self.selector.record(form, time.perf_counter() - t0)
        if self.selector.complete():
            self.chosen = self.selector.decide()
            self.timings_ms = self.selector.timings_ms
            for f in list(self.steps):
                if f != self.chosen:   # the loser's graphs (and their memory pools) go
                    self.steps[f].graph_a = self.steps[f].graph_b = self.steps[f].graph_p = None
                    self.steps[f].static_out = None
            self._arm(self.chosen)
            print('[lvae] gradient exchange: %s' % self.exchange_description(), file=sys.stderr, flush=True)
        return out

    def exchange_description(self):
        if self.chosen is None:
            return 'undecided (trial steps still running)'
        d = self.steps[self.chosen].exchange_description()
        if self.timings_ms:
            d += ' | chosen at run time: ' + ', '.join('%s %.3f ms/step' % (f, t) for f, t in self.timings_ms.items()) + \
                 ' (max over ranks of %d timed steps each)' % self.selector.trial_steps
        return d

    def close(self):
        seen = set()
        for ar in self.ars.values():
            if ar.comm is not None and id(ar.comm) not in seen and ar.owns_comm:
                seen.add(id(ar.comm))
                ar.close()
            else:
                ar.comm = None
