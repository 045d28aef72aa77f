"""Adamax over the flat parameter arena — one kernel per step instead of torch.optim.Adamax's per-tensor loop
(experiment/experiment_manager.py:76-81: lr 3e-4, betas (0.9, 0.999), eps 1e-8, L2 weight decay added to the grad).

With `ema_decay > 0` the same kernel pass also keeps an exponential moving average of the weights (`self.ema`), the weights a test
ELBO / importance-weighted bound is normally reported from; `swap_ema()` puts it in the parameters' place for a test pass.

With a `schedule` (LrSchedule) the kernel computes the learning rate itself from the device step counter, so a captured step replays along
warm-up and decay; `lr_now` holds the rate of the last step.

With a `guard` (GradGuard) the step is preceded by a look at the gradient's norm on the device: the gradient is clipped to `max_norm`, and a
step whose norm is not finite or exceeds `skip_threshold` is left out as if it had not happened (parameters, exp_avg, exp_inf, the step
counter, the average and lr_now keep their bits), all of it inside the captured step.

With `spectral` (spectral.SpectralReg) the step is preceded by one power-iteration step over every convolution weight, which adds the
gradient of lam * sum sigma into the arena before the guard takes its norm; a skipped step leaves the iterate where it was.

`Adam` / `AdamW` are a second update rule on the same arena (torch.optim.Adam with L2 decay, torch.optim.AdamW with decoupled decay) with the
same average, schedule and guard: `ArenaOptimizer` holds what does not depend on the rule, each rule launches its own kernel.
"""
import contextlib
import math

import numpy as np
import torch

from . import kernels as K


def ema_decay_at(decay, n):
    """The decay the kernel applies at the step that follows `n` completed ones: min(decay, (1 + n) / (10 + n)), every operation in fp32
    as on the device (lvae_adamax_ema_step_f32). Returns a numpy float32."""
    f = np.float32
    n = f(n)
    return min(f(decay), (f(1) + n) / (f(10) + n))


class LrSchedule:
    """Linear warm-up over `warmup_steps` steps, then `kind` ('constant', 'cosine', 'linear', 'step', 'exp') over `decay_steps` steps down
    to `min_lr` (struct lvae_lr_schedule of include/lvae_hip.h has the formulas). The base rate is the optimizer's `lr`."""
    FIELDS = ('kind', 'warmup_steps', 'decay_steps', 'min_lr', 'gamma')

    def __init__(self, kind='constant', warmup_steps=0, decay_steps=0, min_lr=0.0, gamma=0.1):
        self.kind, self.warmup_steps, self.decay_steps = str(kind), int(warmup_steps), int(decay_steps)
        self.min_lr, self.gamma = float(min_lr), float(gamma)
        if self.kind not in K._C.LR_KINDS:
            raise ValueError("unknown lr schedule %r (one of %s)" % (kind, ', '.join(K._C.LR_KINDS)))
        if not self.min_lr >= 0.0:
            raise ValueError("min_lr must not be negative, got %r" % (min_lr,))
        if not 0.0 < self.gamma <= 1.0:
            raise ValueError("gamma must lie in (0, 1], got %r" % (gamma,))
        if self.warmup_steps < 0:
            raise ValueError("warmup_steps must not be negative, got %r" % (warmup_steps,))
        if self.kind != 'constant' and self.decay_steps <= 0:
            raise ValueError("a %s schedule needs decay_steps > 0, got %r" % (self.kind, decay_steps))

    def struct(self, base_lr):
        """struct lvae_lr_schedule for this schedule on `base_lr` (checked against it: base_lr > 0, min_lr <= base_lr)."""
        if not float(base_lr) > 0.0:
            raise ValueError("a scheduled lr must be positive, got %r" % (base_lr,))
        if self.min_lr > float(base_lr):
            raise ValueError("min_lr %r exceeds the base lr %r" % (self.min_lr, base_lr))
        return K.lr_schedule_struct(base_lr, self.kind, self.warmup_steps, self.decay_steps, self.min_lr, self.gamma)

    def at(self, base_lr, n):
        """The lr of the step that follows `n` completed ones, as the kernel computes it (lvae_lr_schedule_at: host code, no GPU)."""
        return K.lr_schedule_at(self.struct(base_lr), n)

    def state_dict(self):
        return {k: getattr(self, k) for k in self.FIELDS}

    def __eq__(self, other):
        return isinstance(other, LrSchedule) and self.state_dict() == other.state_dict()

    def __repr__(self):
        return 'LrSchedule(%s)' % ', '.join('%s=%r' % kv for kv in self.state_dict().items())


class GradGuard:
    """Clip the gradient arena to the global norm `max_norm` (torch.nn.utils.clip_grad_norm_'s factor min(1, G / (norm + 1e-6))) and leave
    out every step whose norm is not finite or exceeds `skip_threshold`; None switches either off (non-finite steps are always left out).
    `norm` is the L2 norm of the arena after the gradient exchange times the optimizer's gscale, the number a train line prints as `grad:`.
    Owns the device struct lvae_grad_guard_state (`state`: int64[4]; views `norm`, `scale`, `skip`; cumulative `clipped` / `skipped`
    counters) and, once attached to a model, a shadow of every BatchNorm running statistic with the two copy tables that save and restore
    them: the forward pass of a step that is then skipped has already moved them."""

    def __init__(self, max_norm=None, skip_threshold=None):
        if max_norm is not None:
            max_norm = float(max_norm)
            if not (max_norm > 0.0 and math.isfinite(max_norm)):
                raise ValueError("max_norm must be a positive finite number (None: no clipping), got %r" % (max_norm,))
        if skip_threshold is not None:
            skip_threshold = float(skip_threshold)
            if not skip_threshold >= 0.0:
                raise ValueError("skip_threshold must not be negative or NaN (None or inf: skip non-finite steps only), got %r"
                                 % (skip_threshold,))
        self.max_norm, self.skip_threshold = max_norm, skip_threshold
        self.state = None            # device int64[4]: struct lvae_grad_guard_state
        self.norm = self.scale = self.skip = None
        self.checked = False         # check() ran for the step Adamax.step() is about to apply
        self._counts0 = (0, 0)       # counters to start from (load_state_dict before the state exists)
        self._bn_key = self._shadow = self._save = self._restore = None

    def limits(self):
        return {'max_norm': self.max_norm, 'skip_threshold': self.skip_threshold}

    def _alloc(self, device):
        if self.state is None or self.state.device != device:
            counts = self.counts() if self.state is not None else self._counts0
            self.state = torch.tensor([0, 0, counts[0], counts[1]], dtype=torch.int64).to(device)
            f, i = self.state.view(torch.float32), self.state.view(torch.int32)
            self.norm, self.scale, self.skip = f[0:1], f[1:2], i[2:3]
        return self.state

    def check(self, grads, gscale=None):
        """Takes the norm of `grads` and decides this step (two launches). Before Adamax.step(), which runs it itself if nobody has."""
        self._alloc(grads.device)
        K.grad_guard(grads, gscale, self.max_norm or 0.0, -1.0 if self.skip_threshold is None else self.skip_threshold, self.state)
        self.checked = True

    def attach(self, model):
        """Builds the shadow of the model's BatchNorm running statistics and the save / restore tables (again if the buffers have moved)."""
        self._alloc(next(model.parameters()).device)
        bufs = [b for bn in model.bn_modules() for b in (bn.running_mean, bn.running_var)]
        key = tuple(b.data_ptr() for b in bufs)
        if key == self._bn_key:
            return
        self._bn_key, self._shadow, self._save, self._restore = key, None, None, None
        if not bufs:
            return
        dev = bufs[0].device
        self._shadow = torch.zeros(sum(b.numel() for b in bufs), dtype=torch.float32, device=dev)
        parts = torch.split(self._shadow, [b.numel() for b in bufs])
        self._save = K.copy_table(list(zip(parts, bufs)), dev)
        self._restore = K.copy_table(list(zip(bufs, parts)), dev)

    def save_bn(self, model):
        """Head of a guarded step: every running_mean / running_var into the shadow (one launch)."""
        self.attach(model)
        if self._save is not None:
            K.multi_copy(self._save)

    def restore_bn(self):
        """After check(): the shadow back into the running statistics if this step is skipped (one launch either way)."""
        if self._restore is not None:
            K.multi_copy(self._restore, self.skip, 1)

    def counts(self):
        """(clipped, skipped) steps so far: one device-to-host read."""
        if self.state is None:
            return self._counts0
        c = self.state[2:4].tolist()
        return int(c[0]), int(c[1])

    def state_dict(self):
        clipped, skipped = self.counts()
        return dict(self.limits(), clipped=clipped, skipped=skipped)

    def load_state_dict(self, sd):
        """Continues the counters of `sd`. The limits stay this guard's own (a resumed run uses the limits it was started with)."""
        self._counts0 = (int(sd['clipped']), int(sd['skipped']))
        if self.state is not None:
            self.state[2:4] = torch.tensor(self._counts0, dtype=torch.int64)

    def __repr__(self):
        return 'GradGuard(max_norm=%r, skip_threshold=%r)' % (self.max_norm, self.skip_threshold)


RULES = {'adamax': 'exp_inf', 'adam': 'exp_avg_sq', 'adamw': 'exp_avg_sq'}   # rule -> the name of its second moment (torch's own)


class ArenaOptimizer:
    """What does not depend on the update rule: the state over the flat arena (exp_avg, the rule's second moment under torch's name for it,
    step counter, average, lr_now), zero_grad, swap_ema, current_lr, the guard's hand-shake and the counter's advance. A rule names itself
    (`rule`, a key of RULES) and launches its kernel in `_update(arena, guard_state)`."""
    rule = None

    def __init__(self, model, lr, betas, eps, weight_decay, ema_decay, schedule, guard, spectral=None):
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.ema_decay = float(ema_decay)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("ema_decay must lie in [0, 1), got %r" % (ema_decay,))
        self.exp_avg = self.step_count = None
        setattr(self, RULES[self.rule], None)
        self.ema = None     # float32 [arena.n_train] when ema_decay > 0: the averaged trainable prefix, in the arena's layout
        self.gscale = None  # device float[1]: 1/world_size after a SUM all-reduce
        self.schedule = schedule   # LrSchedule or None: `lr` itself at every step
        self._sched = None if schedule is None else schedule.struct(self.lr)
        self.lr_now = None  # device float[1] with a schedule: the lr the last step applied
        self.guard = guard  # GradGuard or None: clip / skip decided on the device before the update
        self.spectral = spectral   # spectral.SpectralReg or None: its gradient joins the arena before the guard looks at it
        self._arena = None
        self._swapped = False

    def _state(self):
        arena = self.model.pack()
        if self._arena is not arena:
            dev = arena.params.device
            self.exp_avg = torch.zeros(arena.n_train, dtype=torch.float32, device=dev)
            setattr(self, RULES[self.rule], torch.zeros(arena.n_train, dtype=torch.float32, device=dev))
            self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
            if self.ema_decay > 0.0:
                self.ema = arena.params[:arena.n_train].detach().clone()
            if self.schedule is not None:
                self.lr_now = torch.zeros(1, dtype=torch.float32, device=dev)
            self._arena = arena
        return arena

    def zero_grad(self, set_to_none=False):
        self._state().zero_grad()

    def step(self):
        """One update of the trainable prefix. With a schedule the lr is the schedule's at the device step counter and the lr applied is left
        in lr_now. With a guard the step runs under the guard's decision for this gradient (engine.TrainStep has taken it by now; taken here
        otherwise), and a skipped step leaves the step counter where it is."""
        arena = self._state()
        if self._swapped:
            raise RuntimeError("%s.step() inside swap_ema(): the parameters hold the average" % type(self).__name__)
        guard, sr = self.guard, self.spectral
        if sr is not None and not sr.open and not sr.done:
            sr.step(self.model, self.gscale, guarded=guard is not None)   # (engine.TrainStep has run it by now; run here otherwise)
        if guard is None:
            if sr is not None:
                if sr.open:
                    sr.finish()
                sr.done = False   # this step's penalty is in the gradient, once: the next step() takes its own
            self._update(arena, None)
            K.counter_advance(self.step_count, 1)
            return
        if not guard.checked:
            guard.check(arena.grads, self.gscale)
        guard.checked = False
        if sr is not None:
            if sr.open:
                sr.finish(guard.skip)
            sr.done = False
        self._update(arena, guard.state)
        K.counter_advance_unless(self.step_count, 1, guard.skip)

    def _update(self, arena, guard_state):
        """The rule's kernel over arena.params[:arena.n_train] and arena.grads; `guard_state` is None or the checked guard's state, whose
        scale then stands in the place of gscale."""
        raise NotImplementedError

    @contextlib.contextmanager
    def swap_ema(self):
        """Inside the context the model computes with the averaged weights: the average and the trainable prefix of the parameter arena are
        exchanged in place (one kernel pass) on entry and exchanged back on exit, so the captured training graph, captured test graphs and
        every parameter view keep their addresses; the transformed-weight cache is told both times. Only trainable parameters are averaged:
        BatchNorm running statistics (buffers) and frozen parameters are used as they are."""
        arena = self._state()
        if self.ema is None:
            raise RuntimeError("this optimizer keeps no average (ema_decay = 0)")
        if self._swapped:
            raise RuntimeError("swap_ema() is not re-entrant")
        live = arena.params[:arena.n_train]
        K.swap(live, self.ema)
        K.prepared.weights_written()
        self._swapped = True
        try:
            yield self
        finally:
            K.swap(live, self.ema)
            K.prepared.weights_written()
            self._swapped = False

    def state_dict(self):
        self._state()
        second = RULES[self.rule]
        sd = {'rule': self.rule, 'exp_avg': self.exp_avg, second: getattr(self, second), 'step': self.step_count, 'lr': self.lr,
              'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay}
        if self.ema is not None:
            sd['ema'], sd['ema_decay'] = self.ema, self.ema_decay
        sd['schedule'] = None if self.schedule is None else self.schedule.state_dict()
        return sd

    def current_lr(self):
        """The lr the last step applied: `lr` itself without a schedule, else a device-to-host read of lr_now (0 before this optimizer's
        first step)."""
        if self.schedule is None:
            return self.lr
        self._state()
        return float(self.lr_now.item())

    def load_state_dict(self, sd):
        """The state of `state_dict()`. A dict without 'rule' is Adamax's; adam and adamw share their state; a second moment of the other
        kind (exp_inf against exp_avg_sq) is refused."""
        second = check_rule(sd.get('rule', 'adamax'), self.rule)
        self._state()
        self.exp_avg.copy_(sd['exp_avg'])
        getattr(self, second).copy_(sd[second])
        self.step_count.copy_(sd['step'])
        if self.ema is not None and 'ema' in sd:
            self.ema.copy_(sd['ema'])


def check_rule(was, now):
    """The name of the second moment that state written under the rule `was` and an optimizer of the rule `now` share; ValueError naming
    both rules when they keep different ones."""
    if was not in RULES:
        raise ValueError("unknown update rule %r in the saved state (one of %s)" % (was, ', '.join(RULES)))
    if RULES[was] != RULES[now]:
        raise ValueError("the saved state is %s's (second moment %s); this optimizer runs %s (second moment %s)"
                         % (was, RULES[was], now, RULES[now]))
    return RULES[now]


class Adamax(ArenaOptimizer):
    """torch.optim.Adamax with L2 decay, the reference's rule."""
    rule = 'adamax'

    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, ema_decay=0.0, schedule=None, guard=None,
                 spectral=None):
        super().__init__(model, lr, betas, eps, weight_decay, ema_decay, schedule, guard, spectral)

    def _update(self, arena, guard_state):
        p, b1, b2 = arena.params[:arena.n_train], self.betas[0], self.betas[1]
        if guard_state is not None:
            K.adamax_guarded_step(p, arena.grads, self.exp_avg, self.exp_inf, None, self.lr, self._sched, b1, b2, self.eps,
                                  self.weight_decay, self.step_count, self.ema, self.ema_decay, self.lr_now, guard_state)
        elif self.schedule is not None:
            K.adamax_sched_step(p, arena.grads, self.exp_avg, self.exp_inf, None, self._sched, b1, b2, self.eps, self.weight_decay,
                                self.gscale, self.step_count, self.ema, self.ema_decay, self.lr_now)
        elif self.ema is None:
            K.adamax_step(p, arena.grads, self.exp_avg, self.exp_inf, None, self.lr, b1, b2, self.eps, self.weight_decay, self.gscale,
                          self.step_count)
        else:
            K.adamax_ema_step(p, arena.grads, self.exp_avg, self.exp_inf, None, self.lr, b1, b2, self.eps, self.weight_decay, self.gscale,
                              self.step_count, self.ema, self.ema_decay)


class Adam(ArenaOptimizer):
    """torch.optim.Adam over the arena (single-tensor form, no amsgrad): `weight_decay` is L2 decay added to the gradient, or with
    `decoupled_weight_decay` torch.optim.AdamW's p *= 1 - lr * weight_decay. Decay applies to every trainable element. One kernel for every
    combination of average, schedule and guard (lvae_adam_step_f32); the bias corrections are formed in double on the device."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False, ema_decay=0.0,
                 schedule=None, guard=None, spectral=None):
        self.decoupled = bool(decoupled_weight_decay)
        self.rule = 'adamw' if self.decoupled else 'adam'
        if not float(lr) >= 0.0:
            raise ValueError("lr must not be negative, got %r" % (lr,))
        if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
            raise ValueError("betas must be two numbers in [0, 1), got %r" % (betas,))
        if not float(eps) >= 0.0:
            raise ValueError("eps must not be negative, got %r" % (eps,))
        if not float(weight_decay) >= 0.0:
            raise ValueError("weight_decay must not be negative, got %r" % (weight_decay,))
        super().__init__(model, lr, betas, eps, weight_decay, ema_decay, schedule, guard, spectral)

    def _update(self, arena, guard_state):
        K.adam_step(arena.params[:arena.n_train], arena.grads, self.exp_avg, self.exp_avg_sq, None, self.lr, self._sched, self.betas[0],
                    self.betas[1], self.eps, self.weight_decay, self.decoupled, None if guard_state is not None else self.gscale,
                    self.step_count, self.ema, self.ema_decay, self.lr_now, guard_state)


class AdamW(Adam):
    """Adam with decoupled decay and torch.optim.AdamW's default of 1e-2."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True, ema_decay=0.0,
                 schedule=None, guard=None, spectral=None):
        super().__init__(model, lr, betas, eps, weight_decay, decoupled_weight_decay, ema_decay, schedule, guard, spectral)
