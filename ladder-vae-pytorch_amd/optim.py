"""Adamax over the flat parameter arena — one kernel per step instead of torch.optim.Adamax's per-tensor loop
(experiment/experiment_manager.py:76-81: lr 3e-4, betas (0.9, 0.999), eps 1e-8, L2 weight decay added to the grad).

With `ema_decay > 0` the same kernel pass also keeps an exponential moving average of the weights (`self.ema`), the weights a test
ELBO / importance-weighted bound is normally reported from; `swap_ema()` puts it in the parameters' place for a test pass.
"""
import contextlib

import numpy as np
import torch

from . import kernels as K


def ema_decay_at(decay, n):
    """The decay the kernel applies at the step that follows `n` completed ones: min(decay, (1 + n) / (10 + n)), every operation in fp32
    as on the device (lvae_adamax_ema_step_f32). Returns a numpy float32."""
    f = np.float32
    n = f(n)
    return min(f(decay), (f(1) + n) / (f(10) + n))


class Adamax:
    def __init__(self, model, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, ema_decay=0.0):
        self.model = model
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.ema_decay = float(ema_decay)
        if not 0.0 <= self.ema_decay < 1.0:
            raise ValueError("ema_decay must lie in [0, 1), got %r" % (ema_decay,))
        self.exp_avg = self.exp_inf = self.step_count = None
        self.ema = None     # float32 [arena.n_train] when ema_decay > 0: the averaged trainable prefix, in the arena's layout
        self.gscale = None  # device float[1]: 1/world_size after a SUM all-reduce
        self._arena = None
        self._swapped = False

    def _state(self):
        arena = self.model.pack()
        if self._arena is not arena:
            dev = arena.params.device
            self.exp_avg = torch.zeros(arena.n_train, dtype=torch.float32, device=dev)
            self.exp_inf = torch.zeros(arena.n_train, dtype=torch.float32, device=dev)
            self.step_count = torch.zeros(1, dtype=torch.int64, device=dev)
            if self.ema_decay > 0.0:
                self.ema = arena.params[:arena.n_train].detach().clone()
            self._arena = arena
        return arena

    def zero_grad(self, set_to_none=False):
        self._state().zero_grad()

    def step(self):
        arena = self._state()
        if self.ema is None:
            K.adamax_step(arena.params[:arena.n_train], arena.grads, self.exp_avg, self.exp_inf, None, self.lr, self.betas[0],
                          self.betas[1], self.eps, self.weight_decay, self.gscale, self.step_count)
        else:
            if self._swapped:
                raise RuntimeError("Adamax.step() inside swap_ema(): the parameters hold the average")
            K.adamax_ema_step(arena.params[:arena.n_train], arena.grads, self.exp_avg, self.exp_inf, None, self.lr, self.betas[0],
                              self.betas[1], self.eps, self.weight_decay, self.gscale, self.step_count, self.ema, self.ema_decay)
        K.counter_advance(self.step_count, 1)

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
        sd = {'exp_avg': self.exp_avg, 'exp_inf': self.exp_inf, 'step': self.step_count, 'lr': self.lr,
              'betas': self.betas, 'eps': self.eps, 'weight_decay': self.weight_decay}
        if self.ema is not None:
            sd['ema'], sd['ema_decay'] = self.ema, self.ema_decay
        return sd

    def load_state_dict(self, sd):
        self._state()
        self.exp_avg.copy_(sd['exp_avg'])
        self.exp_inf.copy_(sd['exp_inf'])
        self.step_count.copy_(sd['step'])
        if self.ema is not None and 'ema' in sd:
            self.ema.copy_(sd['ema'])
