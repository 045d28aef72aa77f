"""Spectral regularisation of the convolution weights (NVAE, §3.2): the penalty lam * sum_i sigma_i over every trainable
`Conv2dParams.weight`, sigma_i the largest singular value of the weight as it lies in the arena (a [KH*KW*Cin][Cout] matrix), estimated by
one power-iteration step per optimizer step from a persistent u_i (torch.nn.utils.spectral_norm's rule) and differentiated with u', v' held
constant: the step adds (lam / gscale) v' u'^T into the weight's gradient slot. One launch over a device table of all matrices
(kernels.spectral_step), a second small one for the two numbers a train line prints (kernels.spectral_reduce); both captured with the step.

`SpectralReg` is handed to the optimizer (`ArenaOptimizer(..., spectral=)`); `engine.TrainStep` runs `step()` immediately before the guard's
check / the summary fold and `finish()` right after the guard has decided. Under a guard the step writes u', v', sigma into a twin buffer
that `finish()` commits only when the step is applied (lvae_multi_copy_f32 with want = 0 on the skip flag), so a skipped step leaves them
bit for bit. `spectral_norms(model)` is the offline report.
"""
import torch

from . import kernels as K
from .lib.nn import Conv2dParams

COMMIT_CHUNK = 8192   # floats per entry of the commit table: one workgroup of lvae_multi_copy_f32 each


def conv_matrices(model, arena, trainable_only=True):
    """[(parameter name, param offset, grad offset, K, Cout)] of every Conv2dParams.weight of `model` in `arena` (a ParamArena, on any
    device), in the arena's order, each weight once. The matrix view of a slot is arena.params[off:off + K * Cout].view(K, Cout): rows
    (kh, kw, cin), columns cout, plain and transposed convolutions alike. trainable_only: frozen weights (no gradient slot) are left out;
    otherwise their grad offset is -1."""
    convs = {}
    for mod in model.modules():
        if isinstance(mod, Conv2dParams):
            convs[id(mod.weight)] = mod
    named = dict(model.named_parameters())
    rows = []
    for name in arena.names:
        p = named[name]
        mod = convs.get(id(p))
        if mod is None or (trainable_only and not p.requires_grad):
            continue
        off, n = arena.slots[name]
        cout = int(mod.c_out)
        k = n // cout
        assert k * cout == n and k == mod.kernel * mod.kernel * mod.c_in, (name, n, cout)
        rows.append((name, off, off if p.requires_grad else -1, k, cout))
    return rows


def initial_u(seed, entry, cout):
    """The u an entry starts from: a unit vector drawn from a host generator that depends on the seed and the entry's number only (every
    rank holds the same vectors), normalised in float64 and rounded once."""
    g = torch.Generator().manual_seed((int(seed) * 1000003 + int(entry)) % (2 ** 63 - 1))
    u = torch.randn(int(cout), generator=g, dtype=torch.float64)
    return (u / u.norm().clamp_min(1e-12)).float()


class SpectralReg:
    """lam * sum of the convolutions' spectral norms. lam: the penalty's weight (>= 0, finite; 0 still iterates and reports, adding a zero
    gradient). warm_iters: iterate-only launches after the initial u is drawn, so that the first steps do not regularise towards a random
    direction. seed: of the initial u."""

    def __init__(self, lam, warm_iters=10, seed=0):
        lam = float(lam)
        if not (lam >= 0.0 and lam != float('inf')):
            raise ValueError("the spectral penalty's weight must be finite and not negative, got %r" % (lam,))
        if int(warm_iters) < 0:
            raise ValueError("warm_iters must not be negative, got %r" % (warm_iters,))
        self.lam, self.warm_iters, self.seed = lam, int(warm_iters), int(seed)
        self.names = self.shapes = self.table = None
        self.state = self.u = self.v = self.sigma = None     # one flat buffer [u | v | sigma] and its three views
        self.twin = self._twin_views = self._commit = None   # the same layout again: what a guarded step writes before it is committed
        self.metrics = None                                  # device float[2]: sum and max of sigma
        self._arena = self._key = None
        self._loaded = None
        self.open = False                                    # step() ran, finish() has not
        self.done = False                                    # step() and finish() ran for the gradient the optimizer is about to apply
        self._guarded = False

    # ---- state ----------------------------------------------------------------------------------------------------------------------
    def attach(self, model):
        """Builds the table from model.pack() and allocates u, v, sigma (again if the arena moved; the iterate is kept when the matrices
        are the same). A fresh iterate is the seeded u after `warm_iters` iterate-only launches, or the state of load_state_dict()."""
        arena = model.pack()
        if self.build(model, arena) and self._loaded is None:
            for _ in range(self.warm_iters):
                self.iterate()
        elif self._loaded is not None:
            self._take_loaded()
        return self

    def build(self, model, arena):
        """The host part of attach(), on an arena on any device: the table, and a fresh seeded iterate unless the one held belongs to the
        same matrices. -> whether the iterate is fresh (and wants its warm start)."""
        key = (id(arena), arena.params.data_ptr(), arena.grads.data_ptr())
        if key == self._key:
            return False
        rows = conv_matrices(model, arena)
        if not rows:
            raise ValueError("the model has no trainable convolution weight to regularise")
        dev = arena.params.device
        shapes = [(r[3], r[4]) for r in rows]
        nu, nv = sum(c for _, c in shapes), sum(k for k, _ in shapes)
        table, uo, vo = [], 0, 0
        for _, poff, goff, k, c in rows:
            table.append((poff, goff, k, c, uo, vo))
            uo, vo = uo + c, vo + k
        self.table = K.spectral_table(table, dev)
        fresh = self.shapes != shapes or self.state is None or self.state.device != dev
        self.names, self.shapes, self._arena, self._key = [r[0] for r in rows], shapes, arena, key
        if fresh:
            self.state = torch.zeros(nu + nv + len(rows), dtype=torch.float32, device=dev)
            self.u, self.v, self.sigma = self.state[:nu], self.state[nu:nu + nv], self.state[nu + nv:]
            self.twin = self._twin_views = self._commit = None
            self.metrics = torch.zeros(2, dtype=torch.float32, device=dev)
            self.u.copy_(torch.cat([initial_u(self.seed, i, c) for i, (_, c) in enumerate(shapes)]))
        return fresh

    def prepare(self, model, guarded=False):
        """Everything a captured step will use exists afterwards: the table and the iterate and, for a guarded step, the twin buffer and its
        commit table (allocations and host-to-device copies, which a capture cannot hold)."""
        self.attach(model)
        if guarded:
            self._twin()
        return self

    def _twin(self):
        if self.twin is None:
            nu, nv = self.u.numel(), self.v.numel()
            self.twin = self.state.clone()   # (an entry the kernel refuses writes nothing: the commit then copies what was there)
            self._twin_views = (self.twin[:nu], self.twin[nu:nu + nv], self.twin[nu + nv:])
            n = self.state.numel()
            self._commit = K.copy_table([(self.state[i:i + COMMIT_CHUNK], self.twin[i:i + COMMIT_CHUNK]) for i in range(0, n, COMMIT_CHUNK)],
                                        self.state.device)
        return self._twin_views

    def iterate(self, max_workgroups=0):
        """One iterate-only launch: u, v, sigma move, no gradient is touched."""
        K.spectral_step(self.table, self._arena.params, None, self.u, self.u, self.v, self.sigma, 0.0, None, max_workgroups)

    # ---- the training step ----------------------------------------------------------------------------------------------------------
    def step(self, model, gscale=None, guarded=False, max_workgroups=0):
        """The power-iteration step and the penalty's gradient into the arena's gradient slots (one launch). guarded: u', v', sigma go
        into the twin buffer; finish(skip) commits them."""
        self.attach(model)
        arena = self._arena
        u, v, s = self._twin() if guarded else (self.u, self.v, self.sigma)
        K.spectral_step(self.table, arena.params, arena.grads, self.u, u, v, s, self.lam, gscale, max_workgroups)
        self.open, self.done = True, False
        self._guarded = guarded

    def finish(self, skip=None):
        """After the guard's decision (skip: its device int32[1] flag; None without a guard): commits a guarded step's iterate unless the
        step is skipped, then folds sigma into `metrics` (sum, max)."""
        if self._guarded:
            if skip is None:
                raise ValueError("a guarded spectral step is committed on the guard's skip flag")
            K.multi_copy(self._commit, skip, 0)
        K.spectral_reduce(self.sigma, self.metrics)
        self.open, self.done = False, True   # optimizer.step() consumes `done`: it neither repeats the step nor leaves it out

    @property
    def sr_sum(self):
        return self.metrics[0]

    @property
    def sr_max(self):
        return self.metrics[1]

    # ---- checkpoints ----------------------------------------------------------------------------------------------------------------
    def state_dict(self):
        if self.state is None:
            raise RuntimeError("SpectralReg.state_dict() before attach(model)")
        return {'lam': self.lam, 'u': self.u.detach().cpu().clone(), 'v': self.v.detach().cpu().clone(),
                'sigma': self.sigma.detach().cpu().clone(), 'shapes': [list(s) for s in self.shapes]}

    def load_state_dict(self, sd):
        """Continues the iterate of `sd` (u, v, sigma). The penalty's weight stays this object's own. Takes effect at the next attach(),
        or at once when an iterate exists. (`metrics` follow at the next finish().)"""
        self._loaded = {k: sd[k] for k in ('u', 'v', 'sigma')}
        self._loaded['shapes'] = [tuple(s) for s in sd['shapes']] if 'shapes' in sd else None
        if self.state is not None:
            self._take_loaded()

    def _take_loaded(self):
        sd, self._loaded = self._loaded, None
        if sd['shapes'] is not None and sd['shapes'] != self.shapes or any(sd[k].numel() != getattr(self, k).numel() for k in ('u', 'v', 'sigma')):
            raise ValueError("the saved spectral state belongs to other convolutions than this model's")
        for k in ('u', 'v', 'sigma'):
            getattr(self, k).copy_(sd[k])

    def __repr__(self):
        return 'SpectralReg(lam=%r, warm_iters=%r, seed=%r)' % (self.lam, self.warm_iters, self.seed)


def spectral_norms(model, n_iters=50, seed=0):
    """{parameter name: sigma} of every convolution weight of the model (frozen ones too), by `n_iters` iterate-only launches from a fresh
    seeded u: the weights as they are in the arena now (inside optimizer.swap_ema(): the averaged ones)."""
    if int(n_iters) < 1:
        raise ValueError("n_iters must be at least 1, got %r" % (n_iters,))
    arena = model.pack()
    rows = conv_matrices(model, arena, trainable_only=False)
    if not rows:
        return {}
    dev = arena.params.device
    table, uo, vo = [], 0, 0
    for _, poff, _, k, c in rows:
        table.append((poff, 0, k, c, uo, vo))
        uo, vo = uo + c, vo + k
    table = K.spectral_table(table, dev)
    u = torch.cat([initial_u(seed, i, r[4]) for i, r in enumerate(rows)]).to(dev)
    v = torch.zeros(vo, dtype=torch.float32, device=dev)
    sigma = torch.zeros(len(rows), dtype=torch.float32, device=dev)
    for _ in range(int(n_iters)):
        K.spectral_step(table, arena.params, None, u, u, v, sigma)
    return {r[0]: float(s) for r, s in zip(rows, sigma.tolist())}
