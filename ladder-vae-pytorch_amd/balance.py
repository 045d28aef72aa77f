"""KL balancing (NVAE, §3.2): during the KL warm-up the per-layer KL terms of the objective are reweighted so that a layer whose KL is
small is left alone and a layer whose KL is large pays more; the coefficients average 1 and are exactly 1 once beta has reached 1.

    m_l     = mean_n |kl[l][n]| + 0.01
    gamma_l = (m_l / alpha_l) / mean_j (m_j / alpha_j)      while beta < 1, else 1
    kl_loss = sum_l gamma_l * mean_n c(kl[l][n])            c: the free-bits clamp; gamma is a constant of the gradient

Everything is decided on the device inside the step's own forward pass (kernels.kl_balance_fwd, ops.KlBalanceFn), from the beta the loss
head uses: a captured step replays with the coefficients of the step it runs. `KlBalance` holds the fixed weights alpha_l and the beta
source; `LadderVAE.kl_balance` takes it, `engine.forward_pass(kl_balance=)` / `engine.TrainStep(kl_balance=)` bind it.
"""
import math

import torch

RULES = ('equal', 'sqrt', 'linear', 'square')


def latent_ratios(downsample):
    """(r, g) per layer, bottom layer first, from a model's `downsample` list: r_l is the layer's latent height over the smallest latent
    height of the model (bottom-up layer j halves the height downsample[j] times before its output meets the latent of layer j, so the
    layers above l decide it: r_l = 2 ** sum(downsample[l + 1:])), g_l the number of layers with the latent size of layer l."""
    ds = [int(d) for d in downsample]
    r = [2 ** sum(ds[l + 1:]) for l in range(len(ds))]
    return r, [r.count(v) for v in r]


def alpha_table(rule, downsample):
    """The fixed weights alpha_l of a named rule, divided by their minimum (floats, bottom layer first): equal 1, sqrt sqrt(r_l),
    linear r_l, square r_l^2 / g_l (NVAE's choice: what gets balanced is the KL per latent dimension)."""
    if rule not in RULES:
        raise ValueError("the KL-balancing rule must be one of %s, got %r" % (', '.join(RULES), rule))
    r, g = latent_ratios(downsample)
    a = {'equal': [1.0 for _ in r], 'sqrt': [math.sqrt(v) for v in r], 'linear': [float(v) for v in r],
         'square': [float(v) ** 2 / n for v, n in zip(r, g)]}[rule]
    lo = min(a)
    return [v / lo for v in a]


def check_alpha(alpha, n_layers):
    """The explicit list as floats; ValueError for a wrong length or an entry that is not a positive finite number."""
    try:
        a = [float(v) for v in alpha]
    except (TypeError, ValueError):
        raise ValueError("the KL-balancing weights must be a rule (%s) or a list of numbers, got %r" % (', '.join(RULES), alpha))
    if len(a) != int(n_layers):
        raise ValueError("%d KL-balancing weights for a model of %d stochastic layers" % (len(a), n_layers))
    for i, v in enumerate(a):
        f = float(torch.tensor(v, dtype=torch.float32)) if math.isfinite(v) else v   # (the kernel divides by the float32)
        if not (v > 0.0 and math.isfinite(v) and f > 0.0 and math.isfinite(f)):
            raise ValueError("KL-balancing weight %d must be positive and finite (as a float32 too), got %r" % (i, v))
    return a


class KlBalance:
    """alpha: 'equal' | 'sqrt' | 'linear' | 'square' (derived from the model's downsample list at attach()) or a list of L positive finite
    numbers, bottom layer first."""

    def __init__(self, alpha='square'):
        if isinstance(alpha, str):
            if alpha not in RULES:
                raise ValueError("the KL-balancing rule must be one of %s, got %r" % (', '.join(RULES), alpha))
            self.rule, self.values = alpha, None
        else:
            self.rule, self.values = None, list(alpha)
        self._key = None
        self.alpha = None        # device float[L]
        self.coeff = None        # device float[L]: the coefficients of the latest training forward
        self.beta = 1.0          # the beta source: a constant, or (step, anneal_steps) read on the device
        self.step = None
        self.anneal_steps = 0

    def record(self):
        """What a checkpoint notes: the rule's name or the list."""
        return self.rule if self.rule is not None else [float(v) for v in self.values]

    def host_alpha(self, model):
        """The weights for `model` as a list of floats (validated; no device is touched)."""
        if self.rule is not None:
            return check_alpha(alpha_table(self.rule, model.downsample), model.n_layers)
        return check_alpha(self.values, model.n_layers)

    def attach(self, model):
        """Builds the device weights for `model` (again only if the model's layers or device changed). Every allocation and host-to-device
        copy happens here, before a step is captured."""
        dev = next(model.parameters()).device
        key = (id(model), dev, tuple(int(d) for d in model.downsample))
        if key != self._key:
            a = self.host_alpha(model)
            self.alpha = torch.tensor(a, dtype=torch.float32).to(dev)
            self.coeff = torch.ones(len(a), dtype=torch.float32).to(dev)
            self._key = key
        return self

    def bind(self, beta=None, step=None, anneal_steps=0):
        """The beta that decides whether the rule is active: bind(beta=b), a constant, or bind(step=counter, anneal_steps=n),
        linear_anneal(counter[0], 0, 1, n) read on the device (engine.global_step_counter). No device work."""
        if (beta is None) == (step is None):
            raise ValueError("bind(beta=...) or bind(step=..., anneal_steps=...), one of the two")
        if step is not None:
            self.beta, self.step, self.anneal_steps = 1.0, step, int(anneal_steps)
        else:
            self.beta, self.step, self.anneal_steps = float(beta), None, 0
        return self

    def beta_source(self):
        """The keywords of kernels.kl_balance_fwd."""
        if self.alpha is None:
            raise RuntimeError("KlBalance: attach(model) first")
        return {'beta': self.beta, 'step': self.step, 'anneal_steps': self.anneal_steps}

    def __repr__(self):
        return 'KlBalance(alpha=%r)' % (self.record(),)


def klb_suffix(coeff, active):
    """What --kl-balance appends to a train line: the smallest and largest coefficient of the step the line falls due at, or `off` once
    beta has reached 1."""
    if not active:
        return '   klb: off'
    return '   klb: {:.3g}..{:.3g}'.format(min(coeff), max(coeff))
