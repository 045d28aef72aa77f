"""Checkpoint interchange with the reference (SURVEY.md §5 checkpoint row, §8f rank 3).

The reference saves `model.state_dict()` through boilr (absent). The key scheme and tensor shapes of the HIP model are
identical, but its parameters are strided views of one flat arena; `state_dict_reference_layout` returns plain contiguous
CPU tensors in the reference's memory layout, so a file written here loads into the reference's `LadderVAE` with
`load_state_dict` and vice versa. Optimiser state is stored per parameter name (torch.optim.Adamax names: exp_avg,
exp_inf; torch.optim.Adam / AdamW names under those rules: exp_avg, exp_avg_sq) with the rule's name under 'rule', so it can be
re-attached to either implementation. When the optimizer keeps an exponential moving average of the weights, the file
also holds `'ema'`: a second complete state dict of the same keys, shapes and layout whose trainable parameters are the averages (buffers
and frozen parameters as in `'model'`), so the averaged weights load into the reference's `LadderVAE` the same way.
"""
import torch

from .optim import RULES, check_rule


def state_dict_reference_layout(model):
    """{key: contiguous CPU tensor} with the reference's keys, shapes and (row-major) layout."""
    return {k: v.detach().to('cpu').contiguous().clone() for k, v in model.state_dict().items()}


def optimizer_state_by_name(model, optimizer):
    """{'rule': 'adamax' | 'adam' | 'adamw', 'step': int, 'state': {param_name: {'exp_avg', second moment}}} in the parameters' logical
    shapes, the second moment under torch's own name for the rule: 'exp_inf' (Adamax) or 'exp_avg_sq' (Adam, AdamW)."""
    arena = model.pack()
    optimizer._state()
    second = RULES[optimizer.rule]
    out = {}
    named = dict(model.named_parameters())
    for name, (off, n) in arena.slots.items():
        p = named[name]
        if not p.requires_grad:
            continue
        # same strides as the parameter view -> same logical element order
        m = torch.as_strided(optimizer.exp_avg, p.shape, p.stride(), off).detach().cpu().contiguous().clone()
        u = torch.as_strided(getattr(optimizer, second), p.shape, p.stride(), off).detach().cpu().contiguous().clone()
        out[name] = {'exp_avg': m, second: u}
    return {'rule': optimizer.rule, 'step': int(optimizer.step_count.item()), 'state': out, 'lr': optimizer.lr, 'betas': optimizer.betas,
            'eps': optimizer.eps, 'weight_decay': optimizer.weight_decay}


def _ema_views(model, optimizer):
    """{param_name: view of optimizer.ema with the parameter's logical shape} for every trainable parameter."""
    arena = model.pack()
    optimizer._state()
    out = {}
    for name, p in model.named_parameters():
        if p.requires_grad:
            out[name] = torch.as_strided(optimizer.ema, p.shape, p.stride(), arena.slots[name][0])
    return out


def ema_state_dict_reference_layout(model, optimizer):
    """`state_dict_reference_layout(model)` with every trainable parameter replaced by its average (BatchNorm running statistics and frozen
    parameters are not averaged: they are the model's)."""
    sd = state_dict_reference_layout(model)
    for name, v in _ema_views(model, optimizer).items():
        sd[name] = v.detach().to('cpu').contiguous().clone()
    return sd


def noise_state(model):
    """{'seed', 'step'} of the model's on-device Philox stream (None for any other noise source)."""
    from .noise import PhiloxNoise
    nz = getattr(model, 'noise', None)
    if not isinstance(nz, PhiloxNoise):
        return None
    return {'seed': int(nz.seed), 'step': int(nz.step.item()) if nz.step is not None else 0}


def lr_schedule_record(optimizer):
    """What a checkpoint keeps of a scheduled optimizer under 'lr_schedule': LrSchedule's fields and the base lr, plain Python values; None
    without a schedule. A resumed run uses the schedule it was started with (load_checkpoint does not touch it); the record says what the
    file's run used."""
    sched = getattr(optimizer, 'schedule', None)
    return None if sched is None else dict(sched.state_dict(), base_lr=optimizer.lr)


def optimizer_rule_record(ck):
    """The update rule of a loaded file's optimizer state ('adamax' for a file from before there was a second rule); None without one."""
    if not (isinstance(ck, dict) and 'optimizer' in ck):
        return None
    return ck['optimizer'].get('rule', 'adamax')


def rule_warning(path, ck, optimizer):
    """The line a resumed run prints when the file's rule is not the optimizer's own but shares its state (adam <-> adamw: the decay
    differs, the moments do not; the optimizer's rule is the one that runs). None when there is nothing to say."""
    was = optimizer_rule_record(ck)
    if was is None or was == optimizer.rule:
        return None
    return 'warning: %s was written with the update rule %s; continuing with %s' % (path, was, optimizer.rule)


def accum_steps_record(ck):
    """The micro-batches per optimizer step of a loaded file's run: its 'accum_steps', 1 for a file from before there was one (or a bare
    state_dict)."""
    return int(ck.get('accum_steps', 1)) if isinstance(ck, dict) and 'model' in ck else 1


def augment_record(ck):
    """The feed augmentation of a loaded file's run: its 'augment' (FeedAugment.record() plus the data seed under 'seed'); None for a file
    without the key (a run without augmentation, an older file, a bare state_dict)."""
    return ck.get('augment') if isinstance(ck, dict) and 'model' in ck else None


def spectral_record(ck):
    """The 'spectral' entry of a loaded file (SpectralReg.state_dict: lam, u, v, sigma); None for a file without one."""
    return ck.get('spectral') if isinstance(ck, dict) and 'model' in ck else None


def spectral_warning(path, ck, optimizer):
    """The line a resumed run prints when the file's spectral penalty had another weight than the optimizer's own (the command line's is
    the one that runs). None when there is nothing to say: no regulariser here, no entry in the file, or the same weight."""
    sr, was = getattr(optimizer, 'spectral', None), spectral_record(ck)
    if sr is None or was is None or float(was['lam']) == sr.lam:
        return None
    return 'warning: %s was written with --spectral-reg %g; continuing with %g' % (path, float(was['lam']), sr.lam)


def kl_balance_record(ck):
    """The 'kl_balance' note of a loaded file: the rule's name or the list of weights its run balanced the KL terms with; None for a file
    without the key (a run without KL balancing, an older file, a bare state_dict)."""
    return ck.get('kl_balance') if isinstance(ck, dict) and 'model' in ck else None


def kl_balance_warning(path, ck, now):
    """The line a resumed run prints when the file's run balanced its KL terms another way than this one (`now`: this run's rule, list or
    None; the command line's setting is the one that runs). None when they agree."""
    was = kl_balance_record(ck)
    if was == now:
        return None
    word = lambda r: 'no KL balancing' if r is None else '--kl-balance %s' % (r,)
    return 'warning: %s was written with %s; continuing with %s' % (path, word(was), word(now))


def recalibrated_bn_buffers(model, optimizer, bn_recal):
    """{key: CPU tensor} of every BatchNorm running_mean / running_var recalibrated for the AVERAGED weights on the batches bn_recal()
    returns (recalibrate.recalibrated inside optimizer.swap_ema(), as a test pass under --ema-bn-batches does it): the parameters and the
    live statistics are back, bit for bit, on return."""
    from .lib.nn import BatchNorm2dParams
    from .recalibrate import recalibrated
    with optimizer.swap_ema(), recalibrated(model, bn_recal(), step=model.global_step):
        return {k + '.' + name: getattr(m, name).detach().to('cpu').contiguous().clone()
                for k, m in model.named_modules() if isinstance(m, BatchNorm2dParams) for name in ('running_mean', 'running_var')}


def save_checkpoint(path, model, optimizer=None, summary=None, bn_recal=None):
    """Weights (reference layout), global step, Adamax state and the position of the Philox noise stream, so that a resumed run continues
    the original one bit for bit. With a `summary` (summary.TrainSummary) also 'summary': the open log window's accumulator as a list of
    floats, so that the run resumed in the middle of a window prints the train line of the uninterrupted one. A scheduled lr is a function
    of the Adamax step and of the schedule, stored as 'lr_schedule' (`lr_schedule_record`). 'iw_train_samples' notes the K of the objective
    the run trained on (model.iw_train_samples; 1 = the ELBO), by the same rule: load_checkpoint does not touch the resumed run's own.
    A guarded optimizer adds 'grad_guard' (GradGuard.state_dict: its limits and the cumulative clipped / skipped counts). 'accum_steps' notes
    the micro-batches per optimizer step (model.accum_steps; `accum_steps_record` reads it back, 1 from a file without the key).
    A spectrally regularised optimizer adds 'spectral' (SpectralReg.state_dict: lam and the iterate u, v, sigma), so a resumed run continues
    bit for bit; the resumed run's own lam is the one that runs (`spectral_warning`).
    bn_recal (--ema-bn-batches; a callable returning image batches, used only with an averaging optimizer): the BatchNorm running statistics
    of 'ema' are those recalibrated for the averaged weights (`recalibrated_bn_buffers`), so the dict a reference model loads is
    self-consistent, and 'ema_bn_batches' notes the flag (model.ema_bn_batches). 'model', the optimizer state and a resumed run are untouched.
    'augment' notes what the device-fed gather did to the training batches (model.augment: data.FeedAugment.record() and the seed; absent
    without augmentation). The noise is stateless, so it is a note like 'accum_steps': a resumed run uses its own flags.
    'kl_balance' notes how the run balanced its KL terms (model.kl_balance_record, else the record of model.kl_balance: the rule's name or
    the list; absent without balancing). The coefficients have no state, so nothing else is saved and a resumed run continues bit for bit
    under the same setting; its own setting is the one that runs (`kl_balance_warning`)."""
    ck = {'model': state_dict_reference_layout(model), 'global_step': int(model.global_step)}
    if optimizer is not None:
        ck['optimizer'] = optimizer_state_by_name(model, optimizer)
        if getattr(optimizer, 'ema_decay', 0.0) > 0.0:
            ck['ema'] = ema_state_dict_reference_layout(model, optimizer)
            ck['ema_decay'] = optimizer.ema_decay
            if bn_recal is not None:
                ck['ema'].update(recalibrated_bn_buffers(model, optimizer, bn_recal))
                ck['ema_bn_batches'] = int(getattr(model, 'ema_bn_batches', 0))
        if lr_schedule_record(optimizer) is not None:
            ck['lr_schedule'] = lr_schedule_record(optimizer)
        if getattr(optimizer, 'guard', None) is not None:
            ck['grad_guard'] = optimizer.guard.state_dict()
        if getattr(optimizer, 'spectral', None) is not None:
            ck['spectral'] = optimizer.spectral.attach(model).state_dict()
    ck['iw_train_samples'] = int(getattr(model, 'iw_train_samples', 1))   # what the file's run trained on; a resumed run uses its own flag
    ck['accum_steps'] = int(getattr(model, 'accum_steps', 1))             # micro-batches per optimizer step, by the same rule
    # whether conv_in_q predicts offsets from the prior (model.residual_posterior). The same weights mean a different model under the other
    # setting, so unlike the notes above this one is checked on load (check_residual_posterior)
    ck['residual_posterior'] = bool(getattr(model, 'residual_posterior', False))
    if getattr(model, 'augment', None) is not None:
        ck['augment'] = dict(model.augment)   # the feed's augmentation and its seed; a file without the key means none
    klb = getattr(model, 'kl_balance_record', None)
    if klb is None and getattr(model, 'kl_balance', None) is not None:
        klb = model.kl_balance.record()
    if klb is not None:
        ck['kl_balance'] = klb
    nz = noise_state(model)
    if nz is not None:
        ck['noise'] = nz
    if getattr(model, 'global_step_dev', None) is not None:
        ck['global_step_dev'] = int(model.global_step_dev.item())
    tn = getattr(model, 'test_noise', None)
    if tn is not None and getattr(tn, 'step', None) is not None:
        ck['test_noise'] = {'step': int(tn.step.item())}   # where the test passes' own stream stands: resumed test lines repeat exactly
    if summary is not None:
        ck['summary'] = summary.state()
    torch.save(ck, path)


def residual_posterior_record(ck):
    """Whether the file's weights parameterise posteriors relative to the prior; a file without the note (an older one, a bare state_dict)
    is absolute."""
    return bool(ck.get('residual_posterior', False)) if isinstance(ck, dict) and 'model' in ck else False


def check_residual_posterior(path, ck, model):
    """ValueError naming both settings unless the model reads conv_in_q's output the way the file's run did."""
    word = lambda r: 'residual (--residual-posterior: offsets from the prior)' if r else 'absolute (no --residual-posterior)'
    was, now = residual_posterior_record(ck), bool(getattr(model, 'residual_posterior', False))
    if was != now:
        raise ValueError("%s was written by a model whose posteriors are %s; this model's are %s. The same weights mean a different model "
                         "under the other setting: set the flag as the file's run did" % (path, word(was), word(now)))


def load_checkpoint(path, model, optimizer=None, summary=None):
    """Loads a file written by `save_checkpoint` (with the noise stream's position and the device global-step counter when it holds
    them), or a bare reference `state_dict` file. Load before a TrainStep captures its graph: the graph keeps the counters it saw.
    An averaging optimizer gets its average from the file's 'ema'; from a file without one the average starts at the loaded weights.
    A `summary` gets the file's open log window; from a file without one it starts an empty window. A guarded optimizer continues the
    file's clipped / skipped counts under its own limits; from a file without 'grad_guard' it keeps the counts it has. The optimizer
    state must be of the optimizer's own kind: adam and adamw share theirs (`rule_warning` has the line to print), a file without 'rule'
    is Adamax's, and exp_inf against exp_avg_sq is a ValueError naming both rules, raised before anything is loaded."""
    ck = torch.load(path, map_location='cpu')
    sd = ck['model'] if isinstance(ck, dict) and 'model' in ck else ck
    check_residual_posterior(path, ck, model)   # (a mismatching 'residual_posterior' note is refused before anything is loaded)
    second = None
    if optimizer is not None and isinstance(ck, dict) and 'optimizer' in ck:
        second = check_rule(optimizer_rule_record(ck), optimizer.rule)   # (refused before anything is loaded)
    model.load_state_dict(sd)
    if isinstance(ck, dict) and 'model' in ck:
        model.global_step = int(ck.get('global_step', model.global_step))
        from .noise import PhiloxNoise
        if 'noise' in ck and isinstance(getattr(model, 'noise', None), PhiloxNoise):
            dev = next(model.parameters()).device
            model.noise.seed = int(ck['noise']['seed'])
            model.noise.step = torch.full((1,), int(ck['noise']['step']), dtype=torch.int64, device=dev)
        if 'test_noise' in ck:
            model.test_noise_start = int(ck['test_noise']['step'])   # evaluate.test_pass starts its own stream there
        if getattr(model, 'global_step_dev', None) is not None or 'global_step_dev' in ck:
            dev = next(model.parameters()).device
            model.global_step_dev = torch.full((1,), int(ck.get('global_step_dev', model.global_step)), dtype=torch.int64, device=dev)
    if optimizer is not None and isinstance(ck, dict) and 'optimizer' in ck:
        arena = model.pack()
        optimizer._state()
        named = dict(model.named_parameters())
        for name, st in ck['optimizer']['state'].items():
            off, n = arena.slots[name]
            p = named[name]
            torch.as_strided(optimizer.exp_avg, p.shape, p.stride(), off).copy_(st['exp_avg'])
            torch.as_strided(getattr(optimizer, second), p.shape, p.stride(), off).copy_(st[second])
        optimizer.step_count.fill_(int(ck['optimizer']['step']))
    if optimizer is not None and getattr(optimizer, 'ema_decay', 0.0) > 0.0:
        arena = model.pack()
        optimizer._state()
        if isinstance(ck, dict) and 'model' in ck and 'ema' in ck:
            for name, view in _ema_views(model, optimizer).items():
                view.copy_(ck['ema'][name])
        else:
            optimizer.ema.copy_(arena.params[:arena.n_train])
    if optimizer is not None and getattr(optimizer, 'guard', None) is not None and isinstance(ck, dict) and 'grad_guard' in ck:
        optimizer.guard.load_state_dict(ck['grad_guard'])
    if optimizer is not None and getattr(optimizer, 'spectral', None) is not None and spectral_record(ck) is not None:
        optimizer.spectral.load_state_dict(ck['spectral'])   # (a file without the entry: the iterate warm-starts afresh on attach)
    if summary is not None:
        if isinstance(ck, dict) and 'model' in ck and 'summary' in ck:
            summary.load_state(ck['summary'])
        else:
            summary.load_state([0.0] * summary.acc.numel())
    return ck


def load_ema_weights(path, model):
    """Loads the AVERAGED weights of a file written by `save_checkpoint` into the model (offline evaluation of the average). A file without
    'ema' (an averaging-free run, an older file, a bare state_dict) is refused."""
    ck = torch.load(path, map_location='cpu')
    if not (isinstance(ck, dict) and 'model' in ck and 'ema' in ck):
        raise ValueError("%s holds no averaged weights (no 'ema' entry): it was not written by a run with --ema-decay > 0" % path)
    check_residual_posterior(path, ck, model)
    model.load_state_dict(ck['ema'])
    model.global_step = int(ck.get('global_step', model.global_step))
    return ck
