"""Offline evaluation on the HIP engine — the numerical part of the reference's evaluate.py:20-114 (whose loop lives in
the absent boilr.eval.BaseOfflineEvaluator / VAEExperimentManager.test_procedure; restated):

  * `iw_log_likelihood(model, x, S)`  — importance-weighted bound log (1/S) sum_s p(x, z_s)/q(z_s|x), per image.
    In eval mode the bottom-up pass has no noise, so it is run ONCE per batch and only top-down + likelihood are
    replayed S times (saves the 26.5 % bottom-up share of forward FLOPs per extra sample);
  * `evaluate(model, batches, S, world)` — mean ELBO / IW bound over a data set, sharded over ranks, one all-reduce;
  * `test_pass(model, batches, S)` — the reference's test summaries (ELBO, recons, KL, per-layer KL, IW bound), folded on the device
    into double totals, on a noise stream of its own: the trainer's test / log-likelihood pass, which leaves training untouched
    (with `optimizer=` an averaging Adamax: computed from the averaged weights);
  * `prior_samples(model, n)` and `inspect_layer_repr(model, n)` — evaluate.py:34-45, 95-114, as arrays;
  * `reconstructions(model, x)` — inputs beside what the model makes of them (boilr's generate_and_save_reconstructions, restated);
  * `conditional_samples(model, x, k, K)` — K variations per image that keep its top k latents (LadderVAE.sample_conditional);
  * `interpolations(model, x_a, x_b, T, k, mode)` — T steps between two images in the latents of their top k layers, spherical or linear
    (LadderVAE.interpolate);
  * `make_mask(kind, frac, shape, seed)` and `inpaintings(model, x, mask, n_iters, init, final)` — a mask of observed pixels on the host,
    and the images completed under it by the pseudo-Gibbs chain (LadderVAE.inpaint);
  * `nearest_neighbours(model, table, queries, k, space)` — query images beside their nearest table images, in the pixels or in the latents
    of the top k layers (neighbours.py), and how close samples lie to the table against how close held-out images do;
  * `reconstruction_quality(model, batches)` and `quality_ladder(model, batches, temperature)` — mse, PSNR and SSIM of reconstructions,
    and of images rebuilt from the posterior means of their top k layers for every k, measured on the device (quality.py);
  * `image_pass(model, nrows, x, step)` — the trainer's pictures (--ts-img-every): a grid of prior samples and a grid of input /
    reconstruction pairs, formed on the device (images.py), on a noise stream of their own, leaving training untouched.

CLI: python -m lvae_amd.evaluate --synthetic --ll --ll-samples 100 --ps --layer-repr --recons --img-dir DIR  <model flags of main.py>
     --ps and --layer-repr write prior_samples.npy and layer_repr_<i>.npy; with --img-dir DIR they also write the reference's pictures
     DIR/samples_0.png and DIR/sample_mode_layer<i>.png (grids of 12 x 12), and --recons writes DIR/reconstructions.png (72 pairs).
     --cond-samples [--cond-layers k ...] [--cond-variations K] writes cond_samples_top<k>.npy (n, 1 + K, C, H, W) for the first 12
     evaluation images, column 0 the input, and with --img-dir DIR/cond_samples_top<k>.png (one row per image).
     --interp [--interp-layers k ...] [--interp-steps T] [--interp-mode slerp|lerp] writes interp_top<k>.npy (pairs, T + 2, C, H, W) for the
     pairs (2i, 2i + 1) of the first 24 evaluation images: column 0 is x_a, columns 1..T the steps, the last column x_b; with --img-dir
     DIR/interp_top<k>.png (one row per pair). k defaults to the number of layers.
     --inpaint [--inpaint-mask KIND ...] [--inpaint-frac F] [--inpaint-iters N] [--inpaint-init zeros|mean|noise] [--inpaint-final
     sample|mean] writes inpaint_<kind>.npy (n, 3, C, H, W) for the first 12 evaluation images: the image, what the model was shown (the
     missing pixels at 0.5) and the completion; with --img-dir DIR/inpaint_<kind>.png (one row per image). KIND: left, right, top, bottom
     (that strip is hidden), center (a box), random (each pixel with probability F). One line per kind: the mean squared error on the
     missing pixels of the initial fill and of the completion, and the mean ll of the observed pixels in the first and the last round.
     --nn [--nn-k K] [--nn-space pixel|latent] [--nn-layers k] [--nn-table FILE.npz | --nn-table-size N] writes, for 12 prior samples and
     for the first 12 evaluation images, nn_<space>_<samples|heldout>.npy (12, 1 + K, C, H, W): column 0 the query, then its K nearest
     table images (exact squared L2 search on the device, neighbours.NeighbourIndex), with nn_<...>_index.npy and nn_<...>_dist.npy
     (12, K); with --img-dir DIR/nn_<...>.png (one row per query). One line: neighbours.closeness_summary over 144 samples and up to
     1000 evaluation images. The table is key 'data' of FILE.npz, or N synthetic images drawn from seed + 1.
     --temperature T [T ...] (one value, or one per layer, bottom first) tempers the prior draws of --ps, --cond-samples and --interp.
     --recons also prints the mean squared error, PSNR and SSIM of the reconstructions of ALL evaluation images; --inpaint's line ends in
     the PSNR on the missing pixels and the SSIM at missing centres of the initial fill and of the completion; --ll --image-quality ends
     the test line in PSNR and SSIM (quality.py: all measured on the device).
     --quality-ladder [--temperature T] prints, for every k from 0 to L, mse, PSNR and SSIM of the images rebuilt from the posterior means
     of their top k layers with the layers below at the prior (T = 0 by default: its mean), and writes quality_ladder.npy (L + 1, 3).
     --recalibrate-bn data|prior [--recalibrate-batches N] re-estimates the BatchNorm running statistics once, before any output, for the
     weights that were loaded (recalibrate.recalibrate_bn): on the first N (default 20) batches of --batch-size training images, or on N
     train-mode top-down passes from the prior at --temperature (one value). One header line says which.
"""
import contextlib
import os

import numpy as np
import torch

from . import kernels as K
from . import ops
from .passes import eval_mode, replay_loop


def _test_bottom_up(model, x):
    """Eval-mode bottom-up of one NCHW batch (no noise drawn; sample independent, so once per batch) -> (bottom-up values, NHWC image
    for the likelihood)."""
    model._begin(x)
    bu_values, x_nhwc, _ = model._encode_image(x)
    model.noise.end()
    return bu_values, x_nhwc


def _elbo_sample(model, bu_values, x_nhwc, zero, latent_stats=None, image_quality=None):
    """One top-down sample of an evaluation pass: noise.begin, top-down pass, crop, likelihood, KL bookkeeping -> (elbo_sep, ll, kl_sep,
    kl_avg), per image. The caller folds them into its running state (iw_online or eval_online: they accumulate in different precisions)
    and then calls model.noise.end(). With latent_stats (a latent.LatentStats) every stochastic layer also folds its p and q parameters
    into it; the noise drawn is the same either way. With image_quality (a quality.ImageQuality) the head's mean, or its sample where it has
    no mean (the order of `reconstructions`), is judged against x and folded into it, both as they lie here: cropped, channel-last, the
    Gaussian head's mean as the strided view of its parameters (no copy)."""
    model.noise.begin(x_nhwc.device)                 # every sample: same call sites, next RNG step
    out, td = model._topdown(bu_values, latent_stats=latent_stats)
    ll, head = model.likelihood(model._crop(out, x_nhwc.shape[1:3]), x_nhwc, model.noise)
    if image_quality is not None:
        image_quality.fold(x_nhwc, head['mean'] if head['mean'] is not None else head['sample'], channel_last=True)
    kl_ln = ops.StackFn.apply(*td['kl'])
    kl_sep, kl_avg, _ = K.kl_bookkeeping_fwd(kl_ln, float(model.free_bits))
    elbo_sep, _ = K.elbo_loss_fwd(ll, kl_sep, zero, 1.0)
    return elbo_sep, ll, kl_sep, kl_avg


@torch.no_grad()
def iw_log_likelihood(model, x, n_samples, use_graph=None):
    """Returns (iw_bound (N,), elbo_mean (N,)): the S-sample importance-weighted bound and the mean single-sample ELBO.

    The bottom-up pass runs once; one sample = top-down pass + likelihood + KL bookkeeping + an ONLINE update of the per-image
    (max, sum exp, sum) state. With on-device Philox noise that sample is captured once as a hipGraph and replayed (passes.replay_loop;
    the RNG step counter is advanced inside the graph): ~1.5 k launches x S without host work, which is what makes S = 1000 practical.
    use_graph=None: graph when the noise source is PhiloxNoise and S >= 8; a replayed noise tape (parity tests) runs eagerly."""
    from .noise import PhiloxNoise
    with eval_mode(model):
        if not x.is_cuda:
            raise K._C.LvaeHipError("iw_log_likelihood needs a GPU tensor")
        bu_values, x_nhwc = _test_bottom_up(model, x)
        N, dev = x.shape[0], x.device
        state = torch.empty((3, N), dtype=torch.float32, device=dev)
        zero = torch.zeros(1, device=dev)
        K.iw_online(state, 0)

        def one_sample():
            K.iw_online(state, 1, elbo=_elbo_sample(model, bu_values, x_nhwc, zero)[0])
            model.noise.end()

        if use_graph is None:
            use_graph = isinstance(model.noise, PhiloxNoise) and n_samples >= 8
        replay_loop(one_sample, n_samples, use_graph)
        iw = torch.empty((N,), dtype=torch.float32, device=dev)
        mean = torch.empty((N,), dtype=torch.float32, device=dev)
        K.iw_online(state, 2, S=n_samples, iw=iw, mean=mean)
        return iw, mean


def reduce_eval_sums(tot, process_group=None):
    """Per-rank sums of this rank's shard ([sum of IW bounds, sum of ELBOs, image count], or test_pass's totals) -> totals over all
    ranks (one all-reduce)."""
    if torch.distributed.is_initialized() and torch.distributed.get_world_size(process_group) > 1:
        torch.distributed.all_reduce(tot, group=process_group)
    return tot


@torch.no_grad()
def evaluate(model, batches, n_samples, process_group=None):
    """Mean ELBO and IW bound over an iterable of image batches (each rank passes ITS shard of the test set)."""
    tot = torch.zeros(3, dtype=torch.float64, device=next(model.parameters()).device)
    for x in batches:
        iw, elbo = iw_log_likelihood(model, x.to(tot.device), n_samples)
        tot[0] += iw.double().sum()
        tot[1] += elbo.double().sum()
        tot[2] += x.shape[0]
    tot = reduce_eval_sums(tot, process_group)
    n = float(tot[2])
    return {'elbo/elbo': float(tot[1]) / n, 'elbo/elbo_IW_%d' % n_samples: float(tot[0]) / n, 'n_images': int(n)}


class _EvalWeights:
    """Context of a test pass: every convolution transforms its own weights (the transformed-weight table pinned by a captured training
    step, and the stamps of its entries, are left exactly as they were), and entries the pass registered are taken out of the table again.
    Their scratch buffers go to `keep`: an evaluation graph captured meanwhile holds their addresses."""

    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        P = K.prepared
        self.saved = (dict(P.entries), P.table, P.enabled)
        P.enabled = False
        return self

    def __exit__(self, *exc):
        P = K.prepared
        entries, table, enabled = self.saved
        self.keep.extend(e['U'] for k, e in P.entries.items() if entries.get(k) is not e)
        P.entries, P.table, P.enabled = entries, table, enabled
        return False


def _bn_recal(model, source):
    """The context of a pass on the averaged weights: nothing (None) without a source, else recalibrate.recalibrated on source()."""
    if source is None:
        return contextlib.nullcontext()
    from .recalibrate import recalibrated
    return recalibrated(model, source(), step=model.global_step)


def _test_sample(model, bu_values, x_nhwc, state, zero, latent_stats=None, image_quality=None):
    """_elbo_sample, folded into the per-image state of a test pass (lvae_eval_online_f32)."""
    K.eval_online(state, model.n_layers, 1, *_elbo_sample(model, bu_values, x_nhwc, zero, latent_stats, image_quality))
    model.noise.end()


class _TestGraphs:
    """The bottom-up pass and one sample of a test batch shape, captured once and replayed for every batch of that shape, in this and in
    later test passes. Static input x and per-image state; a capture stream of its own (so its scratch workspace is its own too).
    With latent_stats and / or image_quality a second sample graph, which also holds the folds into those objects' accumulators (the L folds
    of the latent statistics, the quality launches), is captured into the same pool: the pass replays it for the first sample of a batch and
    the plain one for the rest."""

    def __init__(self, model, x, noise, latent_stats=None, image_quality=None):
        from .noise import PhiloxNoise
        dev = x.device
        self.noise, self.keep, self.latent_stats, self.image_quality = noise, [], latent_stats, image_quality
        hooks = [h for h in (latent_stats, image_quality) if h is not None]
        self.stream = torch.cuda.Stream(device=dev, priority=-1)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        L = model.n_layers
        with torch.cuda.stream(self.stream), _EvalWeights(self.keep):
            self.x = x.clone()
            self.state = torch.empty(5 * x.shape[0] + L, dtype=torch.float64, device=dev)
            self.zero = torch.zeros(1, device=dev)
            # one eager pass with a throw-away noise source: lazy initialisation and scratch growth happen outside the capture, and the
            # caller's noise stream is not advanced by it
            model.noise = PhiloxNoise(0)
            bu, x_nhwc = _test_bottom_up(model, self.x)
            K.eval_online(self.state, L, 0)
            _test_sample(model, bu, x_nhwc, self.state, self.zero)
            if hooks:   # the folds' scratch grows here too; what this throw-away sample added is taken out again
                sums = [h.buf.clone() for h in hooks]
                _test_sample(model, bu, x_nhwc, self.state, self.zero, latent_stats, image_quality)
                for h, was in zip(hooks, sums):
                    h.buf.copy_(was)
                del sums
            model.noise = noise
            noise.begin(dev)          # its device step counter exists before the capture
            del bu, x_nhwc
            torch.cuda.synchronize(dev)
            self.g_bu = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_bu, stream=self.stream, capture_error_mode='thread_local'):
                self.bu, self.x_nhwc = _test_bottom_up(model, self.x)
            self.g_sample = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.g_sample, pool=self.g_bu.pool(), stream=self.stream, capture_error_mode='thread_local'):
                _test_sample(model, self.bu, self.x_nhwc, self.state, self.zero)
            self.g_sample_stats = None
            if hooks:
                self.g_sample_stats = torch.cuda.CUDAGraph()
                with torch.cuda.graph(self.g_sample_stats, pool=self.g_bu.pool(), stream=self.stream, capture_error_mode='thread_local'):
                    _test_sample(model, self.bu, self.x_nhwc, self.state, self.zero, latent_stats, image_quality)
            self.keep.append(K.workspace(0, dev))   # the scratch buffer the captured launches use

    def run(self, x, n_samples, totals, L):
        cur = torch.cuda.current_stream(x.device)
        self.stream.wait_stream(cur)
        with torch.cuda.stream(self.stream):
            self.x.copy_(x)
            K.eval_online(self.state, L, 0)
            self.g_bu.replay()
            for s in range(n_samples):
                (self.g_sample_stats if s == 0 and self.g_sample_stats is not None else self.g_sample).replay()
            if self.latent_stats is not None:
                self.latent_stats.count(x.shape[0])
            K.eval_totals(self.state, L, n_samples, totals)
        cur.wait_stream(self.stream)


@torch.no_grad()
def test_pass(model, batches, n_samples, noise=None, process_group=None, use_graph=None, optimizer=None, latent_stats=None, bn_recal=None,
              image_quality=None):
    """The reference's test summaries over an iterable of NCHW image batches (each rank passes ITS shard of the test set): means over images
    and samples of 'elbo/elbo', 'elbo/recons', 'elbo/kl', 'kl_layers/kl_layer_<i>', plus 'elbo/elbo_IW_<S>' when S > 1, and 'n_images'.

    Eval mode: bottom-up once per batch, S top-down samples folded on the device (lvae_eval_online_f32), each batch added to a double
    accumulator (lvae_eval_totals_f64); one all-reduce of the totals over ranks and one device-to-host copy per pass. The noise comes from
    `noise` (default: a PhiloxNoise of the model's own, `model.test_noise`, whose stream continues from pass to pass), never from
    `model.noise`; dropout is off and BatchNorm statistics are only read, so a test pass leaves training exactly as it was.
    use_graph=None: with on-device Philox noise, bottom-up and one sample are captured once per batch shape and replayed; a replayed
    noise tape (parity tests) runs eagerly.
    optimizer: when it keeps an average of the weights (Adamax(ema_decay > 0)) the whole pass runs inside `optimizer.swap_ema()`, on the
    averaged weights, and the result says so ('weights': 'ema'). The exchange is in place, so the captured graphs of earlier passes read
    the current average when they are replayed, and the parameters are back, bit for bit, when the pass returns.
    latent_stats: a latent.LatentStats. The FIRST sample of every batch (one ancestral sample per image) also folds every layer's p and q
    parameters into it; the pass ends with its `take()` (a collective, like the all-reduce of the totals) and the result gains the
    'latent/*' counts and 'latent_arrays' (per layer 'kl', 'mu_mean', 'mu_var' as (Z, h, w) arrays). Every other key is bit for bit what the
    pass returns without it: the folds draw no noise and write nothing the pass reads.
    image_quality: a quality.ImageQuality. The FIRST sample of every batch also judges the head's mean (its sample where the head has no
    mean) against x and folds mse, PSNR and SSIM into it; the pass ends with its `take()` (a collective) and the result gains the
    'quality/*' means. Every other key is bit for bit what the pass returns without it, and without it the pass issues exactly the launches
    it issues otherwise. One first-sample graph holds whichever of latent_stats and image_quality are present.
    bn_recal (--ema-bn-batches; read only on the averaged weights): a callable returning image batches. Inside `swap_ema()` the BatchNorm
    statistics are first recalibrated on them (recalibrate.recalibrated, its noise stream placed at model.global_step), the pass reads the
    recalibrated statistics, and the live ones are back before the weights are; the result gains 'bn_recal/rounds'."""
    if optimizer is not None and getattr(optimizer, 'ema_decay', 0.0) > 0.0:
        with optimizer.swap_ema(), _bn_recal(model, bn_recal) as recal:
            res = test_pass(model, batches, n_samples, noise=noise, process_group=process_group, use_graph=use_graph,
                            latent_stats=latent_stats, image_quality=image_quality)
        res['weights'] = 'ema'
        if recal is not None:
            res['bn_recal/rounds'] = recal['rounds']
        return res
    from .noise import PhiloxNoise
    dev = next(model.parameters()).device
    if noise is None:
        if getattr(model, 'test_noise', None) is None:
            model.test_noise = PhiloxNoise(seed=(model.noise.seed if isinstance(model.noise, PhiloxNoise) else 0) ^ 0x7E57)
            start = model.__dict__.pop('test_noise_start', None)   # a resumed run (checkpoint.load_checkpoint): the stream goes on
            if start:
                model.test_noise.step = torch.full((1,), int(start), dtype=torch.int64, device=dev)
        noise = model.test_noise
    if use_graph is None:
        use_graph = isinstance(noise, PhiloxNoise)
    L = model.n_layers
    totals = torch.zeros(5 + L, dtype=torch.float64, device=dev)
    if latent_stats is not None:
        latent_stats.reset()
    if image_quality is not None:
        image_quality.reset()
    with eval_mode(model, noise):
        if use_graph:
            plans = model.__dict__.setdefault('_test_graphs', {})
            for x in batches:
                x = x.to(dev).contiguous().float()
                key = (tuple(x.shape), id(noise), noise.seed, id(model.pack()), model.compute_dtype,
                       None if latent_stats is None else id(latent_stats)) + (() if image_quality is None else (id(image_quality),))
                plan = plans.get(key)
                if plan is None or plan.noise is not noise or plan.latent_stats is not latent_stats or plan.image_quality is not image_quality:
                    plan = plans[key] = _TestGraphs(model, x, noise, latent_stats, image_quality)
                plan.run(x, n_samples, totals, L)
        else:
            keep = []
            with _EvalWeights(keep):
                zero = torch.zeros(1, device=dev)
                for x in batches:
                    x = x.to(dev).contiguous().float()
                    state = torch.empty(5 * x.shape[0] + L, dtype=torch.float64, device=dev)
                    K.eval_online(state, L, 0)
                    bu, x_nhwc = _test_bottom_up(model, x)
                    for s in range(n_samples):
                        _test_sample(model, bu, x_nhwc, state, zero, latent_stats if s == 0 else None, image_quality if s == 0 else None)
                    if latent_stats is not None:
                        latent_stats.count(x.shape[0])
                    K.eval_totals(state, L, n_samples, totals)
            torch.cuda.current_stream(dev).synchronize()   # (the registered scratch buffers of this pass may go now)
    tot = reduce_eval_sums(totals, process_group).cpu().tolist()
    n = tot[4]
    res = {'elbo/elbo': tot[1] / n, 'elbo/recons': tot[2] / n, 'elbo/kl': tot[3] / n}
    for i in range(L):
        res['kl_layers/kl_layer_%d' % i] = tot[5 + i] / n
    if n_samples > 1:
        res['elbo/elbo_IW_%d' % n_samples] = tot[0] / n
    res['n_images'] = int(n)
    if latent_stats is not None:
        lat = latent_stats.take(process_group)
        res.update((k, v) for k, v in lat.items() if k.startswith('latent/'))
        res['latent_arrays'] = lat['arrays']
    if image_quality is not None:
        res.update((k, v) for k, v in image_quality.take(process_group).items() if k.startswith('quality/'))
    return res


@torch.no_grad()
def prior_samples(model, n_imgs, temperature=None):
    """evaluate.py:34-36: unconditional samples, (n, C, H, W) in [0, 1]. temperature: as in LadderVAE.sample_prior (None: the plain call)."""
    with eval_mode(model):
        return model.sample_prior(n_imgs, temperature=temperature)


@torch.no_grad()
def conditional_samples(model, x, n_top_layers, n_samples, temperature=None, use_mode=False):
    """K = n_samples variations of every image of the NCHW batch x that keep its top n_top_layers latents (LadderVAE.sample_conditional,
    eval mode) -> (x, pictures), both on the device: pictures (K * B, C, H, W), sample-major, the likelihood's mean where it has one and
    its sample otherwise (the rule of `reconstructions`). Noise comes from `model.noise`."""
    with eval_mode(model):
        x = x.to(next(model.parameters()).device).contiguous().float()
        out = model.sample_conditional(x, n_top_layers, n_samples, temperature=temperature, use_mode=use_mode)
        return x, (out['mean'] if out['mean'] is not None else out['sample'])


@torch.no_grad()
def interpolations(model, x_a, x_b, n_steps=8, n_top_layers=None, mode='slerp', temperature=None):
    """The path between the images of the NCHW batches x_a and x_b in the latents of the top n_top_layers layers (LadderVAE.interpolate at
    the posterior means, eval mode) -> (x_a, x_b, pictures), all on the device: pictures (T * B, C, H, W), step-major, the likelihood's mean
    where it has one and its sample otherwise (the rule of `reconstructions`). Noise comes from `model.noise`."""
    with eval_mode(model):
        dev = next(model.parameters()).device
        x_a, x_b = x_a.to(dev).contiguous().float(), x_b.to(dev).contiguous().float()
        out = model.interpolate(x_a, x_b, n_steps=n_steps, n_top_layers=n_top_layers, mode=mode, temperature=temperature)
        return x_a, x_b, (out['mean'] if out['mean'] is not None else out['sample'])


MASK_KINDS = ('left', 'right', 'top', 'bottom', 'center', 'random')


def make_mask(kind, frac, shape, seed=0):
    """A mask of OBSERVED pixels on the host: bool, `shape` = (..., H, W), True = observed. `left`, `right`, `top`, `bottom` hide that strip
    of round(frac * W) columns / round(frac * H) rows; `center` hides the centred round(frac * H) x round(frac * W) box; `random` hides each
    pixel independently with probability frac, from torch.Generator().manual_seed(seed). ValueError for an unknown kind, a frac outside
    [0, 1] or a shape of fewer than two dimensions."""
    if kind not in MASK_KINDS:
        raise ValueError("mask kind must be one of %s, got %r" % (MASK_KINDS, kind))
    frac = float(frac)
    if not 0.0 <= frac <= 1.0:
        raise ValueError("frac must be in [0, 1], got %r" % (frac,))
    shape = tuple(int(s) for s in shape)
    if len(shape) < 2:
        raise ValueError("shape must end in (H, W), got %s" % (shape,))
    H, W = shape[-2:]
    if kind == 'random':
        return torch.rand(shape, generator=torch.Generator().manual_seed(int(seed))) >= frac
    mask = torch.ones(shape, dtype=torch.bool)
    h, w = int(round(frac * H)), int(round(frac * W))
    if kind == 'left':
        mask[..., :, :w] = False
    elif kind == 'right':
        mask[..., :, W - w:] = False
    elif kind == 'top':
        mask[..., :h, :] = False
    elif kind == 'bottom':
        mask[..., H - h:, :] = False
    else:
        top, left = (H - h) // 2, (W - w) // 2
        mask[..., top:top + h, left:left + w] = False
    return mask


@torch.no_grad()
def inpaintings(model, x, mask, n_iters=10, init='zeros', final='sample', use_graph=None):
    """The images of the NCHW batch x completed where mask (bool or uint8, (B,H,W) or (B,1,H,W); True = observed) hides them
    (LadderVAE.inpaint) -> (x, shown, completed, ll_observed, first), all on the device: `shown` is what the model was given to look at, x
    with the missing pixels at 0.5 (a picture for the eye: the chain itself starts from `first`, x with `init` at the missing pixels);
    ll_observed (n_iters, B). Noise: `model.noise`."""
    dev = next(model.parameters()).device
    x, mask = x.to(dev).contiguous().float(), mask.to(dev)
    out = model.inpaint(x, mask, n_iters=n_iters, init=init, final=final, return_history=True, use_graph=use_graph)
    m = K.pixel_mask(mask, x.shape[0], x.shape[2], x.shape[3], dev)
    return x, K.mask_select(x, 0.5, m, True), out['completed'], out['ll_observed'], out['history'][0]


@torch.no_grad()
def inspect_layer_repr(model, n=8):
    """evaluate.py:95-114: for every layer i, n calls of `sample_prior(n, mode_layers=range(i), constant_layers=range(i+1, L))`
    concatenated — each call (one row of the reference's image grid) draws the layers above i once for its whole batch, samples
    layer i per image and takes the mode below, so a row shows what layer i encodes. Returns a list of L tensors (n*n, C, H, W);
    the reference writes each as a PNG grid with nrow = n (images.image_grid + write_png; the CLI does so under --img-dir)."""
    with eval_mode(model):
        out = []
        for i in range(model.n_layers):
            mode_layers = range(i)
            constant_layers = range(i + 1, model.n_layers)
            rows = [model.sample_prior(n, mode_layers=mode_layers, constant_layers=constant_layers) for _ in range(n)]
            out.append(torch.cat(rows))
        return out


@torch.no_grad()
def reconstructions(model, x):
    """One eval-mode forward pass of the NCHW batch x -> (x, recon), both NCHW on the device: recon is the likelihood's mean where it has
    one and its sample otherwise (the logistic mixture has no mean), boilr's order of preference. Noise comes from `model.noise`."""
    with eval_mode(model):
        x = x.to(next(model.parameters()).device).contiguous().float()
        out = model(x)
        return x, (out['out_mean'] if out['out_mean'] is not None else out['out_sample'])


@torch.no_grad()
def reconstruction_quality(model, batches):
    """mse, PSNR and SSIM of `reconstructions` over an iterable of NCHW batches, folded on the device -> ImageQuality.take()'s dict."""
    from .quality import ImageQuality
    quality = ImageQuality(next(model.parameters()).device)
    for x in batches:
        quality.fold(*reconstructions(model, x))
    return quality.take()


@torch.no_grad()
def quality_ladder(model, batches, temperature=0.0):
    """Reconstruction quality as a function of how many top layers come from the posterior: for every k from 0 to L the top k layers take
    their posterior means and the layers below draw from the prior at `temperature` (0.0, the default: the prior means, so the curve is
    deterministic): LadderVAE.sample_conditional(x, k, 1, temperature, use_mode=True), batch by batch over `batches` (a sequence of NCHW
    batches, walked once per k). The likelihood's mean, or its sample where it has none, is judged against x on the device
    (quality.ImageQuality) -> float64 array (L + 1, 3): the means over images of mse, PSNR (over the images where it is finite) and SSIM."""
    from .quality import ImageQuality
    dev = next(model.parameters()).device
    quality = ImageQuality(dev)
    rows = np.empty((model.n_layers + 1, 3), dtype=np.float64)
    with eval_mode(model):
        for k in range(model.n_layers + 1):
            for x in batches:
                x = x.to(dev).contiguous().float()
                out = model.sample_conditional(x, k, 1, temperature=temperature, use_mode=True)
                quality.fold(x, out['mean'] if out['mean'] is not None else out['sample'])
            res = quality.take()
            rows[k] = res['quality/mse'], res['quality/psnr'], res['quality/ssim']
    return rows


@torch.no_grad()
def nearest_neighbours(model, table, queries, k, space='pixel', n_top_layers=None, shown=12, batch_size=256):
    """Each query image beside its k nearest images of `table` (a device tensor (N, C, H, W), uint8 or float32, searched where it lies).
    queries: {name: NCHW images, host or device}. space 'pixel': squared L2 distance between images; 'latent': between the posterior means
    of the top n_top_layers layers (neighbours.latent_features of table and queries). Returns {name: {'rows' (n, 1 + k, C, H, W): the first
    `shown` queries, each followed by its neighbours, nearest first; 'index' (n, k); 'dist' (n, k); 'nearest': every query's nearest
    distance}, 'summary': neighbours.closeness_summary of the first two query sets' nearest distances}."""
    from .neighbours import NeighbourIndex, closeness_summary, latent_features
    if space not in ('pixel', 'latent'):
        raise ValueError("space must be 'pixel' or 'latent', got %r" % (space,))
    pixels = NeighbourIndex(table)
    dev = table.device
    if space == 'latent':
        feats = torch.cat([latent_features(model, pixels.rows(torch.arange(lo, min(lo + batch_size, pixels.N), device=dev)), n_top_layers,
                                           batch_size) for lo in range(0, pixels.N, batch_size)])
        search = NeighbourIndex(feats)
    else:
        search = pixels
    res = {}
    for name, x in queries.items():
        x = x.to(dev).contiguous().float()
        q = latent_features(model, x, n_top_layers, batch_size) if space == 'latent' else x
        index, dist = search.query(q, k)
        n = min(int(shown), int(x.shape[0]))
        rows = torch.cat((x[:n].unsqueeze(1), pixels.rows(index[:n])), 1).contiguous()
        res[name] = {'rows': rows, 'index': index[:n], 'dist': dist[:n], 'nearest': dist[:, 0]}
    names = list(queries)
    if len(names) >= 2:
        res['summary'] = closeness_summary(res[names[0]]['nearest'], res[names[1]]['nearest'])
    return res


IMAGE_NOISE_TAG = 0x1A6E5      # the picture noise stream's seed is the model's seed with these bits flipped
IMAGE_NOISE_STRIDE = 1 << 20   # and its counter starts at step * this: the pictures of two steps never share a draw


@torch.no_grad()
def image_pass(model, nrows, x=None, step=0, optimizer=None, bn_recal=None):
    """The trainer's pictures -> (sample grid, reconstruction grid or None), uint8 (Hg, Wg, 3) device tensors (images.image_grid).

    The sample grid holds nrows^2 prior samples; with x (an NCHW batch) the reconstruction grid holds min(nrows^2 // 2, len(x)) input /
    reconstruction pairs, nrows pictures per row. Eval mode, convolutions transform their own weights (_EvalWeights), eager launches; with
    an averaging optimizer the pass runs on the averaged weights (`optimizer.swap_ema()`). Noise comes from a fresh PhiloxNoise made from
    the model's seed and `step`, never from `model.noise` or `model.test_noise`: the pictures of step N do not depend on what ran before,
    so a resumed run writes the same ones. On return training mode, `model.noise` and the prepared-weight table are as they were.
    bn_recal: as in test_pass; the pictures of the averaged weights are then made with recalibrated BatchNorm statistics."""
    if optimizer is not None and getattr(optimizer, 'ema_decay', 0.0) > 0.0:
        with optimizer.swap_ema(), _bn_recal(model, bn_recal):
            return image_pass(model, nrows, x, step)
    from .images import image_grid
    from .noise import PhiloxNoise
    dev = next(model.parameters()).device
    noise = PhiloxNoise(0)
    noise.seed = (model.noise.seed if isinstance(model.noise, PhiloxNoise) else 0) ^ IMAGE_NOISE_TAG
    noise.step = torch.full((1,), int(step) * IMAGE_NOISE_STRIDE, dtype=torch.int64, device=dev)
    nrows = int(nrows)
    keep = []
    with eval_mode(model, noise):
        with _EvalWeights(keep):
            sample_grid = image_grid(model.sample_prior(nrows * nrows), nrows)
            recon_grid = None
            n = 0 if x is None else min(nrows * nrows // 2, int(x.shape[0]))
            if n > 0:
                xin, rec = reconstructions(model, x[:n])
                recon_grid = image_grid(xin, nrows, second=rec)
        torch.cuda.current_stream(dev).synchronize()   # (the registered scratch buffers of this pass may go now)
    return sample_grid, recon_grid


def build_eval_parser():
    from .experiment.experiment_manager import build_parser
    p = build_parser()
    p.add_argument('--ll', action='store_true', help='importance-weighted log-likelihood')
    p.add_argument('--ps', action='store_true', help='prior samples -> prior_samples.npy')
    p.add_argument('--layer-repr', action='store_true', dest='layer_repr', help='layer inspection -> layer_repr_<i>.npy')
    p.add_argument('--checkpoint', type=str, default='', help='state_dict file (reference key scheme)')
    p.add_argument('--n-test', type=int, default=1000)
    p.add_argument('--ema', action='store_true', help="evaluate the averaged weights stored in --checkpoint (its 'ema' entry)")
    # (--img-dir DIR is a flag of build_parser: here samples_0.png with --ps, sample_mode_layer<i>.png with --layer-repr)
    p.add_argument('--recons', action='store_true', help='inputs beside their reconstructions -> DIR/reconstructions.png (needs --img-dir)')
    # (--latent-stats and its two thresholds are flags of build_parser: here with --ll, and the arrays go to latent_stats.npz)
    p.add_argument('--temperature', type=float, nargs='+', default=None, metavar='T',
                   help='temperature of the prior draws of --ps, --cond-samples and --interp: one value, or one per layer (bottom layer first)')
    p.add_argument('--recalibrate-bn', choices=('data', 'prior'), default=None, dest='recalibrate_bn',
                   help='re-estimate the BatchNorm running statistics once, before the requested outputs, for the weights that were loaded '
                        '(with --ema: the averaged ones). data: on the first --recalibrate-batches batches of --batch-size images of the '
                        "training split (key 'data' of --data-npz, or the data set of -d). prior: on that many train-mode top-down passes "
                        'of --batch-size rows from the prior at --temperature (one value), for --ps, --layer-repr, --cond-samples, --interp, --nn')
    p.add_argument('--recalibrate-batches', type=int, default=20, dest='recalibrate_batches', metavar='N')
    p.add_argument('--cond-samples', action='store_true', dest='cond_samples',
                   help='variations of the evaluation images that keep their top k latents -> cond_samples_top<k>.npy')
    p.add_argument('--cond-layers', type=int, nargs='+', default=None, dest='cond_layers', metavar='k',
                   help='the k of --cond-samples (default: every k from 0 to the number of layers)')
    p.add_argument('--cond-variations', type=int, default=7, dest='cond_variations', metavar='K', help='variations per image and k')
    p.add_argument('--interp', action='store_true',
                   help='paths between pairs of evaluation images in the latents of their top k layers -> interp_top<k>.npy')
    p.add_argument('--interp-layers', type=int, nargs='+', default=None, dest='interp_layers', metavar='k',
                   help='the k of --interp (default: the number of layers)')
    p.add_argument('--interp-steps', type=int, default=8, dest='interp_steps', metavar='T', help='steps of a path, both ends included')
    p.add_argument('--interp-mode', choices=('slerp', 'lerp'), default='slerp', dest='interp_mode', help='spherical or linear')
    p.add_argument('--inpaint', action='store_true', help='complete the hidden part of the evaluation images -> inpaint_<kind>.npy')
    p.add_argument('--inpaint-mask', nargs='+', default=['left'], dest='inpaint_mask', metavar='KIND',
                   help='what is hidden: %s' % ', '.join(MASK_KINDS))
    p.add_argument('--inpaint-frac', type=float, default=0.5, dest='inpaint_frac', metavar='F', help='the hidden share, in (0, 1)')
    p.add_argument('--inpaint-iters', type=int, default=10, dest='inpaint_iters', metavar='N', help='rounds of the chain')
    p.add_argument('--inpaint-init', choices=('zeros', 'mean', 'noise'), default='zeros', dest='inpaint_init',
                   help='the first completion at the missing pixels')
    p.add_argument('--inpaint-final', choices=('sample', 'mean'), default='sample', dest='inpaint_final',
                   help="the missing pixels after the last round: the draw, or the likelihood's mean")
    p.add_argument('--quality-ladder', action='store_true', dest='quality_ladder',
                   help='mse, PSNR and SSIM of the evaluation images rebuilt from the posterior means of their top k layers, the layers below '
                        'at the prior (--temperature, one value; default 0: the prior mean), for every k from 0 to the number of layers '
                        '-> one line per k and quality_ladder.npy (L + 1, 3)')
    # (--image-quality is a flag of build_parser: here with --ll, PSNR and SSIM after the test line)
    p.add_argument('--nn', action='store_true',
                   help='prior samples and evaluation images beside their nearest table images -> nn_<space>_<samples|heldout>.npy')
    p.add_argument('--nn-k', type=int, default=7, dest='nn_k', metavar='K', help='neighbours per query, 1 to %d' % K.NN_MAX_K)
    p.add_argument('--nn-space', choices=('pixel', 'latent'), default='pixel', dest='nn_space',
                   help='where the distance is taken: the pixels, or the posterior means of the top --nn-layers layers')
    p.add_argument('--nn-layers', type=int, default=None, dest='nn_layers', metavar='k',
                   help='the top layers of --nn-space latent (default: the number of layers)')
    p.add_argument('--nn-table', type=str, default='', dest='nn_table', metavar='FILE.npz',
                   help="the images searched: key 'data', uint8 or float (N, C, H, W); default: a seeded synthetic set")
    p.add_argument('--nn-table-size', type=int, default=4096, dest='nn_table_size', metavar='N',
                   help='images of the synthetic table (drawn from seed + 1) when there is no --nn-table')
    # (--binarize is a flag of build_parser: here it gives the evaluation images their fixed binarization, data.binarize_fixed)
    p.add_argument('--spectral-norms', action='store_true', dest='spectral_norms',
                   help="the spectral norm of every convolution weight (50 power iterations on the device): sum, max and the five largest "
                        'are printed, all of them written to spectral_norms.npz; with --ema, of the averaged weights')
    p.add_argument('--binarize-seed', type=int, default=None, dest='binarize_seed', metavar='S',
                   help="the seed of --binarize's fixed binarization (default: the one noted in --checkpoint's 'augment' record, else 0)")
    return p


def _nn_table_shape(path):
    """(N, C, H, W) of the 'data' array of an .npz without reading the array (the .npy header inside the archive)."""
    import zipfile
    with zipfile.ZipFile(path) as z, z.open('data.npy') as f:
        version = np.lib.format.read_magic(f)
        shape, _, _ = np.lib.format.read_array_header_1_0(f) if version == (1, 0) else np.lib.format.read_array_header_2_0(f)
    return tuple(int(s) for s in shape)


def parse_eval_args(argv=None):
    p = build_eval_parser()
    args = p.parse_args(argv)
    if args.hflip or args.dequantize:
        p.error('--hflip and --dequantize augment training batches: evaluation has none (--binarize fixes a binarization of the images)')
    # here --binarize is about the evaluation images, not about a device-fed training run: kept apart from the trainer's flag
    args.eval_binarize, args.binarize = args.binarize, False
    if args.eval_binarize:
        from .experiment.experiment_manager import DATASETS
        if (args.likelihood or DATASETS[args.dataset_name][2]) != 'bernoulli':
            p.error('--binarize makes 0/1 images: it needs --likelihood bernoulli')
    elif args.binarize_seed is not None:
        p.error('--binarize-seed needs --binarize')
    if args.recons and not args.img_dir:
        p.error('--recons needs --img-dir DIR: the picture is written there')
    if args.latent_stats and not args.ll:
        p.error('--latent-stats needs --ll: the statistics are folded during the log-likelihood pass')
    if args.image_quality and not args.ll:
        p.error('--image-quality needs --ll: the reconstructions are measured during the log-likelihood pass')
    if args.quality_ladder and args.temperature is not None and len(args.temperature) != 1:
        p.error('--quality-ladder takes one --temperature for all layers, got %d' % len(args.temperature))
    L = len(args.z_dims)
    if args.cond_layers is None:
        args.cond_layers = list(range(L + 1))
    elif any(k < 0 or k > L for k in args.cond_layers):
        p.error('--cond-layers takes values from 0 to %d (the number of layers), got %s' % (L, args.cond_layers))
    if args.cond_variations < 1:
        p.error('--cond-variations must be at least 1, got %d' % args.cond_variations)
    if args.interp_layers is None:
        args.interp_layers = [L]
    elif any(k < 1 or k > L for k in args.interp_layers):
        p.error('--interp-layers takes values from 1 to %d (the number of layers), got %s' % (L, args.interp_layers))
    if args.interp_steps < 1:
        p.error('--interp-steps must be at least 1, got %d' % args.interp_steps)
    if any(k not in MASK_KINDS for k in args.inpaint_mask):
        p.error('--inpaint-mask takes %s, got %s' % (', '.join(MASK_KINDS), args.inpaint_mask))
    if not 0.0 < args.inpaint_frac < 1.0:
        p.error('--inpaint-frac must be inside (0, 1), got %r' % args.inpaint_frac)
    if args.inpaint_iters < 1:
        p.error('--inpaint-iters must be at least 1, got %d' % args.inpaint_iters)
    if args.inpaint_final == 'mean':
        from .experiment.experiment_manager import DATASETS
        if (args.likelihood or DATASETS[args.dataset_name][2]) == 'discr_log_mix':
            p.error("--inpaint-final mean: the discretized logistic mixture has no mean")
    if args.temperature is not None:
        if len(args.temperature) not in (1, L):
            p.error('--temperature takes one value or one per layer (%d), got %d' % (L, len(args.temperature)))
        if any(not 0.0 <= t < float('inf') for t in args.temperature):
            p.error('--temperature takes finite values >= 0, got %s' % args.temperature)
    if args.recalibrate_bn is not None and args.recalibrate_batches < 1:
        p.error('--recalibrate-batches must be at least 1, got %d' % args.recalibrate_batches)
    if args.recalibrate_bn == 'data' and args.synthetic and not args.data_npz:
        p.error('--recalibrate-bn data needs a training split (--data-npz FILE or a data set); --synthetic has none')
    if args.recalibrate_bn == 'prior' and args.temperature is not None and len(args.temperature) != 1:
        p.error('--recalibrate-bn prior takes one --temperature for all layers, got %d' % len(args.temperature))
    if not 1 <= args.nn_k <= K.NN_MAX_K:
        p.error('--nn-k takes values from 1 to %d, got %d' % (K.NN_MAX_K, args.nn_k))
    if args.nn_layers is None:
        args.nn_layers = L
    elif not 1 <= args.nn_layers <= L:
        p.error('--nn-layers takes values from 1 to %d (the number of layers), got %d' % (L, args.nn_layers))
    if args.nn_table_size < 1:
        p.error('--nn-table-size must be at least 1, got %d' % args.nn_table_size)
    if args.nn and args.nn_table:
        from .experiment.experiment_manager import DATASETS
        try:
            shape = _nn_table_shape(args.nn_table)
        except (OSError, KeyError, ValueError) as e:
            p.error("--nn-table %s: no readable 'data' array (%s)" % (args.nn_table, e))
        if len(shape) != 4 or shape[0] < 1:
            p.error("--nn-table: 'data' must be (N, C, H, W), got %s" % (shape,))
        color_ch, img_size, _ = DATASETS[args.dataset_name]
        if args.nn_space == 'latent' and shape[1:] != (color_ch,) + tuple(img_size):
            p.error('--nn-space latent: the table holds images of %s, the model encodes %s' % (shape[1:], (color_ch,) + tuple(img_size)))
    return args


def _recalibrate_from_args(exp, temperature):
    """--recalibrate-bn of the command line -> the header line that says what the statistics were re-estimated on."""
    from .recalibrate import recalibrate_bn
    args, model = exp.args, exp.model
    n, bs = args.recalibrate_batches, args.batch_size
    weights = 'averaged weights' if args.ema else 'weights'
    if args.recalibrate_bn == 'prior':
        info = recalibrate_bn(model, n_prior=n, prior_batch=bs, temperature=temperature)
        return ('BatchNorm recalibrated for the %s on the prior: %d top-down passes of %d rows at temperature %g (%d BatchNorm layers)'
                % (weights, info['rounds'], bs, 1.0 if temperature is None else temperature, info['n_bn']))
    from .data import first_batches
    channels_last = False
    if args.data_npz:
        train = torch.from_numpy(np.load(args.data_npz)['data'])
    else:
        from .data import DatasetLoader
        from .main import image_table
        try:
            train, channels_last = image_table(DatasetLoader(args).train.dataset)
        except RuntimeError as e:
            raise SystemExit('--recalibrate-bn data: no training split (%s)' % e)
    try:
        batches = first_batches(train, n, bs, channels_last)
    except ValueError as e:
        raise SystemExit('--recalibrate-bn data: %s' % e)
    info = recalibrate_bn(model, batches)
    return ('BatchNorm recalibrated for the %s on data: the first %d batches of %d training images (%d BatchNorm layers)'
            % (weights, info['rounds'], bs, info['n_bn']))


IMG_GRID_N = 12   # the reference's evaluate.py:24


def main(argv=None):
    from .experiment.experiment_manager import LVAEExperiment
    from .images import image_grid, write_png
    from .main import synthetic_batch
    args = parse_eval_args(argv)
    if args.ema and not args.checkpoint:
        raise SystemExit('--ema needs --checkpoint FILE: the averaged weights are read from the file')
    exp = LVAEExperiment(args=args)
    model = exp.model
    ck = None
    if args.checkpoint:
        from .checkpoint import load_checkpoint, load_ema_weights, residual_posterior_record
        # the same weights mean a different model under the other setting: build the model the file describes, whatever the command line says
        model.residual_posterior = residual_posterior_record(torch.load(args.checkpoint, map_location='cpu'))
        if model.residual_posterior:
            print('%s: residual posteriors (conv_in_q predicts offsets from the prior of its layer)' % args.checkpoint)
        if args.ema:
            try:
                ck = load_ema_weights(args.checkpoint, model)
            except ValueError as e:
                raise SystemExit(str(e))
        else:
            ck = load_checkpoint(args.checkpoint, model)
    if args.img_dir:
        os.makedirs(args.img_dir, exist_ok=True)
    temperature = None if args.temperature is None else (args.temperature[0] if len(args.temperature) == 1 else args.temperature)
    if args.recalibrate_bn:   # once, before every output below, for the weights just loaded
        print(_recalibrate_from_args(exp, temperature))
    if args.ll or args.recons or args.cond_samples or args.interp or args.inpaint or args.nn or args.quality_ladder:
        gen = torch.Generator().manual_seed(args.seed)
        if args.data_npz:
            data = torch.from_numpy(np.load(args.data_npz)['data']).float()
        else:
            data = synthetic_batch(exp, args.n_test, gen)
        if args.eval_binarize:   # before any output: one binarization per (seed, image number), the one the run's test lines saw
            from .checkpoint import augment_record
            from .data import binarize_fixed
            seed = args.binarize_seed if args.binarize_seed is not None else int((augment_record(ck) or {}).get('seed', 0))
            data = binarize_fixed(data, seed).float()
            print('evaluation images binarized: fixed, seed %d' % seed)
    del ck
    if args.ll:
        bs = args.test_batch_size
        lat = None
        if args.latent_stats:
            from .latent import LatentStats, latent_line_suffix, save_npz
            lat = LatentStats(model, exp.device, args.latent_kl_threshold, args.latent_var_threshold)
        qual = None
        if args.image_quality:
            from .quality import ImageQuality, quality_line_suffix
            qual = ImageQuality(exp.device)
        res = test_pass(model, (data[i:i + bs] for i in range(0, data.shape[0], bs)), args.loglikelihood_samples, latent_stats=lat,
                        image_quality=qual)
        if args.ema:
            res['weights'] = 'ema'
        line = exp.test_log_str(res, model.global_step)
        if lat is not None:
            line += latent_line_suffix(res, lat.kl_threshold, lat.var_threshold)
            save_npz('latent_stats.npz', res['latent_arrays'], lat.kl_threshold, lat.var_threshold, res['n_images'])
        if qual is not None:
            line += quality_line_suffix(res)
        print(line)
    if args.spectral_norms:
        from .spectral import spectral_norms
        norms = spectral_norms(model, 50, seed=args.seed)
        top = sorted(norms.items(), key=lambda kv: -kv[1])[:5]
        print('spectral norms of %d convolution weights%s: sum %.5g   max %.5g' % (len(norms), ' (averaged weights)' if args.ema else '',
                                                                                 sum(norms.values()), top[0][1]))
        for name, s in top:
            print('    %-60s %.5g' % (name, s))
        np.savez('spectral_norms.npz', names=np.array(list(norms)), sigma=np.array(list(norms.values()), dtype=np.float32))
    if args.ps:
        np.save('prior_samples.npy', prior_samples(model, 64, temperature).cpu().numpy())
    if args.layer_repr:
        for i, s in enumerate(inspect_layer_repr(model, 8)):
            np.save('layer_repr_%d.npy' % i, s.cpu().numpy())
    if args.cond_samples:  # one row per image: the input, then its K variations
        n, nv = min(IMG_GRID_N, int(data.shape[0])), args.cond_variations
        for k in args.cond_layers:
            xin, pics = conditional_samples(model, data[:n], k, nv, temperature)
            rows = torch.cat((xin.unsqueeze(1), pics.view(nv, n, *pics.shape[1:]).transpose(0, 1)), 1).contiguous()
            np.save('cond_samples_top%d.npy' % k, rows.cpu().numpy())
            if args.img_dir:
                write_png(os.path.join(args.img_dir, 'cond_samples_top%d.png' % k), image_grid(rows.view(-1, *rows.shape[2:]), 1 + nv))
    if args.interp:  # one row per pair of images (2i, 2i + 1): x_a, the T steps, x_b
        n, nt = min(IMG_GRID_N, int(data.shape[0]) // 2), args.interp_steps
        if n < 1:
            raise SystemExit('--interp needs at least two evaluation images')
        for k in args.interp_layers:
            xa, xb, pics = interpolations(model, data[0:2 * n:2], data[1:2 * n:2], nt, k, args.interp_mode, temperature)
            rows = torch.cat((xa.unsqueeze(1), pics.view(nt, n, *pics.shape[1:]).transpose(0, 1), xb.unsqueeze(1)), 1).contiguous()
            np.save('interp_top%d.npy' % k, rows.cpu().numpy())
            if args.img_dir:
                write_png(os.path.join(args.img_dir, 'interp_top%d.png' % k), image_grid(rows.view(-1, *rows.shape[2:]), nt + 2))
    if args.inpaint:  # one row per image: the image, what the model was shown, the completion
        from .quality import ImageQuality
        qual = ImageQuality(exp.device)
        n = min(IMG_GRID_N, int(data.shape[0]))
        for j, kind in enumerate(args.inpaint_mask):
            mask = make_mask(kind, args.inpaint_frac, (n,) + tuple(data.shape[2:]), args.seed + j)
            xin, shown, done, ll_obs, first = inpaintings(model, data[:n], mask, args.inpaint_iters, args.inpaint_init, args.inpaint_final)
            rows = torch.stack((xin, shown, done), 1).contiguous()
            np.save('inpaint_%s.npy' % kind, rows.cpu().numpy())
            if args.img_dir:
                write_png(os.path.join(args.img_dir, 'inpaint_%s.png' % kind), image_grid(rows.view(-1, *rows.shape[2:]), 3))
            hidden = (~mask)[:, None].expand_as(data[:n])
            truth = data[:n].float()[hidden].double()
            mse0 = float(((first.cpu()[hidden].double() - truth) ** 2).mean()) if truth.numel() else float('nan')
            mse1 = float(((done.cpu()[hidden].double() - truth) ** 2).mean()) if truth.numel() else float('nan')
            ll_obs = ll_obs.cpu().double()
            # on the device, over the missing pixels (SSIM: the windows whose centre is missing), means over the images
            qual.fold(xin, first, mask.to(xin.device), count='missing')
            q0 = qual.take()
            qual.fold(xin, done, mask.to(xin.device), count='missing')
            q1 = qual.take()
            print('inpaint %s (hidden %.3f, %d rounds): mse on the missing pixels %.5g (initial fill) -> %.5g (completion); '
                  'll_observed %.5g (first round) -> %.5g (last round); PSNR on the missing pixels %.2f dB -> %.2f dB; '
                  'SSIM at the missing centres %.4f -> %.4f'
                  % (kind, float((~mask).float().mean()), args.inpaint_iters, mse0, mse1, float(ll_obs[0].mean()), float(ll_obs[-1].mean()),
                     q0['quality/psnr'], q1['quality/psnr'], q0['quality/ssim'], q1['quality/ssim']))
    if args.nn:  # one row per query: the query, then its K nearest table images, nearest first
        from .data import device_storage
        from .neighbours import closeness_line
        if args.nn_table:
            table = torch.from_numpy(np.load(args.nn_table)['data'])
        else:
            table = synthetic_batch(exp, args.nn_table_size, torch.Generator().manual_seed(args.seed + 1))
        if tuple(table.shape[1:]) != tuple(data.shape[1:]):
            raise SystemExit('--nn: the table holds images of %s, the queries are %s' % (tuple(table.shape[1:]), tuple(data.shape[1:])))
        table = device_storage(table)[0].to(exp.device)
        samples = prior_samples(model, IMG_GRID_N ** 2, temperature)
        res = nearest_neighbours(model, table, {'samples': samples, 'heldout': data[:1000]}, args.nn_k, args.nn_space, args.nn_layers,
                                 shown=IMG_GRID_N)
        for name in ('samples', 'heldout'):
            stem = 'nn_%s_%s' % (args.nn_space, name)
            np.save(stem + '.npy', res[name]['rows'].cpu().numpy())
            np.save(stem + '_index.npy', res[name]['index'].cpu().numpy())
            np.save(stem + '_dist.npy', res[name]['dist'].cpu().numpy())
            if args.img_dir:
                rows = res[name]['rows']
                write_png(os.path.join(args.img_dir, stem + '.png'), image_grid(rows.view(-1, *rows.shape[2:]).contiguous(), 1 + args.nn_k))
        print(closeness_line(args.nn_space, res['summary']))
    if args.quality_ladder:  # one row per k: how much of an image its top k layers hold
        bs = args.test_batch_size
        rows = quality_ladder(model, [data[i:i + bs] for i in range(0, data.shape[0], bs)], 0.0 if temperature is None else temperature)
        np.save('quality_ladder.npy', rows)
        for k, (mse, psnr, ssim) in enumerate(rows):
            print('quality ladder top %d of %d layers: mse %.5g   PSNR %.2f dB   SSIM %.4f' % (k, model.n_layers, mse, psnr, ssim))
    if not args.img_dir:
        return
    # the reference's pictures, after everything above so that the arrays do not depend on --img-dir
    if args.ps:            # evaluate.py:34-36
        write_png(os.path.join(args.img_dir, 'samples_0.png'), image_grid(prior_samples(model, IMG_GRID_N ** 2, temperature), IMG_GRID_N))
    if args.recons:        # evaluate.py:39-41, from the first images of the evaluation data
        xin, rec = reconstructions(model, data[:IMG_GRID_N ** 2 // 2])
        write_png(os.path.join(args.img_dir, 'reconstructions.png'), image_grid(xin, IMG_GRID_N, second=rec))
    if args.layer_repr:    # evaluate.py:95-114
        for i, s in enumerate(inspect_layer_repr(model, IMG_GRID_N)):
            write_png(os.path.join(args.img_dir, 'sample_mode_layer%d.png' % i), image_grid(s.contiguous(), IMG_GRID_N))
    if args.recons:        # after every picture, whose noise draws stay where they were: all evaluation images, not only the 72 shown
        bs = args.test_batch_size
        res = reconstruction_quality(model, (data[i:i + bs] for i in range(0, data.shape[0], bs)))
        print('reconstructions of %d images: mse %.5g   PSNR %.2f dB (of the mean mse: %.2f dB)   SSIM %.4f'
              % (res['n_images'], res['quality/mse'], res['quality/psnr'], res['quality/psnr_of_mean_mse'], res['quality/ssim']))


if __name__ == '__main__':
    main()
