"""Device-fed training steps with the gather augmenting its batch against without, in interleaved pairs (README "Feed augmentation").

Two arms, two captured TrainSteps on ONE model and optimizer (every step of either arm is a real training step of it), each fed by its own
DeviceDataset over the same seeded images (CIFAR10's train size, 8-bit levels, never read from disk):
  plain  TrainStep(feed=DeviceDataset(...)): lvae_batch_gather_f32 inside the captured step;
  aug    the same with augment=FeedAugment(hflip=True, dequantize=True): lvae_batch_gather_aug_f32, two Philox blocks per four pixels.
(The trainer pairs --dequantize with the Gaussian head; the step's cost does not depend on what the pixels mean, so the flagship
configuration is timed as it is.) A pair is one window of `--steps` steps of each arm, plain first, between two device events on the
step's stream; before each window the arm's feed is re-attached to the model, outside the timed part, so that its cursor continues from
the model's step count. Reported: each arm's median over the pairs, the median of the per-pair differences, and the spread of the plain
arm's windows, which is the noise a difference has to exceed.

    python tools/feed_aug_ab.py --out profiles/feed_aug_ab.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd import configs  # noqa: E402
from lvae_amd.data import DeviceDataset, FeedAugment  # noqa: E402

NAME, BATCH = 'cifar15', 256


def make_model(cfg):
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    torch.manual_seed(0)
    model = LadderVAE(**cfg).cuda().train()
    model.noise = PhiloxNoise(seed=42)
    return model, Adamax(model, lr=3e-4)


def window(step, n):
    """ms per step of n steps of one arm, between device events."""
    step.feed.attach(step.model)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def gather_alone_us(ds, reps=200):
    """The gather kernel by itself, eager launches between two device events."""
    out = ds.new_batch()
    for _ in range(10):
        ds.gather(out)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        ds.gather(out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='', help='also write the report to this file')
    ap.add_argument('--pairs', type=int, default=8)
    ap.add_argument('--steps', type=int, default=10, help='steps per window')
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--images', type=int, default=50000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feed_aug_ab.py times training steps on the GPU; there is none here')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    from lvae_amd.engine import TrainStep
    cfg = configs.BY_NAME[NAME]
    shape = (args.images, cfg['color_ch']) + tuple(cfg['img_shape'])
    images = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(1234))
    feeds = {'plain': DeviceDataset(images, BATCH, seed=1234),
             'aug': DeviceDataset(images, BATCH, seed=1234, augment=FeedAugment(hflip=True, dequantize=True))}
    model, opt = make_model(cfg)
    arms = {k: TrainStep(model, opt, use_graph=True, feed=ds) for k, ds in feeds.items()}
    for step in arms.values():                                  # eager warm-up steps, the capture, and a few replays
        window(step, args.warmup)
    times = {k: [] for k in arms}
    for _ in range(args.pairs):
        for k, step in arms.items():
            times[k].append(window(step, args.steps))
    say('device-fed training steps, plain gather vs --hflip --dequantize in the gather: %s, batch %d, %d images, one process, %d interleaved '
        'pairs of %d captured steps per arm, device events (%s)' % (NAME, BATCH, args.images, args.pairs, args.steps, torch.cuda.get_device_name(0)))
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        say('  %-6s median %8.3f ms/step   min %8.3f   max %8.3f   windows: %s' % (k, med[k], min(ts), max(ts), ' '.join('%.3f' % t for t in ts)))
    diffs = [a - p for p, a in zip(times['plain'], times['aug'])]
    spread = max(times['plain']) - min(times['plain'])
    d = statistics.median(diffs)
    say('  aug - plain, median of the per-pair differences: %+.3f ms/step (%+.2f %% of the plain step); spread of the plain windows %.3f ms: %s'
        % (d, 100.0 * d / med['plain'], spread, 'within the spread' if abs(d) <= spread else 'augmenting is SLOWER' if d > 0 else 'augmenting is faster'))
    for k, ds in feeds.items():
        say('  %-6s gather kernel alone, eager: %.1f us per launch' % (k, gather_alone_us(ds)))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
