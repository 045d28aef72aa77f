"""Host-fed against device-fed training steps, alternating in one process (README "Device-resident data").

Two arms per configuration, two TrainSteps on ONE model and optimizer (every step of either arm is a real training step of it):
  host    the batch as main.py forms it without --device-data: next(iter(DataLoader(TensorDataset, shuffle, drop_last)))[0], the rank's
          slice, .to(device) from pageable memory, TrainStep(x) (which copies it into the graph's input buffer);
  device  TrainStep(feed=DeviceDataset): the gather kernel inside the captured step.
The data set is generated from a seed (CIFAR10's train size: 50,000 images of the model's shape, 8-bit levels, or 0/1 for the Bernoulli
head), never read from disk. Windows of `--steps` steps alternate host, device, host, ... `--rounds` times; every window ends in a device
synchronise and is timed with the host clock; before each of its windows the feed is re-attached to the model (outside the timed part),
so that its cursor continues from the model's step count, which the host-fed steps advanced too. The spread of one arm's windows is the noise a difference between the arms has to exceed.

    python tools/feed_ab.py --out profiles/device_data_ab.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.utils.data import DataLoader, TensorDataset  # noqa: E402

import lvae_amd  # noqa: E402,F401
from lvae_amd import configs  # noqa: E402
from lvae_amd.data import DeviceDataset  # noqa: E402
from lvae_amd.dist import shard_batch  # noqa: E402

CASES = [('cifar15', 256, 20), ('mnist3', 64, 100)]   # (configuration, batch, steps per window unless --steps is given)


def make_images(cfg, n, seed):
    """Seeded uint8 NCHW images of the model's shape: all 256 levels, or 0 / 255 for binary data."""
    g = torch.Generator().manual_seed(seed)
    shape = (n, cfg['color_ch']) + tuple(cfg['img_shape'])
    u = torch.randint(0, 256, shape, dtype=torch.uint8, generator=g)
    return (u > 127).to(torch.uint8) * 255 if cfg['likelihood_form'] == 'bernoulli' else u


def make_model(cfg):
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    from lvae_amd.optim import Adamax
    torch.manual_seed(0)
    model = LadderVAE(**cfg).cuda().train()
    model.noise = PhiloxNoise(seed=42)
    return model, Adamax(model, lr=3e-4)


class HostFeed:
    """The trainer's loop over a DataLoader, one batch per call."""

    def __init__(self, images_u8, batch):
        x = images_u8.float().div_(255.0)                      # what data._cifar10 builds: the float NCHW tensor of a TensorDataset
        self.loader = DataLoader(TensorDataset(x, torch.zeros(x.shape[0], dtype=torch.int64)), batch_size=batch, shuffle=True, drop_last=True)
        self.batches = None
        self.lo, self.hi = shard_batch(batch, 0, 1)

    def next(self):
        if self.batches is None:
            self.batches = iter(self.loader)
        try:
            xb = next(self.batches)[0]
        except StopIteration:
            self.batches = iter(self.loader)
            xb = next(self.batches)[0]
        return xb[self.lo:self.hi]


def window(step, host, n):
    if host is None:
        step.feed.attach(step.model)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if host is None:
        for _ in range(n):
            step()
    else:
        for _ in range(n):
            step(host.next().to('cuda', non_blocking=True))
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def gather_alone_us(ds, reps=200):
    """The gather kernel by itself, eager launches between two device events (launch-latency sized: see the kernel's header)."""
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


def run_case(name, batch, steps, rounds, n_images, warmup, say):
    cfg = configs.BY_NAME[name]
    images = make_images(cfg, n_images, seed=1234)
    ds = DeviceDataset(images, batch, seed=1234)
    host = HostFeed(images, batch)
    from lvae_amd.engine import TrainStep
    model, opt = make_model(cfg)
    arms = {'host': (TrainStep(model, opt, use_graph=True), host), 'device': (TrainStep(model, opt, use_graph=True, feed=ds), None)}
    for step, h in arms.values():                               # eager warm-up steps, the capture, and a few replays
        window(step, h, warmup)
    times = {k: [] for k in arms}
    for _ in range(rounds):
        for k, (step, h) in arms.items():
            times[k].append(window(step, h, steps))
    say('%s, batch %d, %d images (%.1f MB as %s in device memory), %d rounds of %d steps per arm' %
        (name, batch, ds.N, ds.nbytes / 1e6, ds.kind, rounds, steps))
    med = {}
    for k, ts in times.items():
        med[k] = statistics.median(ts)
        say('  %-6s  median %8.3f ms/step   min %8.3f   max %8.3f   windows: %s' %
            (k, med[k], min(ts), max(ts), ' '.join('%.3f' % t for t in ts)))
    spread = max(max(ts) - min(ts) for ts in times.values())
    diff = med['host'] - med['device']
    say('  host - device = %+.3f ms/step (%+.1f %% of the host-fed step); largest spread of one arm\'s windows %.3f ms: %s' %
        (diff, 100.0 * diff / med['host'], spread,
         'device-fed is faster' if diff > spread else 'device-fed is SLOWER' if -diff > spread else 'within the spread'))
    say('  gather kernel alone, eager: %.1f us per launch' % gather_alone_us(ds))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--out', default='', help='also write the report to this file')
    ap.add_argument('--rounds', type=int, default=6)
    ap.add_argument('--steps', type=int, default=0, help='steps per window (0: 20 for cifar15, 100 for mnist3)')
    ap.add_argument('--warmup', type=int, default=8)
    ap.add_argument('--images', type=int, default=50000)
    ap.add_argument('--only', choices=[c[0] for c in CASES], default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('feed_ab.py times training steps on the GPU; there is none here')
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say('host-fed vs device-fed training steps, one process, alternating windows, single rank (%s)' % torch.cuda.get_device_name(0))
    for name, batch, steps in CASES:
        if args.only in (None, name):
            run_case(name, batch, args.steps or steps, args.rounds, args.images, args.warmup, say)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
