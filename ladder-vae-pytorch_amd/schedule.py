"""When the trainer tests, estimates the log-likelihood, writes checkpoints and writes pictures (the cadence flags of boilr's trainer:
--ts-log-every, --ll-every / --ll-samples, --checkpoint-every / --keep-checkpoint-max, --ts-img-every). Host logic only."""
import os
import re


class TrainSchedule:
    """at(step) -> (test_samples, checkpoint) for a 1-based training step.

    test_samples: 0 = no test pass; 1 = a test pass (every `test_every` steps); `ll_samples` = a test pass whose summary also carries the
    importance-weighted bound (every `ll_every` steps; it replaces the plain test pass of that step). No test split: never.
    checkpoint: every `checkpoint_every` steps, only when a checkpoint directory was given.
    images_at(step) -> whether sample / reconstruction pictures are due: every `images_every` steps (0 or less: never). Whether they are
    written is the caller's matter (a picture directory; a test split for the reconstructions)."""

    def __init__(self, test_every, ll_every, ll_samples, checkpoint_every, has_test, checkpoint_dir='', images_every=0):
        self.test_every, self.ll_every, self.ll_samples = int(test_every), int(ll_every), max(1, int(ll_samples))
        self.checkpoint_every, self.has_test, self.checkpoint_dir = int(checkpoint_every), bool(has_test), checkpoint_dir
        self.images_every = int(images_every)

    @classmethod
    def from_args(cls, args, has_test):
        return cls(args.test_log_every, args.loglikelihood_every, args.loglikelihood_samples, args.checkpoint_every, has_test,
                   args.checkpoint_dir, images_every=args.test_imgs_every)

    def at(self, step):
        samples = 0
        if self.has_test:
            if self.ll_every > 0 and step % self.ll_every == 0:
                samples = self.ll_samples
            elif self.test_every > 0 and step % self.test_every == 0:
                samples = 1
        ckpt = bool(self.checkpoint_dir) and self.checkpoint_every > 0 and step % self.checkpoint_every == 0
        return samples, ckpt

    def images_at(self, step):
        return self.images_every > 0 and step % self.images_every == 0


CHECKPOINT_RE = re.compile(r'^model_(\d+)\.pt$')


def checkpoint_path(directory, step):
    return os.path.join(directory, 'model_%d.pt' % int(step))


def checkpoints_to_delete(names, keep_max):
    """File names of `names` (model_<step>.pt; others are ignored) that rotation deletes: all but the `keep_max` newest steps.
    keep_max <= 0 keeps everything."""
    found = sorted((int(m.group(1)), n) for n in names for m in [CHECKPOINT_RE.match(n)] if m)
    if keep_max <= 0:
        return []
    return [n for _, n in found[:max(0, len(found) - int(keep_max))]]
