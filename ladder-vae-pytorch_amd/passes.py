"""What the sampling and evaluation passes share beside the model: the eval-mode context and the warm-up / capture / replay loop."""
import contextlib

import torch


@contextlib.contextmanager
def eval_mode(model, noise=None):
    """Inside: the model in eval mode and, when `noise` is given, drawing from it. On exit the training flag and `model.noise` are what
    they were, also when the body raises."""
    was_training, old_noise = model.training, model.noise
    model.eval()
    if noise is not None:
        model.noise = noise
    try:
        yield model
    finally:
        model.noise = old_noise
        model.train(was_training)


def replay_loop(body, n, use_graph, between=None):
    """body() n times, between(i, result) after iteration i; returns the last result. With use_graph two iterations run eagerly
    (allocator warm-up; they count, also when n < 2: whether a graph is worth it for a small n is the caller's rule), the device is
    synchronized, one iteration is captured as a hipGraph and replayed for the rest: `result` is then what the capture returned, tensors
    the replays write again, so `between` copies what it wants to keep (device copies in stream order; the host does not wait). body must
    issue the same launches every time and advance its own state on the device (the RNG step counter is advanced inside the graph)."""
    res = None
    eager = 2 if use_graph else n
    for i in range(eager):
        res = body()
        if between is not None:
            between(i, res)
    if use_graph:
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, capture_error_mode='thread_local'):
            res = body()
        for i in range(eager, n):
            graph.replay()
            if between is not None:
                between(i, res)
    return res
