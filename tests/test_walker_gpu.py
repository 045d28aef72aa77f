"""The one top-down walk (LadderVAE._walk) and the scaffolding the evaluation passes share (passes.eval_mode): the parts a refactor gets
wrong are the guards and the ordering, so these pin the seam where rows are repeated, where the walk stops, and what an exception leaves
behind. Calls are counted by wrapping `kernels.call`."""
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

REPEAT = 'lvae_repeat_samples_fwd_f32'
UPSAMPLE = 'lvae_upsample2x_fwd_f32'      # tiny_cifar's final_top_down starts with it, and nothing above the tail issues it
NOISE_END = 'lvae_counter_advance'


@pytest.fixture(scope='module')
def K():
    import lvae_amd  # noqa: F401
    from lvae_amd import kernels
    return kernels


@pytest.fixture(scope='module')
def cifar():
    from lvae_amd.models.lvae import LadderVAE
    from lvae_amd.noise import PhiloxNoise
    g = load_golden('tiny_cifar')
    m = LadderVAE(**g.cfg)
    m.load_state_dict(g.state_dict())
    m.cuda().eval()
    m.noise = PhiloxNoise(seed=5)
    return m, g.t('x').cuda()


def _record_calls(K, monkeypatch):
    names, real = [], K.call
    monkeypatch.setattr(K, 'call', lambda name, *args: (names.append(name), real(name, *args))[1])
    return names


def test_eval_mode_restores_the_flag_and_the_noise_when_the_body_raises(cifar):
    from lvae_amd.evaluate import eval_mode
    from lvae_amd.noise import PhiloxNoise
    m, x = cifar
    own, other = m.noise, PhiloxNoise(seed=9)
    m.train()
    try:
        with pytest.raises(ValueError):
            with eval_mode(m, other):
                assert not m.training and m.noise is other
                m.encode(x, n_top_layers=m.n_layers + 1)
        assert m.training and m.noise is own
        with pytest.raises(ValueError):
            with eval_mode(m):
                assert not m.training and m.noise is own
                m.encode(x, n_top_layers=m.n_layers + 1)
        assert m.training and m.noise is own
        m.eval()
        with eval_mode(m, other):
            assert not m.training and m.noise is other
        assert not m.training and m.noise is own
    finally:
        m.eval()
        m.noise = own


@pytest.mark.parametrize('n_top', ['0', 'L'])
def test_sample_conditional_edges_repeat_once_or_not_at_all(K, cifar, monkeypatch, n_top):
    m, x = cifar
    L, B = m.n_layers, x.shape[0]
    k = 0 if n_top == '0' else L
    names = _record_calls(K, monkeypatch)
    with torch.no_grad():
        one = m.sample_conditional(x, k, 1)
        n_one = names.count(REPEAT)
        del names[:]
        three = m.sample_conditional(x, k, 3)
        n_three = names.count(REPEAT)
    assert n_one == 0, n_one
    # k = L: what the posterior layers hand down is repeated once, in front of the tail; k = 0: nothing is handed down, the top layer
    # broadcasts its prior over the 3 * B rows itself
    assert n_three == (1 if k == L else 0), n_three
    assert one['sample'].shape[0] == B and three['sample'].shape[0] == 3 * B
    assert all(z.shape[0] == (B if k == L else 3 * B) for z in three['z'])
    assert bool(torch.isfinite(three['sample']).all())


def test_sample_conditional_in_between_repeats_once_at_the_seam(K, cifar, monkeypatch):
    m, x = cifar
    L, B = m.n_layers, x.shape[0]
    names = _record_calls(K, monkeypatch)
    with torch.no_grad():
        for k in range(1, L):
            del names[:]
            m.sample_conditional(x, k, 1)
            assert names.count(REPEAT) == 0, k
            del names[:]
            out = m.sample_conditional(x, k, 3)
            assert names.count(REPEAT) == 1, k
            assert [z.shape[0] for z in out['z']] == [3 * B] * (L - k) + [B] * k


def test_encode_of_the_top_layers_launches_nothing_below(K, cifar, monkeypatch):
    m, x = cifar
    L = m.n_layers
    names = _record_calls(K, monkeypatch)
    with torch.no_grad():
        full = m.encode(x)
        all_calls = list(names)
        del names[:]
        m._begin(x)
        m._encode_image(x, need_image=False)
        m.noise.end()
        n_bottom_up = len(names) - 1
        for k in range(1, L):
            del names[:]
            part = m.encode(x, k)
            calls = list(names)
            assert calls[-1] == NOISE_END and all_calls[-1] == NOISE_END
            body = calls[:-1]                      # (noise.end() closes both calls)
            assert n_bottom_up < len(body) < len(all_calls) - 1, (k, n_bottom_up, len(body), len(all_calls))
            assert body == all_calls[:len(body)], k
            assert UPSAMPLE not in body
            assert [z is not None for z in part] == [i >= L - k for i in range(L)]
            for a, b in zip(part, full):
                assert a is None or torch.equal(a, b)
    assert UPSAMPLE not in all_calls              # nor does the full encode run the tail: the walk has nothing to decode
